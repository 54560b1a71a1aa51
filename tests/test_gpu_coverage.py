"""Coverage and candidate positions on the GPU (include/demux_hip.h "Coverage"): the device against the recorded f10 fixture
and the hand-written table, equal integers everywhere, in both accumulation forms; against the Python restatement on random
reads with every CIGAR operation and on a piled-up problem; the invalid inputs; coexistence with a resident problem and the
records of read counting; detect_snps_positions_from_reads against the reference's recorded detect_snps_positions and against
detect_snps_positions_from_calls."""
import numpy as np
import pandas as pd
import pytest

from demuxalot_amd import (BarcodeHandler, DecodedReads, Demultiplexer, ProbabilisticGenotypes, _lib, count_snps_from_reads,
                           coverage_from_reads, detect_snps_positions_from_calls, detect_snps_positions_from_reads,
                           find_candidate_positions)
from demuxalot_amd.device import DeviceContext, get_context, shared_context_lock
from demuxalot_amd.snp_counter import quality_table
from tests import coverage_restatement as cr
from tests import fixture_io as fio
from tests.test_coverage_cpu import FIXTURE, fixture_reads, threshold_kwargs
from tests.test_gpu_count_reads import random_problem, skewed_problem

pytestmark = pytest.mark.gpu

FORMS = {'atomic': _lib.COVERAGE_ATOMIC, 'tiled': _lib.COVERAGE_TILED}


def device_coverage(reads, start, stop, quality_threshold=15):
    """The window in both accumulation forms (they must agree); the tiled form's is returned and left on the context."""
    got = {}
    with shared_context_lock:
        ctx = get_context()
        for name, form in FORMS.items():
            ctx.set_coverage_form(form)
            got[name] = ctx.coverage_count(DecodedReads(**reads), start, stop, quality_threshold)
    assert got['atomic'].dtype == np.int32 and got['atomic'].shape == (4, stop - start)
    assert np.array_equal(got['atomic'], got['tiled'])
    return got['tiled']


def device_candidates(reads, start, stop, quality_threshold=15, fetch_counts=False, **thresholds):
    thresholds.setdefault('max_snp_candidates', 10000)
    with shared_context_lock:
        ctx = get_context()
        ctx.coverage_count(DecodedReads(**reads), start, stop, quality_threshold, fetch=False)
        return ctx.coverage_candidates(thresholds['minimum_coverage'], thresholds['minimum_alternative_fraction'],
                                       thresholds['minimum_alternative_coverage'], thresholds['minimum_fraction_of_ref_and_alt'],
                                       thresholds['max_snp_candidates'], fetch_counts=fetch_counts)


@pytest.mark.parametrize('case', cr.HAND_TABLE, ids=[case[0] for case in cr.HAND_TABLE])
def test_device_gives_the_hand_written_coverage(case):
    _name, rows, start, stop, quality_threshold, expected = case
    assert np.array_equal(device_coverage(cr.make_reads(rows), start, stop, quality_threshold), expected)


def test_device_equals_the_fixture():
    fx = fio.load(FIXTURE)
    length = int(fx['length'])
    for i in range(len(fx['chroms'])):
        reads = fixture_reads(fx, i)
        assert np.array_equal(device_coverage(reads, 0, length), fx[f'cov{i}'])
        assert np.array_equal(coverage_from_reads(DecodedReads(**reads), 0, length), fx[f'cov{i}'])
        for s, row in enumerate(fx['thresholds']):
            positions, counts = device_candidates(reads, 0, length, fetch_counts=True, **threshold_kwargs(row))
            assert positions.dtype == np.int32 and np.array_equal(positions, fx[f'cand{s}_c{i}'])
            assert np.array_equal(counts, fx[f'cov{i}'][:, positions].T)
    capped = device_candidates(fixture_reads(fx, 0), 0, length, max_snp_candidates=int(fx['cap']), **threshold_kwargs(fx['thresholds'][0]))
    assert np.array_equal(capped, fx['capped_c0'])
    for w, (chrom, start, stop) in enumerate(fx['windows']):
        got = device_candidates(fixture_reads(fx, int(chrom)), int(start), int(stop), **threshold_kwargs(fx['thresholds'][0]))
        assert np.array_equal(got, fx[f'window{w}'] + start)  # absolute, where the reference returned window-relative indices


def test_a_tie_at_the_cut_goes_to_the_higher_position():
    # alt 5, 9, 5, 5 at the positions 101, 103, 105, 107 over a reference base seen 50 times
    rows = [(100, '8M', 'AAAAAAAA', 30)] * 50
    for position, n in ((101, 5), (103, 9), (105, 5), (107, 5)):
        rows += [(position, '1M', 'G', 30)] * n
    rows.sort(key=lambda row: row[0])
    reads = cr.make_reads(rows)
    kwargs = dict(minimum_coverage=10, minimum_alternative_fraction=0.01, minimum_alternative_coverage=2, minimum_fraction_of_ref_and_alt=0.98)
    for cap, want in ((10, [101, 103, 105, 107]), (4, [101, 103, 105, 107]), (3, [103, 105, 107]), (2, [103, 107]), (1, [103])):
        assert list(device_candidates(reads, 90, 120, max_snp_candidates=cap, **kwargs)) == want
        assert list(cr.candidates(cr.coverage(reads, 90, 120), 90, max_snp_candidates=cap, **kwargs)) == want


def test_the_filter_rounds_each_product_once():
    rows = [(0, '1M', 'A', 30)] * 97 + [(0, '1M', 'C', 30), (0, '1M', 'G', 30), (0, '1M', 'T', 30)]
    rows += [(1, '1M', 'A', 30)] * 97 + [(1, '1M', 'C', 30)] * 2 + [(1, '1M', 'G', 30)]
    rows += [(2, '1M', 'A', 30)] * 10 + [(2, '1M', 'C', 30)] + [(3, '1M', 'A', 30)] * 10 + [(3, '1M', 'C', 30)] * 2
    reads = cr.make_reads(rows)
    kwargs = dict(minimum_coverage=0, minimum_alternative_coverage=0)
    assert list(device_candidates(reads, 0, 4, minimum_alternative_fraction=0.0, minimum_fraction_of_ref_and_alt=0.98, **kwargs)) == [1, 2, 3]
    assert list(device_candidates(reads, 0, 4, minimum_alternative_fraction=0.1, minimum_fraction_of_ref_and_alt=0.0, **kwargs)) == [3]


@pytest.mark.parametrize('kwargs', [
    dict(seed=1, n_reads=3000, n_positions=1, length=6000, n_cb=4, n_ub=3, step=1),        # deep: hundreds of reads per position
    dict(seed=2, n_reads=3000, n_positions=1, length=400000, n_cb=3, n_ub=2, step=260),    # sparse, long N skips reach over later reads
    dict(seed=5, n_reads=1, n_positions=1, length=300, n_cb=1, n_ub=1, step=1),
], ids=lambda k: f'seed{k["seed"]}')
def test_device_equals_the_restatement_on_random_reads(kwargs):
    reads, _positions = random_problem(**kwargs)
    assert set(np.unique(reads['cigar'] & 15)) == set(range(9)) or kwargs['n_reads'] == 1
    end = max(cr.reference_end(reads, r) for r in range(len(reads['reference_start'])))
    first = int(reads['reference_start'][0])
    middle = (first + end) // 2
    windows = [(0, end + 5), (middle, min(end, middle + 4100)), (max(0, first - 3), first + 1), (end - 1, end + 200), (middle, middle)]
    for quality_threshold in (15, 0, 61):
        for start, stop in windows:
            want = cr.coverage(reads, start, stop, quality_threshold)
            got = device_coverage(reads, start, stop, quality_threshold)
            print(kwargs['seed'], (start, stop), quality_threshold, 'bases counted', int(want.sum()))
            assert np.array_equal(got, want)
    # candidates and fragments of a few hundred bases, with a cap that bites
    thresholds = dict(minimum_coverage=3, minimum_alternative_fraction=0.05, minimum_alternative_coverage=1, minimum_fraction_of_ref_and_alt=0.7)
    length = min(end, first + 5000)
    for step, cap in ((300, 10000), (257, 5)):
        got = find_candidate_positions({'chrR': DecodedReads(**reads)}, max_fragment_step=step, max_snp_candidates=cap,
                                       chromosome2length={'chrR': length}, **thresholds)['chrR']
        want = cr.find_candidates(reads, length, max_fragment_step=step, max_snp_candidates=cap, **thresholds)
        print(kwargs['seed'], 'step', step, 'cap', cap, len(want), 'candidates')
        assert got.dtype == np.int32 and np.array_equal(got, want)
    default_length = find_candidate_positions({'chrR': DecodedReads(**reads)}, max_fragment_step=1 << 20, **thresholds)['chrR']
    assert np.array_equal(default_length, cr.find_candidates(reads, None, max_fragment_step=1 << 20, **thresholds))


def test_device_equals_the_restatement_on_a_piled_up_problem():
    """Thousands of reads on one start: tiles split over several workgroups, counters far above any lane count."""
    reads, _positions = skewed_problem()
    for start, stop in ((0, 6000), (5000, 5100), (150, 5050)):
        want = cr.coverage(reads, start, stop)
        assert want.sum(axis=0).max() > 3000 or (start, stop) != (0, 6000)
        assert np.array_equal(device_coverage(reads, start, stop), want)
    thresholds = dict(minimum_coverage=100, minimum_alternative_fraction=0.01, minimum_alternative_coverage=100, minimum_fraction_of_ref_and_alt=0.3)
    for cap in (10000, 17):
        want = cr.candidates(cr.coverage(reads, 0, 6000), 0, max_snp_candidates=cap, **thresholds)
        assert len(want) == min(cap, 200)
        assert np.array_equal(device_candidates(reads, 0, 6000, max_snp_candidates=cap, **thresholds), want)


def invalid_reads():
    good = [(0, '4M', 'ACGT', 30), (2, '2M 1D 2M', 'ACGT', 30), (3, '2H 3M', 'ACG', 30)]

    def broken(name, index, value):
        reads = cr.make_reads(good)
        reads[name][index] = value
        return reads

    return cr.make_reads(good), {
        'an operation above 8': broken('cigar', 0, (4 << 4) | 9),
        'an aligned base beyond l_seq': broken('l_seq', 1, 3),
        'a cigar range outside the array': broken('n_cigar', 2, 3),
        'a negative cigar range': broken('n_cigar', 1, -1),
        'a seq range outside the array': broken('seq_begin', 2, 9),
        'a negative seq_begin': broken('seq_begin', 0, -1),
        'a decreasing reference_start': broken('reference_start', 2, 1),
        'a reference_end beyond 2^31': broken('cigar', 4, ((1 << 28) - 1) << 4 | 3) | dict(reference_start=np.asarray([0, 2, 2 ** 31 - 100], np.int32)),
    }


def test_invalid_inputs_return_the_invalid_argument_status_and_the_context_stays_usable():
    good, invalid = invalid_reads()
    want = cr.coverage(good, 0, 12)
    assert np.array_equal(device_coverage(good, 0, 12), want)
    for name, reads in invalid.items():
        with pytest.raises(cr.InvalidReads):
            cr.coverage(reads, 0, 12)
        for form in FORMS.values():
            with shared_context_lock:
                ctx = get_context()
                ctx.set_coverage_form(form)
                with pytest.raises(_lib.DemuxHipError, match=r'status -1\)') as error:
                    ctx.coverage_count(DecodedReads(**reads), 0, 12)
                with pytest.raises(_lib.DemuxHipError, match='call order'):  # no window is left behind
                    ctx.coverage_candidates(1, 0.01, 1, 0.98, 10)
        print(name, '->', error.value)
        assert np.array_equal(device_coverage(good, 0, 12), want), f'after {name}'
    # invalid whatever the window: the broken read lies outside it
    with pytest.raises(_lib.DemuxHipError, match=r'status -1\)'):
        device_coverage(invalid['an operation above 8'], 6, 12)
    with shared_context_lock:
        ctx = get_context()
        for arguments in ((-1, 0.01, 1, 0.98, 10), (1, 0.01, -1, 0.98, 10), (1, 0.01, 1, 0.98, 0), (1, float('nan'), 1, 0.98, 10),
                          (1, 0.01, 1, float('inf'), 10)):
            with pytest.raises(_lib.DemuxHipError, match=r'status -1\)'):
                ctx.coverage_candidates(*arguments)
        for window in ((-1, 5), (5, 4)):
            with pytest.raises(_lib.DemuxHipError, match=r'status -1\)'):
                ctx.coverage_count(DecodedReads(**good), *window)
        with pytest.raises(_lib.DemuxHipError, match=r'status -1\)'):
            ctx.coverage_count(DecodedReads(**good), 0, 12, quality_threshold=256)
    empty = device_coverage(cr.make_reads([]), 3, 9)
    assert empty.shape == (4, 6) and not empty.any()
    assert device_coverage(good, 5, 5).shape == (4, 0)


def test_coverage_leaves_a_resident_problem_and_the_read_counting_records_unchanged():
    fx = fio.load('f3_small_2.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    posteriors = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.35, on_device=True)
    try:
        ctx = posteriors._ctx
        before = (ctx.get_logits().copy(), ctx.get_probs().copy(), posteriors.assignments(0.8).to_dict())
        reads, positions = skewed_problem()
        molecules, snp_calls = ctx.count_reads(DecodedReads(**reads), positions, quality_table())
        bytes_before = ctx.device_bytes()
        counts = ctx.coverage_count(DecodedReads(**reads), 0, 6000)
        found = ctx.coverage_candidates(100, 0.01, 100, 0.3, 50)
        # 12 003 reads of 100 bases, qualities uniform over 0 .. 60: 46 of 61 reach the threshold of 15, about 905 000 bases
        assert counts.sum() > 800_000 and len(found) == 50 and ctx.device_bytes() > bytes_before
        timings = ctx.coverage_timings()
        assert list(timings) == list(_lib.COVERAGE_STAGES) and all(ms >= 0 for ms in timings.values()) and timings['accumulate'] > 0
        after = (ctx.get_logits(), ctx.get_probs(), posteriors.assignments(0.8).to_dict())
        fio.assert_bitwise(after[0], before[0], 'logits of the resident problem')
        fio.assert_bitwise(after[1], before[1], 'posteriors of the resident problem')
        assert after[2] == before[2]
        # the records of the last count_reads are still the ones fetched before the coverage call
        again_molecules = np.empty_like(molecules)
        again_calls = np.empty_like(snp_calls)
        _lib.check(ctx._lib.dmx_count_reads_fetch(ctx._h, _lib.ptr(again_molecules), _lib.ptr(again_calls)))
        assert again_molecules.tobytes() == molecules.tobytes() and again_calls.tobytes() == snp_calls.tobytes()
    finally:
        posteriors.close()
    fresh = DeviceContext(0)
    try:
        empty = fresh.device_bytes()
        fresh.coverage_count(DecodedReads(**reads), 0, 6000, fetch=False)
        fresh.coverage_candidates(100, 0.01, 100, 0.3, 50)
        assert fresh.device_bytes() > empty
        fresh.release_problem()
        assert fresh.device_bytes() == empty
        with pytest.raises(_lib.DemuxHipError, match='call order'):
            fresh.coverage_candidates(100, 0.01, 100, 0.3, 50)
    finally:
        fresh.close()


def fixture_inputs(fx):
    """(every read parse_read accepts, the whitelisted ones, genotypes, barcode handler) of the f10 fixture."""
    everything, whitelisted = {}, {}
    for i, chrom in enumerate(fx['chroms']):
        reads = fixture_reads(fx, i)
        everything[str(chrom)] = DecodedReads(**reads)
        keep = reads['compressed_cb'] >= 0
        assert keep.any() and not keep.all()
        kept = {name: reads[name][keep] for name in ('reference_start', 'compressed_cb', 'compressed_ub', 'p_misaligned',
                                                     'alignment_score', 'cigar_begin', 'n_cigar', 'seq_begin', 'l_seq')}
        whitelisted[str(chrom)] = DecodedReads(cigar=reads['cigar'], seq=reads['seq'], qual=reads['qual'], **kept)
    genotypes = ProbabilisticGenotypes([str(s) for s in fx['genotype_names']], default_prior=float(fx['default_prior']))
    genotypes.var2varid = {(str(c), int(p), 'ACGTN'[int(b)]): int(r)
                           for c, p, b, r in zip(fx['var_chrom'], fx['var_pos'], fx['var_base'], fx['var_row'])}
    genotypes.variant_betas = np.array(fx['betas'], dtype=np.float32)
    handler = BarcodeHandler([str(b) for b in fx['barcodes']])
    assert handler.ordered_barcodes == [str(b) for b in fx['barcodes']]
    return everything, whitelisted, genotypes, handler


def detection_kwargs(fx, e):
    s, n_best, n_add, ignore = (int(v) for v in fx['end_to_end'][e])
    kwargs = threshold_kwargs(fx['thresholds'][s])
    del kwargs['minimum_fraction_of_ref_and_alt']  # the reference's detect_snps_positions leaves it at its default
    kwargs.update(n_best_snps_per_donor=n_best, n_additional_best_snps=n_add, ignore_known_snps=bool(ignore))
    return kwargs


@pytest.mark.parametrize('e', [0, 1])
def test_detect_snps_positions_from_reads_equals_the_reference(e, tmp_path):
    fx = fio.load(FIXTURE)
    everything, whitelisted, genotypes, handler = fixture_inputs(fx)
    chroms = [str(c) for c in fx['chroms']]
    path = str(tmp_path / 'prior.parquet')
    result = detect_snps_positions_from_reads(whitelisted, genotypes, handler, coverage_reads=everything,
                                              chromosome2length={c: int(fx['length']) for c in chroms},
                                              result_beta_prior_filename=path, **detection_kwargs(fx, e))
    assert [(c, p) for c, p, *_ in result] == [(chroms[c], int(p)) for c, p in zip(fx[f'detect{e}_chrom'], fx[f'detect{e}_pos'])]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), fx[f'detect{e}_importances'], 'importances')
    assert [''.join(bc) for *_, bc in result] == [str(b) for b in fx[f'detect{e}_bases']]
    assert np.array_equal([list(bc.values()) for *_, bc in result], fx[f'detect{e}_totals'])
    index = pd.read_parquet(path).index.to_frame()
    # the reference lists the positions of a chromosome in the order its calls meet them, this package ascending: compared
    # position by position, ref base before alt base as recorded
    order = sorted(range(len(fx[f'detect{e}_parquet_pos'])), key=lambda k: (chroms.index(str(fx[f'detect{e}_parquet_chrom'][k])), int(fx[f'detect{e}_parquet_pos'][k])))
    assert list(index['CHROM']) == [str(fx[f'detect{e}_parquet_chrom'][k]) for k in order]
    assert list(index['POS']) == [int(fx[f'detect{e}_parquet_pos'][k]) for k in order]
    assert list(index['BASE']) == [str(fx[f'detect{e}_parquet_base'][k]) for k in order]


def test_detect_snps_positions_from_reads_equals_detection_from_its_own_calls():
    fx = fio.load(FIXTURE)
    everything, whitelisted, genotypes, handler = fixture_inputs(fx)
    kwargs = detection_kwargs(fx, 0)
    candidate_kwargs = {name: kwargs[name] for name in ('minimum_coverage', 'minimum_alternative_fraction', 'minimum_alternative_coverage')}
    for coverage_reads in (everything, None):
        from_reads = detect_snps_positions_from_reads(whitelisted, genotypes, handler, coverage_reads=coverage_reads, **kwargs)
        candidates = find_candidate_positions(whitelisted if coverage_reads is None else coverage_reads, **candidate_kwargs)
        assert list(candidates) == list(whitelisted)
        known_calls = count_snps_from_reads(whitelisted, genotypes.get_chromosome2positions())
        candidate_calls = count_snps_from_reads(whitelisted, candidates)
        from_calls = detect_snps_positions_from_calls(known_calls, candidate_calls, genotypes, handler,
                                                      **{name: kwargs[name] for name in kwargs if name not in candidate_kwargs})
        assert len(from_reads) > 0
        assert [(c, p) for c, p, *_ in from_reads] == [(c, p) for c, p, *_ in from_calls]
        fio.assert_bitwise(np.stack([imp for _, _, imp, _ in from_reads]), np.stack([imp for _, _, imp, _ in from_calls]), 'importances')
        assert [bc for *_, bc in from_reads] == [bc for *_, bc in from_calls]
