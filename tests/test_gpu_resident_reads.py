"""Resident read sets on the GPU (include/demux_hip_debug.h "Resident reads"): counting, streamed range pushes, coverage,
candidates and detection from a set that was uploaded once give what the host-array calls give on the same reads - records bit
for bit, equal integers, equal statuses - and upload nothing, which the context's byte counter shows."""
import ctypes

import numpy as np
import pytest

from demuxalot_amd import (DecodedReads, Demultiplexer, ReadCounter, ResidentReads, _lib, count_snps_from_reads, coverage_from_reads,
                           detect_snps_positions_from_reads, find_candidate_positions)
from demuxalot_amd.device import DeviceContext, get_context, shared_context_lock
from demuxalot_amd.snp_counter import quality_table
from demuxalot_amd.snp_detection import reference_ends
from demuxalot_amd.synth import generate_reads
from tests import coverage_restatement as cr
from tests import fixture_io as fio
from tests.count_reads_stream_restatement import even_cuts
from tests.test_count_reads_cpu import FIXTURES, assert_records_equal, fixture_chromosomes
from tests.test_count_reads_stream_cpu import chunkings
from tests.test_coverage_cpu import FIXTURE, fixture_reads, threshold_kwargs
from tests.test_gpu_count_reads import random_problem, skewed_problem
from tests.test_gpu_coverage import FORMS, detection_kwargs, fixture_inputs, invalid_reads

pytestmark = pytest.mark.gpu

INVALID = r'status -1\)'  # DMX_ERR_INVALID
COVERAGE_BYTES_PER_READ = 3 * 4 + 2 * 8  # reference_start, n_cigar, l_seq; cigar_begin, seq_begin


def coverage_bytes(reads):
    """Bytes of the eight arrays a coverage pass reads."""
    return reads.n_reads * COVERAGE_BYTES_PER_READ + reads.cigar.nbytes + reads.seq.nbytes + reads.qual.nbytes


def assert_same(got, want, what):
    assert_records_equal(got[0], want[0], f'{what}: molecules')
    assert_records_equal(got[1], want[1], f'{what}: snp_calls')


def stream_ranges(resident, positions, cuts):
    """(molecules, snp_calls) of a resident set pushed as the device ranges the cuts give."""
    bounds = [0] + [int(c) for c in cuts] + [resident.n_reads]
    parts = []
    with ReadCounter(positions) as counter:
        for k, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            parts.append(counter.finish((resident, lo, hi)) if k == len(bounds) - 2 else counter.push((resident, lo, hi)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def one_call(reads, positions):
    with shared_context_lock:
        return get_context().count_reads(reads, positions, quality_table())


def resident_call(resident, positions):
    with shared_context_lock:
        return get_context().count_reads_resident(resident._handle, positions, quality_table())


def upload_bytes():
    with shared_context_lock:
        return get_context().reads_upload_bytes()


# ---- 1 counting on the fixtures

@pytest.mark.parametrize('name', FIXTURES)
def test_resident_counting_gives_the_recorded_records(name):
    for chromosome, reads, positions, molecules, snp_calls in fixture_chromosomes(name):
        with ResidentReads(DecodedReads(**reads)) as resident:
            assert resident.n_reads == len(reads['reference_start'])
            assert_same(resident_call(resident, positions), (molecules, snp_calls), f'{name} {chromosome} one call')
            for what, cuts in chunkings(resident.n_reads).items():
                assert_same(stream_ranges(resident, positions, cuts), (molecules, snp_calls), f'{name} {chromosome} {what}')


# ---- 2 counting on synthetic reads

@pytest.fixture(scope='module')
def synthetic():
    reads, positions = generate_reads(200_000, 2_000)
    with shared_context_lock:
        ctx = get_context()
        want = ctx.count_reads(reads, positions, quality_table())
        return reads, positions, want, ctx.count_reads_peak_bytes()


def test_one_call_resident_call_and_resident_stream_agree(synthetic):
    reads, positions, want, one_call_peak = synthetic
    assert len(want[0]) > 5_000 and len(want[1]) > 5_000
    before = upload_bytes()
    with ResidentReads(reads) as resident:
        uploaded = upload_bytes() - before
        assert uploaded == coverage_bytes(reads) + reads.n_reads * (3 * 4 + 8)  # all twelve arrays, once
        assert_same(resident_call(resident, positions), want, 'resident call')
        assert_same(stream_ranges(resident, positions, even_cuts(reads.n_reads, 16)), want, 'resident stream of 16 ranges')
        by_dict = count_snps_from_reads({'chr1': resident}, {'chr1': positions, 'none': positions[:3]}, max_reads_per_call=30_000)
        assert_same((by_dict['chr1'].molecules, by_dict['chr1'].snp_calls), want, 'count_snps_from_reads, device ranges')
        assert by_dict['none'].n_molecules == 0
        assert upload_bytes() - before == uploaded, 'the resident calls upload no reads'
        with shared_context_lock:
            peak = get_context().count_reads_peak_bytes()
        # the last push, 20 000 of 200 000 reads and a carry: its scratch and gathered input, not the set (every cost is linear
        # in the reads of a call; the bound leaves room for rocPRIM's fixed temporaries)
        assert 0 < peak < one_call_peak / 2


# ---- 3 coverage

def both_forms(count):
    got = {}
    with shared_context_lock:
        ctx = get_context()
        for name, form in FORMS.items():
            ctx.set_coverage_form(form)
            got[name] = count(ctx)
    assert np.array_equal(got['atomic'], got['tiled'])
    return got['tiled']


def resident_coverage(resident, start, stop, quality_threshold=15):
    got = both_forms(lambda ctx: ctx.coverage_count_resident(resident._handle, start, stop, quality_threshold))
    assert got.dtype == np.int32 and got.shape == (4, stop - start)
    return got


@pytest.mark.parametrize('case', cr.HAND_TABLE, ids=[case[0] for case in cr.HAND_TABLE])
def test_resident_set_gives_the_hand_written_coverage(case):
    _name, rows, start, stop, quality_threshold, expected = case
    with ResidentReads(DecodedReads(**cr.make_reads(rows))) as resident:
        assert np.array_equal(resident_coverage(resident, start, stop, quality_threshold), expected)
        assert np.array_equal(coverage_from_reads(resident, start, stop, quality_threshold=quality_threshold), expected)


def test_resident_set_gives_the_recorded_candidates():
    fx = fio.load(FIXTURE)
    length = int(fx['length'])
    residents = [ResidentReads(DecodedReads(**fixture_reads(fx, i))) for i in range(len(fx['chroms']))]
    try:
        for i, resident in enumerate(residents):
            assert np.array_equal(resident_coverage(resident, 0, length), fx[f'cov{i}'])
            for s, row in enumerate(fx['thresholds']):
                got = find_candidate_positions({'c': resident}, chromosome2length={'c': length}, max_fragment_step=length, **threshold_kwargs(row))
                assert got['c'].dtype == np.int32 and np.array_equal(got['c'], fx[f'cand{s}_c{i}'])
        assert any(int(start) > 0 for _chrom, start, _stop in fx['windows'])
        for w, (chrom, start, stop) in enumerate(fx['windows']):
            with shared_context_lock:
                ctx = get_context()
                ctx.coverage_count_resident(residents[int(chrom)]._handle, int(start), int(stop), fetch=False)
                kwargs = threshold_kwargs(fx['thresholds'][0])
                got = ctx.coverage_candidates(kwargs['minimum_coverage'], kwargs['minimum_alternative_fraction'],
                                              kwargs['minimum_alternative_coverage'], kwargs['minimum_fraction_of_ref_and_alt'], 10000)
            assert np.array_equal(got, fx[f'window{w}'] + start)
    finally:
        for resident in residents:
            resident.close()


@pytest.fixture(scope='module')
def random_reads():
    """A few thousand reads with every operation, letters ACGTN, qualities 0 .. 60; long N skips that reach over later reads."""
    reads, _positions = random_problem(seed=2, n_reads=3000, n_positions=1, length=400000, n_cb=3, n_ub=2, step=260)
    assert set(np.unique(reads['cigar'] & 15)) == set(range(9))
    return reads


def test_resident_coverage_equals_the_restatement_on_random_reads(random_reads):
    reads = random_reads
    end = max(cr.reference_end(reads, r) for r in range(len(reads['reference_start'])))
    first = int(reads['reference_start'][0])
    middle = (first + end) // 2
    only_coverage = DecodedReads(**reads)
    with ResidentReads(only_coverage) as resident, ResidentReads(only_coverage, coverage_only=True) as lean:
        assert lean.nbytes < resident.nbytes
        for quality_threshold, (start, stop) in ((15, (0, end + 5)), (0, (middle, min(end, middle + 4100))), (61, (end - 1, end + 200))):
            want = cr.coverage(reads, start, stop, quality_threshold)
            assert np.array_equal(resident_coverage(resident, start, stop, quality_threshold), want)
            assert np.array_equal(resident_coverage(lean, start, stop, quality_threshold), want), 'a set without the counting columns'
        # 6 info: the largest reference_end, from the device
        assert resident.reference_length == int(reference_ends(only_coverage).max()) == end == lean.reference_length
        with pytest.raises(_lib.DemuxHipError, match=INVALID):  # counting on a coverage-only set
            resident_call(lean, np.array([5], np.int32))
        with pytest.raises(_lib.DemuxHipError, match=INVALID):
            stream_ranges(lean, np.array([5], np.int32), [10])
        assert resident_coverage(lean, 0, 50).shape == (4, 50), 'the context and the set stay usable'
    with ResidentReads(DecodedReads(**cr.make_reads([]))) as empty:
        assert empty.reference_length == 0 and empty.n_reads == 0
        assert not resident_coverage(empty, 3, 9).any()
        assert len(resident_call(empty, np.array([5], np.int32))[0]) == 0


# ---- 4 shuffled offsets

def shuffled_reads(seed=11):
    """Reads whose cigar and seq segments lie in a random permutation of the read order, with unused elements between them;
    some reads have no operation at all, one skips 40 000 bases."""
    reads, positions = random_problem(seed=seed, n_reads=700, n_positions=400, length=30000, n_cb=4, n_ub=3, step=90)
    rng = np.random.default_rng(seed)
    n = len(reads['reference_start'])
    reads = {name: value.copy() for name, value in reads.items()}
    cigar_of = [reads['cigar'][c0:c0 + k] for c0, k in zip(reads['cigar_begin'], reads['n_cigar'])]
    seq_of = [reads['seq'][s0:s0 + k] for s0, k in zip(reads['seq_begin'], reads['l_seq'])]
    qual_of = [reads['qual'][s0:s0 + k] for s0, k in zip(reads['seq_begin'], reads['l_seq'])]
    for r in rng.choice(n, 25, replace=False):
        cigar_of[r] = cigar_of[r][:0]
    cigar_of[5] = np.array([30 << 4, 40_000 << 4 | 3, 30 << 4], dtype=np.uint32)
    seq_of[5], qual_of[5] = np.full(60, ord('G'), np.uint8), np.full(60, 33, np.uint8)
    cigars, seqs, quals, c_at, s_at = [], [], [], 0, 0
    for r in rng.permutation(n):
        pad = int(rng.integers(0, 3))
        cigars += [np.full(pad, 15, np.uint32), cigar_of[r]]
        seqs += [np.full(pad, ord('R'), np.uint8), seq_of[r]]
        quals += [np.zeros(pad, np.uint8), qual_of[r]]
        reads['cigar_begin'][r], reads['seq_begin'][r] = c_at + pad, s_at + pad
        reads['n_cigar'][r], reads['l_seq'][r] = len(cigar_of[r]), len(seq_of[r])
        c_at, s_at = c_at + pad + len(cigar_of[r]), s_at + pad + len(seq_of[r])
    reads.update(cigar=np.concatenate(cigars), seq=np.concatenate(seqs), qual=np.concatenate(quals))
    assert np.any(np.diff(reads['cigar_begin']) < 0) and np.any(np.diff(reads['seq_begin']) < 0)
    positions = np.unique(np.concatenate([positions, reads['reference_start'][5] + np.array([3, 40_035, 40_050], np.int32)]))
    return DecodedReads(**reads), positions.astype(np.int32)


@pytest.mark.parametrize('width', [1, 7, 64])
def test_ranges_of_shuffled_offsets_equal_the_one_call(width):
    reads, positions = shuffled_reads()
    want = one_call(reads, positions)
    assert len(want[0]) > 100 and len(want[1]) > 100
    with ResidentReads(reads) as resident:
        assert_same(resident_call(resident, positions), want, 'resident call')
        assert_same(stream_ranges(resident, positions, range(width, reads.n_reads, width)), want, f'ranges of {width} reads')


# ---- 5 uploads

def test_find_candidate_positions_uploads_a_chromosome_once(synthetic):
    reads = synthetic[0]
    thresholds = dict(minimum_coverage=5, minimum_alternative_fraction=0.02, minimum_alternative_coverage=1, minimum_fraction_of_ref_and_alt=0.5)
    with ResidentReads(reads) as resident:
        length = resident.reference_length
        assert length == int(reference_ends(reads).max())
        step = (length + 7) // 8
        assert len(range(0, length, step)) == 8
        before = upload_bytes()
        from_resident = find_candidate_positions({'chr1': resident}, max_fragment_step=step, **thresholds)['chr1']
        assert upload_bytes() - before == 0
    before = upload_bytes()
    from_host = find_candidate_positions({'chr1': reads}, max_fragment_step=step, **thresholds)['chr1']
    assert upload_bytes() - before == coverage_bytes(reads), 'eight fragments, one upload of the arrays the coverage reads'
    assert len(from_host) > 0 and np.array_equal(from_host, from_resident)


def test_detection_from_resident_reads_uploads_nothing_and_equals_the_reference():
    fx = fio.load(FIXTURE)
    everything, whitelisted, genotypes, handler = fixture_inputs(fx)
    chroms = [str(c) for c in fx['chroms']]
    kwargs = dict(chromosome2length={c: int(fx['length']) for c in chroms}, **detection_kwargs(fx, 0))
    from_host = detect_snps_positions_from_reads(whitelisted, genotypes, handler, coverage_reads=everything, **kwargs)
    resident = {c: ResidentReads(reads) for c, reads in whitelisted.items()}
    resident_coverage_reads = {c: ResidentReads(reads, coverage_only=True) for c, reads in everything.items()}
    try:
        before = upload_bytes()
        result = detect_snps_positions_from_reads(resident, genotypes, handler, coverage_reads=resident_coverage_reads, **kwargs)
        assert upload_bytes() - before == 0
    finally:
        for held in list(resident.values()) + list(resident_coverage_reads.values()):
            held.close()
    assert len(result) > 0 and [(c, p) for c, p, *_ in result] == [(c, p) for c, p, *_ in from_host]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), np.stack([imp for _, _, imp, _ in from_host]), 'importances')
    assert [bc for *_, bc in result] == [bc for *_, bc in from_host]
    assert [(c, p) for c, p, *_ in result] == [(chroms[c], int(p)) for c, p in zip(fx['detect0_chrom'], fx['detect0_pos'])]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), fx['detect0_importances'], 'importances against the reference')


# ---- 7 status and lifetime

def test_status_codes_and_lifetime_of_a_set():
    reads, positions = skewed_problem()
    decoded, table = DecodedReads(**reads), quality_table()
    want = one_call(decoded, positions)
    other = DeviceContext(0)
    try:
        foreign = ResidentReads(decoded.slice(0, 10), on_context=other)
        with shared_context_lock:
            ctx = get_context()
            resident = ResidentReads(decoded)
            handle = resident._handle
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # a push with no open stream
                ctx.count_reads_push_resident(handle, 0, 5)
            for call in (lambda h: ctx.count_reads_resident(h, positions, table), lambda h: ctx.coverage_count_resident(h, 0, 10),
                         ctx.reads_info, ctx.reads_release):
                with pytest.raises(_lib.DemuxHipError, match=INVALID):  # a handle of another context
                    call(foreign._handle)
            # null pointers on a live context: refused before anything is read or written
            raw, count = ctx._lib, ctypes.c_int64(0)
            arrays = decoded.arrays()
            desc = _lib.DecodedReadsStruct(n_reads=decoded.n_reads, n_cigar_ops=len(arrays['cigar']), n_bases=len(arrays['seq']),
                                           **{name: _lib.ptr(a) for name, a in arrays.items()})
            valid_reads = ctypes.cast(ctypes.byref(desc), ctypes.c_void_p)
            for refused in (raw.dmx_reads_upload(ctx._h, valid_reads, None), raw.dmx_reads_upload(ctx._h, None, ctypes.byref(count)),
                            raw.dmx_reads_info(ctx._h, handle, None), raw.dmx_get_reads_upload_bytes(ctx._h, None),
                            raw.dmx_count_reads_resident(ctx._h, handle, _lib.ptr(positions), len(positions), _lib.ptr(table), None,
                                                         ctypes.byref(count))):
                assert refused == -1
            assert ctx.reads_info(handle)['n_reads'] == decoded.n_reads
            ctx.count_reads_begin(positions, table)
            try:
                for lo, hi in ((5, 4), (0, decoded.n_reads + 1), (-1, 3)):
                    with pytest.raises(_lib.DemuxHipError, match=INVALID):
                        ctx.count_reads_push_resident(handle, lo, hi)
                with pytest.raises(_lib.DemuxHipError, match=INVALID):
                    ctx.count_reads_push_resident(foreign._handle, 0, 5)
                # refused arguments leave the stream open: it counts the set
                parts = [ctx.count_reads_push_resident(handle, 0, 7000), ctx.count_reads_push_resident(handle, 7000, decoded.n_reads, final=True)]
                assert_same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want, 'two ranges')
            finally:
                ctx.count_reads_end()
            with pytest.raises(ValueError, match='another context'):
                count_snps_from_reads({'c': resident}, {'c': positions}, on_context=other)
            with pytest.raises(ValueError, match='another context'):
                coverage_from_reads(foreign, 0, 10, on_context=ctx)
            with pytest.raises(ValueError, match='one context'):
                find_candidate_positions({'a': resident, 'b': foreign}, minimum_coverage=1)
            resident.close()
            resident.close()  # (idempotent)
            for call in (lambda: ctx.count_reads_resident(handle, positions, table), lambda: ctx.coverage_count_resident(handle, 0, 10),
                         lambda: ctx.reads_info(handle), lambda: ctx.reads_release(handle)):
                with pytest.raises(_lib.DemuxHipError, match=INVALID):  # a released handle
                    call()
            with pytest.raises(ValueError, match='closed'):
                resident.n_reads
            with pytest.raises(ValueError, match='closed'):
                count_snps_from_reads({'c': resident}, {'c': positions})
            # the context then counts a valid set correctly
            with ResidentReads(decoded) as again:
                assert again._handle != handle, 'handles are never reused'
                assert_same(ctx.count_reads_resident(again._handle, positions, table), want, 'a valid set after the refusals')
        assert foreign.n_reads == 10
        foreign.close()
    finally:
        other.close()


def test_invalid_reads_give_the_status_of_the_host_array_call():
    good, invalid = invalid_reads()
    want = cr.coverage(good, 0, 12)
    for name, reads in invalid.items():
        decoded = DecodedReads(**reads)
        with ResidentReads(decoded) as resident:  # the upload refuses no read: the passes judge them
            with shared_context_lock:
                ctx = get_context()
                with pytest.raises(_lib.DemuxHipError, match=INVALID) as from_host:
                    ctx.coverage_count(decoded, 0, 12)
                with pytest.raises(_lib.DemuxHipError, match=INVALID) as from_set:
                    ctx.coverage_count_resident(resident._handle, 0, 12)
                assert str(from_set.value) == str(from_host.value), name
                with pytest.raises(_lib.DemuxHipError, match='call order'):  # no window is left behind
                    ctx.coverage_candidates(1, 0.01, 1, 0.98, 10)
                # counting: the same answer from both, an error or the records
                positions, outcomes = np.arange(12, dtype=np.int32), []
                for count in (lambda: ctx.count_reads(decoded, positions, quality_table()),
                              lambda: ctx.count_reads_resident(resident._handle, positions, quality_table())):
                    try:
                        molecules, snp_calls = count()
                        outcomes.append((molecules.tobytes(), snp_calls.tobytes()))
                    except _lib.DemuxHipError as error:
                        outcomes.append(str(error))
                assert outcomes[0] == outcomes[1], name
        assert resident.closed, 'the set stays releasable'
        with ResidentReads(DecodedReads(**good)) as resident:
            assert np.array_equal(resident_coverage(resident, 0, 12), want), f'after {name}'


def test_two_sets_used_alternately_do_not_disturb_each_other(random_reads):
    first = DecodedReads(**random_reads)
    second_arrays, positions = skewed_problem()
    second = DecodedReads(**second_arrays)
    first_positions = np.unique(first.reference_start[::7] + 2).astype(np.int32)
    want = (one_call(first, first_positions), one_call(second, positions), cr.coverage(random_reads, 0, 3000), cr.coverage(second_arrays, 4990, 5100))
    with ResidentReads(first) as a, ResidentReads(second) as b:
        for _round in range(2):
            assert_same(resident_call(a, first_positions), want[0], 'first set')
            assert_same(resident_call(b, positions), want[1], 'second set')
            assert np.array_equal(resident_coverage(a, 0, 3000), want[2])
            assert np.array_equal(resident_coverage(b, 4990, 5100), want[3])


def test_resident_sets_leave_the_resident_problem_and_survive_its_release():
    fx = fio.load('f3_small_2.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    posteriors = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.35, on_device=True)
    try:
        ctx = posteriors._ctx
        before = (ctx.get_logits().copy(), ctx.get_probs().copy())
        reads, positions = skewed_problem()
        decoded = DecodedReads(**reads)
        with ResidentReads(decoded, on_context=ctx) as resident:
            molecules, snp_calls = ctx.count_reads_resident(resident._handle, positions, quality_table())
            assert_same((molecules, snp_calls), ctx.count_reads(decoded, positions, quality_table()), 'on the posteriors\' context')
            counts = ctx.coverage_count_resident(resident._handle, 0, 6000)
            found = ctx.coverage_candidates(100, 0.01, 100, 0.3, 50)
            assert counts.sum() > 800_000 and len(found) == 50
            fio.assert_bitwise(ctx.get_logits(), before[0], 'logits of the resident problem')
            fio.assert_bitwise(ctx.get_probs(), before[1], 'posteriors of the resident problem')
            again_molecules, again_calls = np.empty_like(molecules), np.empty_like(snp_calls)  # the d_cr_* records are the last count's
            _lib.check(ctx._lib.dmx_count_reads_fetch(ctx._h, _lib.ptr(again_molecules), _lib.ptr(again_calls)))
            assert again_molecules.tobytes() == molecules.tobytes() and again_calls.tobytes() == snp_calls.tobytes()
    finally:
        posteriors.close()
    fresh = DeviceContext(0)
    try:
        empty = fresh.device_bytes()
        resident = ResidentReads(decoded, on_context=fresh)
        assert fresh.device_bytes() == empty + resident.nbytes
        fresh.coverage_count_resident(resident._handle, 0, 6000, fetch=False)
        fresh.release_problem()  # the window goes, the set is the caller's and stays
        assert fresh.device_bytes() == empty + resident.nbytes
        with pytest.raises(_lib.DemuxHipError, match='call order'):
            fresh.coverage_candidates(100, 0.01, 100, 0.3, 50)
        assert np.array_equal(fresh.coverage_count_resident(resident._handle, 0, 6000), counts)
        fresh.release_problem()
        resident.close()
        assert fresh.device_bytes() == empty
    finally:
        fresh.close()


def free_device_memory():
    hip = ctypes.CDLL(_lib.runtime_info()['hip'][0])  # the runtime the library runs on, mapped already
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_close_gives_the_device_memory_back(synthetic):
    """After close() and a trim of the block cache the set's blocks are the driver's again.  The slack: the driver hands memory
    out in 2 MiB pages, and a dozen of the context's small blocks may have moved between two of them."""
    reads = synthetic[0]
    slack = 12 * (2 << 20)
    with shared_context_lock:
        ctx = get_context()
        ctx.trim_cache()
        before = free_device_memory()
        resident = ResidentReads(reads)
        assert resident.nbytes > 2 * slack
        held = before - free_device_memory()
        assert held >= resident.nbytes - slack
        resident.close()
        ctx.trim_cache()
        assert free_device_memory() >= before - slack
