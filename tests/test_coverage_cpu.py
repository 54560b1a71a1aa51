"""Coverage and candidate positions without a GPU (DESIGN.md "Coverage and candidates"): the plain restatement
(tests/coverage_restatement.py) against the hand-written table of the coverage rules and against what the reference handed to
its count_snps (tests/golden/f10_coverage_synthetic.npz); the tie rule; the refused arguments; the fragment arithmetic of
find_candidate_positions with the device replaced by the restatement."""
import numpy as np
import pytest

from tests import coverage_restatement as cr
from tests import fixture_io as fio

FIXTURE = 'f10_coverage_synthetic.npz'
READ_ARRAYS = ('reference_start', 'compressed_cb', 'compressed_ub', 'p_misaligned', 'alignment_score', 'cigar_begin', 'n_cigar',
               'seq_begin', 'l_seq', 'cigar', 'seq', 'qual')


def fixture_reads(fx, i):
    return {name: fx[f'r{i}_{name}'] for name in READ_ARRAYS}


def threshold_kwargs(row):
    minimum_coverage, alternative_fraction, alternative_coverage, fraction_of_both = (float(v) for v in row)
    return dict(minimum_coverage=minimum_coverage, minimum_alternative_fraction=alternative_fraction,
                minimum_alternative_coverage=alternative_coverage, minimum_fraction_of_ref_and_alt=fraction_of_both)


class RestatementContext:
    """coverage_count / coverage_candidates of a DeviceContext, answered by the restatement; records the windows asked for."""

    def __init__(self):
        self.windows = []

    def coverage_count(self, reads, start, stop, quality_threshold=15, fetch=True):
        self.windows.append((start, stop))
        self._counts, self._start = cr.coverage(reads.arrays(), start, stop, quality_threshold), start
        return self._counts if fetch else None

    def coverage_candidates(self, minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                            minimum_fraction_of_ref_and_alt, max_snp_candidates, fetch_counts=False):
        return cr.candidates(self._counts, self._start, minimum_coverage=minimum_coverage,
                             minimum_alternative_fraction=minimum_alternative_fraction,
                             minimum_alternative_coverage=minimum_alternative_coverage,
                             minimum_fraction_of_ref_and_alt=minimum_fraction_of_ref_and_alt, max_snp_candidates=max_snp_candidates)


@pytest.mark.parametrize('case', cr.HAND_TABLE, ids=[case[0] for case in cr.HAND_TABLE])
def test_restatement_gives_the_hand_written_coverage(case):
    _name, rows, start, stop, quality_threshold, expected = case
    got = cr.coverage(cr.make_reads(rows), start, stop, quality_threshold)
    assert got.dtype == np.int32 and np.array_equal(got, expected)


def test_hard_clips_and_padding_move_neither_cursor_unlike_read_counting():
    """The same read under both walkers: pysam's pairs here, the reference's own walker in count_reads (H and P move the
    read cursor there)."""
    from tests import count_reads_restatement as counting
    reads = cr.make_reads([(10, '3H 5M', 'ACGTACGT', 30)])
    assert cr.aligned_pairs(reads, 0) == [(0, 10), (1, 11), (2, 12), (3, 13), (4, 14)]
    assert [chr(letter) for _p, letter, _q in counting.observations(reads, 0, np.arange(10, 15))] == list('TACGT')


def test_restatement_matches_the_recorded_coverage_and_the_references_candidates():
    fx = fio.load(FIXTURE)
    length = int(fx['length'])
    for i in range(len(fx['chroms'])):
        reads = fixture_reads(fx, i)
        counts = cr.coverage(reads, 0, length)
        assert np.array_equal(counts, fx[f'cov{i}'])
        for s, row in enumerate(fx['thresholds']):
            want = fx[f'cand{s}_c{i}']
            assert 0 < len(want) < length  # both outcomes of the filter
            assert np.array_equal(cr.candidates(counts, 0, **threshold_kwargs(row)), want)
    assert np.array_equal(cr.candidates(fx['cov0'], 0, max_snp_candidates=int(fx['cap']), **threshold_kwargs(fx['thresholds'][0])),
                          fx['capped_c0'])
    assert len(fx['capped_c0']) == int(fx['cap']) < len(fx['cand0_c0'])


def test_windows_are_absolute_where_the_reference_is_relative():
    fx = fio.load(FIXTURE)
    for w, (chrom, start, stop) in enumerate(fx['windows']):
        assert start > 0
        reads = fixture_reads(fx, int(chrom))
        got = cr.candidates(cr.coverage(reads, int(start), int(stop)), int(start), **threshold_kwargs(fx['thresholds'][0]))
        assert np.array_equal(got, fx[f'window{w}'] + start)  # recorded as the reference returned them
        whole = fx[f'cand0_c{int(chrom)}']
        assert np.array_equal(got, whole[(whole >= start) & (whole < stop)])


def test_a_tie_at_the_cut_goes_to_the_higher_position():
    # alt: positions 1, 3, 5, 7 hold 5, 9, 5, 5; ref 50 everywhere; position 0 is no candidate
    counts = np.zeros((4, 8), dtype=np.int32)
    counts[0] = 50
    counts[2, [1, 3, 5, 7]] = [5, 9, 5, 5]
    kwargs = dict(minimum_coverage=10, minimum_alternative_fraction=0.01, minimum_alternative_coverage=2, minimum_fraction_of_ref_and_alt=0.98)
    assert list(cr.candidates(counts, 100, **kwargs)) == [101, 103, 105, 107]
    assert list(cr.candidates(counts, 100, max_snp_candidates=4, **kwargs)) == [101, 103, 105, 107]
    assert list(cr.candidates(counts, 100, max_snp_candidates=3, **kwargs)) == [103, 105, 107]
    assert list(cr.candidates(counts, 100, max_snp_candidates=2, **kwargs)) == [103, 107]
    assert list(cr.candidates(counts, 100, max_snp_candidates=1, **kwargs)) == [103]
    # the tail of a stable ascending argsort of alt * is_candidate, as the contract words it
    alt = np.sort(counts, axis=0)[-2]
    assert list(np.sort(np.argsort(alt * (alt > 2), kind='stable')[-2:]) + 100) == [103, 107]


def test_the_filter_compares_in_float64_with_one_rounding_per_product():
    # 97 + 1 of 100: 0.98 * 100 rounds to 98.0 in float64, so 98 > 98.0 fails (in exact arithmetic 0.98's double is below 0.98
    # and it would pass); 97 + 2 of 100 passes
    counts = np.asarray([[97, 97], [1, 2], [1, 1], [1, 0]], dtype=np.int32)
    kwargs = dict(minimum_coverage=0, minimum_alternative_fraction=0.0, minimum_alternative_coverage=0, minimum_fraction_of_ref_and_alt=0.98)
    assert 0.98 * 100.0 == 98.0
    assert list(cr.candidates(counts, 0, **kwargs)) == [1]
    # alt > ref * fraction: 1 > 10 * 0.1 fails, 2 > 10 * 0.1 passes
    counts = np.asarray([[10, 10], [1, 2], [0, 0], [0, 0]], dtype=np.int32)
    kwargs.update(minimum_alternative_fraction=0.1, minimum_fraction_of_ref_and_alt=0.0)
    assert list(cr.candidates(counts, 0, **kwargs)) == [1]


BAD_ARGUMENTS = [dict(minimum_alternative_coverage=-1), dict(minimum_coverage=-1), dict(max_snp_candidates=0),
                 dict(minimum_coverage=float('nan')), dict(minimum_alternative_fraction=float('inf')),
                 dict(minimum_fraction_of_ref_and_alt=float('-inf')), dict(minimum_alternative_coverage=float('nan'))]


@pytest.mark.parametrize('bad', BAD_ARGUMENTS, ids=[next(iter(bad)) + '=' + str(next(iter(bad.values()))) for bad in BAD_ARGUMENTS])
def test_refused_arguments_raise_value_error(bad):
    from demuxalot_amd import DecodedReads, detect_snps_positions_from_reads, find_candidate_positions
    reads = {'chr1': DecodedReads(**cr.make_reads([(0, '4M', 'ACGT', 30)]))}
    kwargs = dict(minimum_coverage=1)
    kwargs.update(bad)
    ctx = RestatementContext()
    with pytest.raises(ValueError):
        find_candidate_positions(reads, on_context=ctx, **kwargs)
    assert ctx.windows == []  # refused before anything is counted
    with pytest.raises(ValueError):
        detect_snps_positions_from_reads(reads, None, None, **kwargs)
    with pytest.raises(ValueError):
        cr.candidates(np.zeros((4, 1), dtype=np.int32), 0, **kwargs)


def test_argument_types_and_windows():
    from demuxalot_amd import DecodedReads, coverage_from_reads, find_candidate_positions
    reads = DecodedReads(**cr.make_reads([(0, '4M', 'ACGT', 30)]))
    with pytest.raises(TypeError):
        find_candidate_positions([reads], minimum_coverage=1)
    with pytest.raises(TypeError):
        find_candidate_positions({'chr1': reads.arrays()}, minimum_coverage=1)
    with pytest.raises(TypeError):
        coverage_from_reads(reads.arrays(), 0, 4)
    for start, stop in ((-1, 4), (5, 4)):
        with pytest.raises(ValueError):
            coverage_from_reads(reads, start, stop, on_context=RestatementContext())
    with pytest.raises(ValueError):
        find_candidate_positions({'chr1': reads}, minimum_coverage=1, max_fragment_step=0)
    with pytest.raises(ValueError):
        find_candidate_positions({'chr1': reads}, minimum_coverage=1, quality_threshold=256)


def test_restatement_rejects_the_invalid_inputs():
    good = [(0, '4M', 'ACGT', 30), (2, '2M 1D 2M', 'ACGT', 30)]
    cr.coverage(cr.make_reads(good), 0, 10)

    def broken(change):
        reads = cr.make_reads(good)
        change(reads)
        return reads

    def set_item(name, index, value):
        def change(reads):
            reads[name][index] = value
        return change

    for change in (set_item('cigar', 0, (4 << 4) | 9),            # an operation above 8
                   set_item('l_seq', 1, 3),                       # an aligned base beyond l_seq
                   set_item('n_cigar', 1, 4),                     # a cigar range outside the array
                   set_item('seq_begin', 1, 6),                   # a seq range outside the array
                   set_item('reference_start', 1, -1)):           # a decreasing reference_start
        with pytest.raises(cr.InvalidReads):
            cr.coverage(broken(change), 0, 10)


@pytest.mark.parametrize('step', [1000, 400, 333, 250, 1])
def test_fragments_of_find_candidate_positions(step):
    """The reference's fragments [k * step, min((k + 1) * step, length)), the cut per fragment, absolute positions."""
    from demuxalot_amd import DecodedReads, find_candidate_positions
    fx = fio.load(FIXTURE)
    if step == 1:  # one position per fragment: a small chromosome
        reads = {'tiny': DecodedReads(**cr.make_reads([(2, '6M', 'ACGTAC', 30)] * 3 + [(4, '3M', 'TTT', 30)] * 2))}
        kwargs = dict(minimum_coverage=3, minimum_alternative_fraction=0.01, minimum_alternative_coverage=1, minimum_fraction_of_ref_and_alt=0.98)
        lengths = None
    else:
        reads = {str(chrom): DecodedReads(**fixture_reads(fx, i)) for i, chrom in enumerate(fx['chroms'])}
        reads['empty'] = DecodedReads(**cr.make_reads([]))
        kwargs = threshold_kwargs(fx['thresholds'][0])
        lengths = {str(chrom): int(fx['length']) for chrom in fx['chroms']}
    ctx = RestatementContext()
    cap = 7
    got = find_candidate_positions(reads, max_fragment_step=step, chromosome2length=lengths, max_snp_candidates=cap, on_context=ctx, **kwargs)
    assert list(got) == list(reads)
    asked = iter(ctx.windows)
    for chrom, chromosome_reads in reads.items():
        assert got[chrom].dtype == np.int32
        if chromosome_reads.n_reads == 0:
            assert len(got[chrom]) == 0
            continue
        arrays = chromosome_reads.arrays()
        length = lengths[chrom] if lengths else max(cr.reference_end(arrays, r) for r in range(chromosome_reads.n_reads))
        want = []
        for k in range((length + step - 1) // step):
            window = (k * step, min((k + 1) * step, length))
            assert next(asked) == window
            part = cr.candidates(cr.coverage(arrays, *window), window[0], max_snp_candidates=cap, **kwargs)
            assert len(part) <= cap
            want.append(part)
        assert np.array_equal(got[chrom], np.concatenate(want))
        assert np.all(np.diff(got[chrom]) > 0)
        assert np.array_equal(got[chrom], cr.find_candidates(arrays, length, max_fragment_step=step, max_snp_candidates=cap, **kwargs))
    assert next(asked, None) is None
    if step == 1:
        assert list(got['tiny']) == [4, 6]  # 3 G + 2 T at 4, 3 A + 2 T at 6; 5 T at 5 have no alt


def test_default_length_is_the_largest_reference_end():
    from demuxalot_amd import DecodedReads
    from demuxalot_amd.snp_detection import reference_ends
    rows = [(5, '2S 3M 4D 2M 10N 1M 2H', 'AAAAAAAA', 30), (7, '1M', 'A', 30), (9, '3= 2X 1I', 'AAAAAA', 30)]
    reads = DecodedReads(**cr.make_reads(rows))
    assert list(reference_ends(reads)) == [5 + 3 + 4 + 2 + 10 + 1, 8, 14]
    assert list(reference_ends(reads)) == [cr.reference_end(reads.arrays(), r) for r in range(3)]


def test_c_entry_points_validate_their_arguments_without_a_gpu():
    """Null and out-of-range arguments are refused before any device work (the library loads without a GPU)."""
    import ctypes
    from demuxalot_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(0)
    assert lib.dmx_coverage_count(None, None, 0, 10, 15, None) != 0
    assert lib.dmx_coverage_candidates(None, 1.0, 0.01, 1.0, 0.98, 10, ctypes.byref(n)) != 0
    assert lib.dmx_coverage_fetch_candidates(None, None, None) != 0
    assert lib.dmx_set_coverage_form(None, 0) != 0
    assert len(_lib.COVERAGE_STAGES) == 6
