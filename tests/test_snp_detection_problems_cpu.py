"""The designed problems of tests/snp_detection_problems.py hold what their docstrings claim, and the ones that are there to notice a
wrong association of the overall ranking's row sum do notice one: on the committed seeds the ranking read through select changes under a
sequential sum at every donor count from 8 on, and under numpy's tree limited to six splits (csrc/snp_detect.hip's row sum before
csrc/pairwise_sum.h) at the donor counts where that tree differs from numpy's - and nowhere else.  No GPU."""
import functools

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import snp_detection_problems as sp
from tests import test_snp_detection_cpu as r

P = sp.TWIN_P


@functools.lru_cache(maxsize=None)
def twin(D):
    parts, dob, counts, rolls = sp.twin_positions(D, seed=sp.TWIN_SEEDS[D])
    importances = r.score(counts)[0]
    importances.flags.writeable = False
    return parts, dob, counts, rolls, importances


def ranking_under(importances, row_sum=None):
    sums = None if row_sum is None else row_sum(importances)  # (once, not at every select)
    return sp.ranking_via_select(lambda n_best, n_add: r.select(importances, n_best, n_add, row_sum and (lambda _: sums)), len(importances))


# ---- the explicit container list and the read-out of the ranking ---------------------------------------------------------------------------
def test_explicit_parts_restate_the_dict():
    _fx, calls, _genotypes, handler = r.load('f8_snp_synthetic.npz')
    dob = (np.arange(len(handler.ordered_barcodes)) % 4 - 1).astype(np.int32)
    parts = list(enumerate(calls.values()))
    assert len(parts) > 1
    for a, b in zip(r.flat_calls(calls), r.flat_calls(None, parts)):
        assert np.array_equal(a, b)
    want = r.count(calls, dob, 3)
    for order in (parts, parts[::-1]):  # the canonical order is the chrom VALUE's, whatever the list's
        for a, b in zip(r.count(None, dob, 3, parts=order), want):
            assert np.array_equal(a, b)
    assert r.count(calls, dob, 3, p_below=np.inf)[2].sum() >= want[2].sum() > r.count(calls, dob, 3, p_below=0.)[2].sum() == 0


def test_ranking_via_select_reads_the_ranking():
    rng = np.random.default_rng(0)
    importances = rng.integers(0, 3, (37, 5)).astype(np.float64)  # full of ties
    want = np.argsort(-importances.sum(axis=1), kind='stable')
    assert len(np.unique(importances.sum(axis=1))) < 15
    assert np.array_equal(ranking_under(importances), want)
    assert np.array_equal(ranking_under(importances, sp.tree_row_sum), want)
    for n_add in (0, 3, 50):  # (select without its per-donor sort at n_best = 0 is what [:0] leaves of it)
        assert np.array_equal(r.select(importances, 0, n_add), np.sort(want[:n_add]))


# ---- twin positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', sp.TWIN_DONORS)
def test_twin_positions_hold_what_they_claim(D):
    parts, dob, counts, rolls, importances = twin(D)
    (_chrom, calls), = parts
    assert counts.shape == (P, D, 4) and set(np.unique(counts)) <= {0, 1} and (counts.sum(axis=(0, 1)) > 0).sum() <= 2
    assert 0.4 * P * D <= calls.n_snp_calls <= 2 * P * D and len(dob) in (D, 2 * D)
    chrom, pos, restated = r.count(None, dob, D, cap=3, parts=parts)
    assert np.array_equal(restated, counts) and np.array_equal(pos, 100 + 3 * np.arange(P)) and not chrom.any()
    # rotations of one pattern: row p is row q rolled by rolls[p] - rolls[q]
    for p in (1, P // 2, P - 1):
        assert np.array_equal(counts[p], np.roll(counts[0], rolls[p] - rolls[0], axis=0))
    # exact duplicates, which only stability orders
    twins = [(p, q) for p in range(P) for q in range(p + 1, P) if rolls[p] == rolls[q]]
    assert len(twins) >= sp.TWIN_DUPLICATES
    for p, q in twins[:8]:
        fio.assert_bitwise(importances[p], importances[q], 'twin rows')
    # one sum mathematically; a handful of float64 values next to each other
    sums = importances.sum(axis=1)
    assert np.array_equal(sp.tree_row_sum(importances).view(np.uint64), sums.view(np.uint64))
    distinct = np.unique(sums)
    assert len(distinct) <= 16 and (D < 8 or len(distinct) >= 2), distinct
    assert (distinct[-1] - distinct[0]) <= 64 * np.spacing(distinct[0])
    want = np.argsort(-sums, kind='stable')
    if D in (1, 9, 8191):  # (the read-out through 129 selects is what the device is asked; once here per regime is enough)
        assert np.array_equal(ranking_under(importances), want)
    for p, q in twins[:8]:
        assert list(want).index(p) < list(want).index(q)


def test_the_affected_donor_counts_by_the_predicate():
    affected = [D for D in range(1, 8193) if sp.overlong_block(D)]
    assert len(affected) == 441 and affected[0] == 7689 and affected[-1] == 8191
    listed = [D for D in sp.TWIN_DONORS if sp.overlong_block(D)]
    assert len(listed) == 3 and {7689, 8191} < set(listed)
    assert not sp.overlong_block(7688) and not sp.overlong_block(8192) and {7688, 8192} < set(sp.TWIN_DONORS)
    assert not any(sp.overlong_block(D, depth=7) for D in range(1, 8193))


@pytest.mark.parametrize('D', [D for D in sp.TWIN_DONORS if D >= 8])
def test_a_sequential_sum_changes_the_ranking(D):
    importances = twin(D)[4]
    assert sp.sequential_row_sum in sp.twin_mutants(D)
    moved = ranking_under(importances, sp.sequential_row_sum) != np.argsort(-importances.sum(axis=1), kind='stable')
    assert moved.any(), f'D = {D}, seed {sp.TWIN_SEEDS[D]}: a sequential row sum ranks as numpy does; the seed proves nothing'


@pytest.mark.parametrize('D', [D for D in sp.TWIN_DONORS if sp.overlong_block(D)])
def test_a_tree_of_six_splits_changes_the_ranking(D):
    importances = twin(D)[4]
    assert sp.depth6_row_sum in sp.twin_mutants(D)
    moved = ranking_under(importances, sp.depth6_row_sum) != np.argsort(-importances.sum(axis=1), kind='stable')
    assert moved.any(), f'D = {D}, seed {sp.TWIN_SEEDS[D]}: the six-split tree ranks as numpy does; the seed proves nothing'


@pytest.mark.parametrize('D', [7688, 8192])
def test_a_tree_of_six_splits_is_numpy_on_both_sides_of_the_affected_counts(D):
    importances = twin(D)[4]
    fio.assert_bitwise(sp.depth6_row_sum(importances), importances.sum(axis=1), 'row sums')


@pytest.mark.parametrize('D', [8, 9, 129])
def test_the_seed_search_finds_the_committed_seeds(D):
    assert sp.search_twin_seed(D, r.score) == sp.TWIN_SEEDS[D]


# ---- runs ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', sp.RUN_OFFSETS)
def test_run_problem_counts_have_the_closed_form(offset):
    parts, dob, D, starts = sp.run_problem(offset)
    _chrom, _pos, base, cb, _p = r.flat_calls(None, parts)
    assert len(cb) == sum(sp.RUN_LENGTHS) + offset
    # the sorted keys of the count: the singles' position first, then the runs back to back in the order of RUN_LENGTHS
    pos = r.flat_calls(None, parts)[1]
    unsorted = ((pos == 9) * 4 + base) * D * len(dob) + dob[cb] * len(dob) + cb
    key = np.sort(unsorted)
    heads = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    assert np.array_equal(heads[offset:], starts) and np.array_equal(heads[:offset], np.arange(offset))
    assert np.array_equal(np.diff(np.concatenate([heads[offset:], [len(key)]])), sp.RUN_LENGTHS)
    assert not np.array_equal(unsorted, key)  # (the input is not in key order)
    for start, length in zip(starts, sp.RUN_LENGTHS):
        if length >= 4095:  # the long runs lie across a workgroup's last key
            assert start // sp.COUNT_BLOCK < (start + length - 1) // sp.COUNT_BLOCK
    for cap in sp.RUN_CAPS:
        chrom, pos, counts = r.count(None, dob, D, cap=cap, parts=parts)
        assert list(pos) == ([5, 9] if offset else [9])
        assert np.array_equal(counts, sp.run_counts(offset, sp.RUN_LENGTHS, cap))
        assert counts[-1].sum() == sum(min(length, cap) for length in sp.RUN_LENGTHS)


def test_run_problem_offsets_put_every_run_at_every_place_of_a_chunk():
    starts = np.array([sp.run_problem(offset)[3] for offset in sp.RUN_OFFSETS])
    for run in range(len(sp.RUN_LENGTHS)):
        assert set(starts[:, run] % sp.COUNT_CHUNK) == set(range(sp.COUNT_CHUNK))
    assert set(sp.RUN_CAPS) >= {0, sp.COUNT_CHUNK - 1, sp.COUNT_CHUNK, sp.COUNT_CHUNK + 1, sp.COUNT_BLOCK}


@pytest.mark.parametrize('m', sp.KEPT_TOTALS)
def test_kept_total_problem_keeps_exactly_m(m):
    parts, dob, D, cap = sp.kept_total_problem(m)
    _chrom, _pos, base, cb, p = r.flat_calls(None, parts)
    assert int(((p < r.P_BELOW) & (base < 4) & (dob[cb] >= 0)).sum()) == m and len(p) == m + m // 2 + 3
    assert r.count(None, dob, D, cap=cap, parts=parts)[2].sum() <= m


# ---- the filter, nothing kept --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threshold, kept_p', [
    (sp.THRESHOLDS[0], (-1., -0., 0., 0.0099)),
    (sp.THRESHOLDS[1], (-1., -0., 0., 0.0099, np.float32(0.01), 1.)),
    (sp.THRESHOLDS[2], (-1.,)),
    (sp.THRESHOLDS[3], (-1.,)),
])
def test_filter_problem_keeps_what_float32_less_than_keeps(threshold, kept_p):
    parts, dob, D = sp.filter_problem()
    assert parts[0][1].n_snp_calls == len(sp.P_VALUES) * len(sp.BASE_VALUES) * 3
    _chrom, pos, counts = r.count(None, dob, D, cap=3, parts=parts, p_below=threshold)
    kept_p = np.asarray(kept_p, dtype=np.float32)
    want = sorted(16 * ip + ib for ip, p in enumerate(sp.P_VALUES) for ib, base in enumerate(sp.BASE_VALUES)
                  if base < 4 and np.any(p == kept_p))
    assert list(pos) == want and len(want) == 4 * len(kept_p)
    assert (counts.sum(axis=2) == 1).all()  # barcodes 0 and 2 of donors 0 and 1; barcode 1 has no donor


def test_nothing_kept_problems_keep_nothing():
    problems = sp.nothing_kept_problems()
    assert len(problems) == 7
    for name, (parts, dob, D, threshold) in problems.items():
        chrom, pos, counts = r.count(None, dob, D, parts=parts, p_below=threshold)
        assert len(chrom) == 0 and len(pos) == 0 and counts.shape == (0, D, 4), name
        importances, bases, totals = r.score(counts)
        assert importances.shape == (0, D) and bases.shape == (0, 2) and totals.shape == (0, 2), name
    # the two thresholds are what drops the calls of their inputs
    for name in ('threshold 0', 'threshold NaN'):
        parts, dob, D, _threshold = problems[name]
        assert len(r.count(None, dob, D, parts=parts)[1]) > 0
    assert sum(calls.n_snp_calls for _c, calls in problems['parts without calls'][0]) == 0 and problems['no part'][0] == []


# ---- keys and order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chroms, positions', [(sp.EXTREME_CHROMS, sp.EXTREME_POSITIONS), (sp.SCATTERED_CHROMS, (3, 10, 11))])
def test_positions_problem_order_and_merged_parts(chroms, positions):
    parts, dob, D = sp.positions_problem(chroms, positions)
    assert [c for c, _ in parts] == list(chroms) and len(set(chroms)) < len(chroms) and list(chroms) != sorted(chroms)
    chrom, pos, counts = r.count(None, dob, D, cap=3, parts=parts)
    want = [(c, p) for c in sorted(set(chroms)) for p in sorted(positions)]
    assert list(zip(chrom.tolist(), pos.tolist())) == want and max(chroms) >= 2 ** 31 - 2
    # a repeated chrom: barcode 0's calls of base 0 at positions[0] make one run across its parts, and the cap cuts it
    repeated = max(set(chroms), key=list(chroms).count)
    at = want.index((repeated, positions[0]))
    uncapped = r.count(None, dob, D, cap=100, parts=parts)[2]
    assert uncapped[at, 0, 0] >= 2 * list(chroms).count(repeated) > 3 and uncapped[at].sum() - counts[at].sum() >= 1


def test_tiny_problems():
    parts, dob, D = sp.one_donor_one_barcode()
    chrom, pos, counts = r.count(None, dob, D, cap=3, parts=parts)
    assert D == 1 and len(dob) == 1 and list(pos) == [-4, 0, 4, 9]
    assert counts[:, 0].tolist() == [[0, 0, 0, 1], [0, 2, 1, 0], [3, 0, 0, 0], [2, 0, 0, 2]]
    parts, dob, D = sp.one_position()
    chrom, pos, counts = r.count(None, dob, D, cap=3, parts=parts)
    assert list(chrom) == [2] and list(pos) == [-7] and counts.shape == (1, 3, 4) and counts.sum() > 10
