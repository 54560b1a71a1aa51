"""SNP detection on the GPU at the edges of its kernels (csrc/snp_detect.hip, csrc/pairwise_sum.h) on the designed problems of
tests/snp_detection_problems.py (what each holds is asserted without a GPU by tests/test_snp_detection_problems_cpu.py): every regime
of the overall ranking's row sum, runs of equal keys against the cap and the chunks of the count, inputs that keep nothing, extreme
positions and chrom values, zero-bit key fields, the filter's values, regularizations the façade refuses, the selection's arithmetic
and the state of one context across calls.  Every case compares with the restatement of tests/test_snp_detection_cpu.py: integers
equal, importances bit for bit, selections equal; there is no tolerance here."""
import functools

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import snp_detection_problems as sp
from tests import test_snp_detection_cpu as r

pytestmark = pytest.mark.gpu

P_BELOW = np.float32(0.01)


def _context():
    from demuxalot_amd.device import get_context
    return get_context()


def _fresh():
    from demuxalot_amd.device import DeviceContext
    return DeviceContext(0)


def _count_and_score(ctx, parts, dob, D, reg=3., cap=3, threshold=P_BELOW):
    n = ctx.snp_count(sp.containers(parts), dob, D, threshold, cap)
    scored = ctx.snp_score(reg)
    assert len(scored['pos']) == n
    return scored


def _assert_same_floats(got, want, what):
    """Bit for bit, but for NaN, where only the place must agree (the sign and payload of a NaN are the hardware's)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fio.assert_bitwise(np.where(np.isnan(got), 0., got), np.where(np.isnan(want), 0., want), what)


def _restate(parts, dob, D, reg=3., cap=3, threshold=P_BELOW):
    chrom, pos, counts = r.count(None, dob, D, cap, parts=parts, p_below=threshold)
    with np.errstate(all='ignore'):
        importances, bases, totals = r.score(counts, reg)
    return dict(chrom=chrom, pos=pos, counts=counts, importances=importances, bases=bases, base_totals=totals)


def _check_scored(scored, want):
    assert scored['chrom'].dtype == np.int32 and scored['pos'].dtype == np.int32
    assert np.array_equal(scored['chrom'], want['chrom']) and np.array_equal(scored['pos'], want['pos'])
    assert scored['counts'].dtype == np.int32 and np.array_equal(scored['counts'], want['counts'])
    _assert_same_floats(scored['importances'], want['importances'], 'importances')
    assert np.array_equal(scored['bases'], want['bases']) and np.array_equal(scored['base_totals'], want['base_totals'])


def _select(importances, n_best, n_add):
    with np.errstate(all='ignore'):
        return r.select(importances, n_best, n_add)


# ---- the row sum of the overall ranking ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', sp.TWIN_DONORS)
def test_twin_positions_rank_by_numpys_row_sum(D):
    """Row sums an ulp apart, and exact duplicates: the ranking is numpy's only if the sum is associated as numpy associates it (8-lane
    blocks up to 128 donors, splits above; at 7689, 7951 and 8191 donors six splits still leave more than a block) and ties stay in
    the canonical order."""
    P = sp.TWIN_P
    parts, dob, counts, _rolls = sp.twin_positions(D, seed=sp.TWIN_SEEDS[D])
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D)
    want = _restate(parts, dob, D)
    assert np.array_equal(want['counts'], counts)
    _check_scored(scored, want)
    importances = want['importances']
    ranking = sp.ranking_via_select(ctx.snp_select, P)
    assert np.array_equal(ranking, np.argsort(-importances.sum(axis=1), kind='stable')), \
        f'{int((ranking != np.argsort(-importances.sum(axis=1), kind="stable")).sum())} of {P} ranks differ'
    for n_best, n_add in [(0, 0), (1, 0), (2, 0), (P - 1, 0), (P, 0), (P + 1, 0), (1, 5)]:
        assert np.array_equal(ctx.snp_select(n_best, n_add), _select(importances, n_best, n_add)), (n_best, n_add)


def test_facade_at_200_donors():
    from demuxalot_amd import BarcodeHandler, select_snps_from_calls
    D = 200
    parts, dob, _counts, _rolls = sp.twin_positions(D, seed=0)
    handler = BarcodeHandler([f'BC{b:06d}' for b in range(len(dob))])
    barcode2donor = {f'BC{b:06d}': f'donor{d:04d}' for b, d in enumerate(dob)}
    result = select_snps_from_calls({'chrT': parts[0][1]}, handler, barcode2donor, n_best_snps_per_donor=1, n_additional_best_snps=7)
    want = _restate(parts, dob, D)
    selected = _select(want['importances'], 1, 7)
    assert 7 < len(selected) < sp.TWIN_P
    assert [(c, p) for c, p, *_ in result] == [('chrT', int(want['pos'][i])) for i in selected]
    fio.assert_bitwise(np.stack([imp for _, _, imp, _ in result]), want['importances'][selected], 'importances')
    assert [list(bc.values()) for *_, bc in result] == want['base_totals'][selected].tolist()
    assert [['ACGT'.index(b) for b in bc] for *_, bc in result] == want['bases'][selected].tolist()


# ---- the cap and the chunks of the count -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', sp.RUN_OFFSETS)
def test_runs_across_chunks_and_workgroups_at_every_cap(offset):
    """Runs of 1 .. 4097 equal keys starting `offset` keys later: the look-back key[i - cap] stays in the lane's 16 keys, reaches the
    lane before, another workgroup's keys, or further back than there are keys (cap 2^31 - 1); cap 0 counts nothing."""
    parts, dob, D, _starts = sp.run_problem(offset)
    ctx = _context()
    for cap in sp.RUN_CAPS:
        scored = _count_and_score(ctx, parts, dob, D, cap=cap)
        assert np.array_equal(scored['counts'], sp.run_counts(offset, sp.RUN_LENGTHS, cap)), cap
        assert list(scored['pos']) == ([5, 9] if offset else [9])
    _check_scored(scored, _restate(parts, dob, D, cap=sp.RUN_CAPS[-1]))


@pytest.mark.parametrize('m', sp.KEPT_TOTALS)
def test_kept_call_totals_around_the_chunks(m):
    parts, dob, D, cap = sp.kept_total_problem(m)
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D, cap=cap)
    want = _restate(parts, dob, D, cap=cap)
    _check_scored(scored, want)
    assert np.array_equal(ctx.snp_select(1, 2), _select(want['importances'], 1, 2))


# ---- nothing kept ----------------------------------------------------------------------------------------------------------------------------
def test_nothing_kept():
    """No part, parts without calls, every call filtered: no position, empty arrays of the right shapes and types, an empty selection,
    and no device memory held - on a context that has counted nothing yet and right after a count that kept something."""
    ctx = _fresh()
    try:
        never = ctx.device_bytes()
        good_parts, good_dob, good_D = sp.one_position()
        for name, (parts, dob, D, threshold) in sp.nothing_kept_problems().items():
            for after_a_count in (False, True):
                if after_a_count:
                    assert ctx.snp_count(sp.containers(good_parts), good_dob, good_D, P_BELOW, 3) == 1
                    ctx.snp_score(3.)
                    assert len(ctx.snp_select(1, 1)) == 1 and ctx.device_bytes() > never
                assert ctx.snp_count(sp.containers(parts), dob, D, threshold, 3) == 0, name
                scored = ctx.snp_score(3.)
                for key, shape, dtype in [('chrom', (0,), np.int32), ('pos', (0,), np.int32), ('counts', (0, D, 4), np.int32),
                                          ('importances', (0, D), np.float64), ('bases', (0, 2), np.uint8), ('base_totals', (0, 2), np.int64)]:
                    assert scored[key].shape == shape and scored[key].dtype == dtype, (name, key)
                for n_best, n_add in [(0, 0), (3, 5), (2 ** 40, 2 ** 40)]:
                    selected = ctx.snp_select(n_best, n_add)
                    assert selected.shape == (0,) and selected.dtype == np.int64, name
                held = ctx.device_bytes()
                ctx.release_problem()
                freed = held - ctx.device_bytes()
                assert ctx.device_bytes() == never and held == never + freed and freed >= 0, name
                with pytest.raises(Exception, match='call order'):
                    ctx.snp_score(3.)
    finally:
        ctx.close()


# ---- keys and order ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('problem', [
    lambda: sp.positions_problem(sp.EXTREME_CHROMS, sp.EXTREME_POSITIONS),
    lambda: sp.positions_problem(sp.SCATTERED_CHROMS, (3, 10, 11)),
    sp.one_donor_one_barcode,
    sp.one_position,
], ids=['extreme positions', 'chrom values', 'one donor one barcode', 'one position'])
def test_keys_and_order(problem):
    """INT32_MIN .. INT32_MAX through the biased position key; repeated, out-of-order and large chrom values (the canonical order is the
    value's; equal values merge, runs and all); donor and barcode fields of zero bits; a single position."""
    parts, dob, D = problem()
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D)
    want = _restate(parts, dob, D)
    _check_scored(scored, want)
    P = len(want['pos'])
    assert np.array_equal(sp.ranking_via_select(ctx.snp_select, P), np.argsort(-want['importances'].sum(axis=1), kind='stable'))
    for n_best, n_add in [(1, 0), (1, 1), (P, 0), (0, P)]:
        assert np.array_equal(ctx.snp_select(n_best, n_add), _select(want['importances'], n_best, n_add))


# ---- the filter --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threshold', sp.THRESHOLDS, ids=['0.01', 'inf', '-0', '0'])
def test_filter_values(threshold):
    """NaN, negative, signed zeros, float32(0.01) and infinite p_base_wrong against the threshold as numpy's float32 `<` has it;
    base_index 4, 5 and 255; a barcode without donor."""
    parts, dob, D = sp.filter_problem()
    scored = _count_and_score(_context(), parts, dob, D, threshold=threshold)
    want = _restate(parts, dob, D, threshold=threshold)
    assert len(want['pos']) in (4, 16, 24)
    _check_scored(scored, want)


# ---- scores outside the façade's range ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tied_problem():
    rng = np.random.default_rng(11)
    parts = sp.random_parts(rng, 2, 3000, 30, 40)
    dob = rng.integers(-1, 3, 30).astype(np.int32)
    return parts, dob, 3


@pytest.mark.parametrize('reg', [0., 1e-300, 1e300])
def test_regularizations_at_the_ends_of_the_range(reg):
    parts, dob, D = _tied_problem()
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D, reg=reg)
    want = _restate(parts, dob, D, reg=reg)
    assert np.isfinite(want['importances']).all()
    _check_scored(scored, want)
    for n_best, n_add in [(0, 7), (2, 0), (2, 7)]:
        assert np.array_equal(ctx.snp_select(n_best, n_add), _select(want['importances'], n_best, n_add))


def test_infinite_regularization_ranks_in_the_canonical_order():
    """inf * p_avg / inf: every importance is NaN.  snp_detect.hip's contract for the rankings is "larger first, NaN last", stable: all
    equal, so every ranking is the canonical order (numpy's stable argsort of all-NaN keys agrees)."""
    parts, dob, D = _tied_problem()
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D, reg=np.inf)
    want = _restate(parts, dob, D, reg=np.inf)
    assert np.isnan(want['importances']).all() and np.isnan(scored['importances']).all()
    _check_scored(scored, want)
    P = len(want['pos'])
    for k in range(P + 1):
        assert np.array_equal(ctx.snp_select(0, k), np.arange(k))
    assert np.array_equal(ctx.snp_select(2, 0), [0, 1]) and np.array_equal(ctx.snp_select(2, 3), [0, 1, 2, 3, 4])


def test_negative_regularization_with_infinite_importances():
    """A regularization that cancels (c0 + c1) of some donors exactly: their importances are +inf (NaN where the numerator is 0 too), and
    those positions lead the rankings, in the canonical order among themselves."""
    parts, dob, D = _tied_problem()
    counts = r.count(None, dob, D, parts=parts)[2]
    bases = r.score(counts)[1]
    rows = np.arange(len(counts))
    pairs = (counts[rows, :, bases[:, 1]] + 1e-4) + (counts[rows, :, bases[:, 0]] + 1e-4)  # (c0 + c1) as the score forms it
    values, n = np.unique(pairs, return_counts=True)
    reg = -float(values[np.argmax(n)])
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D, reg=reg)
    want = _restate(parts, dob, D, reg=reg)
    infinite = np.isinf(want['importances'])
    assert infinite.any() and not infinite.all(axis=1).all() and (want['importances'][infinite] > 0).all()
    _check_scored(scored, want)
    P = len(want['pos'])
    with np.errstate(all='ignore'):
        ranking = np.argsort(-want['importances'].sum(axis=1), kind='stable')
    assert np.array_equal(sp.ranking_via_select(ctx.snp_select, P), ranking)
    for n_best, n_add in [(1, 0), (3, 2), (P, 0)]:
        assert np.array_equal(ctx.snp_select(n_best, n_add), _select(want['importances'], n_best, n_add))


# ---- the selection's arithmetic ----------------------------------------------------------------------------------------------------------------
def test_selection_arithmetic_at_the_number_of_new_positions():
    parts, dob, D = _problem(5, 240, 12, 60, 3)  # few calls per position: many positions with equal counts
    ctx = _context()
    scored = _count_and_score(ctx, parts, dob, D)
    want = _restate(parts, dob, D)
    _check_scored(scored, want)
    importances = want['importances']
    P = len(importances)
    assert len(np.unique(importances.sum(axis=1))) < P - 5 and len(np.unique(importances[:, 0])) < P - 5  # ties
    seen = set()
    for n_best in (0, 1, P - 1, P, P + 1, 2 ** 40):
        n_new = P - len(np.unique(np.argsort(-importances, axis=0, kind='stable')[:n_best]))
        seen.add(n_new)
        for n_add in sorted({0, 1, n_new - 1, n_new, n_new + 1, 2 ** 40} - {-1}):
            assert np.array_equal(ctx.snp_select(n_best, n_add), _select(importances, n_best, n_add)), (n_best, n_add, n_new)
    assert 0 in seen and P in seen and len(seen) >= 3


# ---- one context across calls ---------------------------------------------------------------------------------------------------------------------
def _problem(seed, n_calls, n_barcodes, n_positions, D):
    rng = np.random.default_rng(seed)
    return sp.random_parts(rng, 2, n_calls, n_barcodes, n_positions), rng.integers(-1, D, n_barcodes).astype(np.int32), D


def test_one_context_sees_nothing_stale():
    """A smaller and then a larger problem on the context of another; a second score; a second select; a refused count."""
    A, B, C = _problem(1, 4000, 50, 80, 5), _problem(2, 300, 9, 6, 2), _problem(3, 9000, 120, 300, 9)
    ctx = _fresh()
    try:
        for parts, dob, D in (A, B, C):
            scored = _count_and_score(ctx, parts, dob, D)
            want = _restate(parts, dob, D)
            _check_scored(scored, want)
            other = _fresh()
            try:
                alone = _count_and_score(other, parts, dob, D)
                for key in scored:
                    assert scored[key].tobytes() == alone[key].tobytes(), key
                for n_best, n_add in [(2, 3), (0, 5), (4, 0)]:
                    selected = ctx.snp_select(n_best, n_add)
                    assert np.array_equal(selected, other.snp_select(n_best, n_add))
                    assert np.array_equal(selected, _select(want['importances'], n_best, n_add))
            finally:
                other.close()
        # score with 3, then with 0.5: the selection is that of 0.5; selecting twice changes nothing
        assert len(A[0]) and ctx.snp_count(sp.containers(A[0]), A[1], A[2], P_BELOW, 3) == len(_restate(*A)['pos'])
        ctx.snp_score(3.)
        first = ctx.snp_select(2, 3)
        scored = ctx.snp_score(0.5)
        want = _restate(*A, reg=0.5)
        _check_scored(scored, want)
        assert not np.array_equal(_select(want['importances'], 2, 3), _select(_restate(*A)['importances'], 2, 3))
        assert np.array_equal(first, _select(_restate(*A)['importances'], 2, 3))
        for _ in range(2):
            assert np.array_equal(ctx.snp_select(2, 3), _select(want['importances'], 2, 3))
        # a refused count leaves nothing to score or to select from
        bad = A[0][0][1]
        calls = bad.snp_calls[:bad.n_snp_calls].copy()
        calls['molecule_index'][len(calls) // 2] = bad.n_molecules
        with pytest.raises(Exception, match='molecule_index outside the molecule table'):
            ctx.snp_count([(0, calls, bad.molecules[:bad.n_molecules])], A[1], A[2], P_BELOW, 3)
        with pytest.raises(Exception, match='call order'):
            ctx.snp_score(3.)
        with pytest.raises(Exception, match='call order'):
            ctx.snp_select(2, 3)
        # and the context counts again
        _check_scored(_count_and_score(ctx, *B), _restate(*B))
    finally:
        ctx.close()


@pytest.mark.parametrize('change, message', [
    (dict(D=0), r'n_donors must be 1\.\.8192'),
    (dict(D=8193), r'n_donors must be 1\.\.8192'),
    (dict(cap=-1), 'cap must be >= 0'),
    (dict(dob_entry=-2), r'donor_of_barcode\[4\] out of range'),
    (dict(dob_entry='D'), r'donor_of_barcode\[4\] out of range'),
    (dict(chrom=-1), 'container chrom must be >= 0'),
], ids=['no donor', '8193 donors', 'cap -1', 'donor -2', 'donor D', 'chrom -1'])
def test_refused_arguments(change, message):
    parts, dob, D = _problem(2, 300, 9, 6, 2)
    ctx = _fresh()
    try:
        _count_and_score(ctx, parts, dob, D)
        dob = dob.copy()
        if 'dob_entry' in change:
            dob[4] = D if change['dob_entry'] == 'D' else change['dob_entry']
        given = sp.containers(parts)
        if 'chrom' in change:
            given[1] = (change['chrom'],) + given[1][1:]
        with pytest.raises(Exception, match=message):
            ctx.snp_count(given, dob, change.get('D', D), P_BELOW, change.get('cap', 3))
    finally:
        ctx.close()
