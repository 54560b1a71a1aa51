"""The posterior read-outs at their kernels' shape edges, on designed posteriors (tests/readout_designs.py): k_top_options<1..4>,
k_option_partial / k_option_final, k_allowed_mass and k_donor_readout of csrc/results.hip, k_assign of csrc/kernels.hip,
dmx_get_block.

The input of every reference computation is P = ctx.get_probs(), the float32 matrix the kernels read; no expectation comes from
a design.  Every test first asserts on P that the matrix has the edge it is about (designs.structure: bit-equal ties, exact
zeros, an all-NaN row), so that it cannot pass on a matrix that lacks it.

Every case is a matrix of at most 1025 x 257, or 5 x 8256; the 228 cases take about four seconds on an MI355X.

Three one-line changes of csrc/results.hip were run against this file when it was written.  better() preferring the higher column
among equals fails the designs with ties or zeros (159 cases); an insertion that drops the displaced candidate instead of pushing
it down fails the lanes that meet their largest value last (51 cases); k_option_partial with B / 512 rows per slab fails the sums
at every B but 512 (16 cases).  Leaving out the clearing of the last register when a lane pops its head changes no output - TOP
rounds pop a lane at most TOP times, and the stale copy would be the (TOP + 1)-th - and no case fails on it."""
import math

import numpy as np
import pytest

from tests import donor_readout_restatement as restated
from tests import fixture_io as fio
from tests import readout_designs as designs
from tests.test_gpu_donor_readout import assert_readout

pytestmark = pytest.mark.gpu

F32 = np.float32


def installed(design, B):
    return designs.install(*design, B)


def stable_top(P, k):
    """(columns int32[B, k], probabilities float32[B, k]) of the k best options, ties to the lower column; -1 / NaN past a short row."""
    B, K = P.shape
    order = np.argsort(-P, axis=1, kind='stable')[:, :k]
    columns, probs = np.full((B, k), -1, dtype=np.int32), np.full((B, k), np.nan, dtype=np.float32)
    columns[:, :order.shape[1]] = order
    probs[:, :order.shape[1]] = np.take_along_axis(P, order, axis=1)
    return columns, probs


def check_top_options(ctx, P, what):
    for k in (1, 2, 3, 4):
        options, probs = ctx.get_top_options(k)
        want_options, want_probs = stable_top(P, k)
        assert options.dtype == np.int32 and np.array_equal(options, want_options), (what, k, options[:4], want_options[:4])
        fio.assert_bitwise(probs, want_probs, f'{what}: top {k} probabilities')


def check_argmax_read_outs(ctx, P, what):
    """get_assignments, get_top_options(1) and get_assignments_above(t) against np.argmax / the row maximum, and each other."""
    B = len(P)
    top, peak = np.argmax(P, axis=1).astype(np.int32), P.max(axis=1)
    best, prob = ctx.get_assignments()
    assert np.array_equal(best, top), (what, best[:8], top[:8])
    fio.assert_bitwise(prob, peak, f'{what}: get_assignments probability')
    options, probs = ctx.get_top_options(1)
    assert np.array_equal(options[:, 0], top), what
    fio.assert_bitwise(probs[:, 0], peak, f'{what}: get_top_options(1) probability')
    one = peak[B // 2]  # below every row maximum; one row's maximum; a float32 step to either side of it
    for t in (np.nextafter(peak.min(), F32(-1)), one, np.nextafter(one, F32(-1)), np.nextafter(one, F32(2))):
        assert np.float32(float(t)) == t
        above, prob_t, n = ctx.get_assignments_above(float(t))
        assigned = peak > t  # `gt` is strict
        assert np.array_equal(above, np.where(assigned, top, -1)), (what, t)
        fio.assert_bitwise(prob_t, peak, f'{what}: get_assignments_above({t}) probability')
        assert n == int(assigned.sum()), (what, t, n)
    _, _, n = ctx.get_assignments_above(float(np.nextafter(peak.min(), F32(-1))))
    assert n == B, what


def check_donor_read_out(ctx, P, G, what):
    got = ctx.get_donor_readout(marginals=True)
    assert_readout(got, P, G, what)
    # the better of (best singlet, best pair) - larger value, lower column - is the overall arg-max
    pair_wins = (got['best_pair'] >= 0) & (got['best_pair_prob'] > got['best_singlet_prob'])  # singlet columns come first
    overall = np.where(pair_wins, got['best_pair'], got['best_singlet'])
    assert np.array_equal(overall, np.argmax(P, axis=1)), what
    fio.assert_bitwise(np.where(pair_wins, got['best_pair_prob'], got['best_singlet_prob']), P.max(axis=1), f'{what}: best of both')


@pytest.mark.parametrize('K,name,B', designs.catalogue())
def test_arg_max_and_top_read_outs_on_a_design(K, name, B):
    design = designs.design(name, K, B)
    what = f'{name} K={K} B={B}'
    ctx = installed(design, B)
    try:
        P = ctx.get_probs()
        assert P.shape == (B, K) and P.dtype == np.float32
        designs.structure(P, designs.designed_logits(name, K, B), what)  # the precondition: P has the designed edge
        check_top_options(ctx, P, what)
        check_argmax_read_outs(ctx, P, what)
        check_donor_read_out(ctx, P, design[0], what)
    finally:
        ctx.close()


def random_posteriors(ctx, K, B, what):
    P = ctx.get_probs()
    assert P.shape == (B, K) and P.dtype == np.float32 and np.isfinite(P).all() and (P >= 0).all(), what
    assert np.allclose(P.astype(np.float64).sum(axis=1), 1, rtol=1e-4, atol=0), what  # (a float32 softmax: K roundings of 2^-24)
    assert B == 1 or K == 1 or len(np.unique(P, axis=0)) == B, f'{what}: rows repeat'
    return P


def restated_option_sums(P):
    """The documented order of dmx_get_option_sums: float64 sums of 512 slabs of ceil(B / 512) consecutive rows in row order,
    then the 512 slabs in order."""
    B, K = P.shape
    per = -(-B // 512)
    total = np.zeros(K, dtype=np.float64)
    for slab in range(512):
        partial = np.zeros(K, dtype=np.float64)
        for b in range(slab * per, min(slab * per + per, B)):
            partial = partial + P[b].astype(np.float64)
        total = total + partial
    return total


@pytest.mark.parametrize('K', [1, 255, 256, 257])
@pytest.mark.parametrize('B', [1, 511, 512, 513, 1025])
def test_option_sums_at_the_slab_and_block_boundaries(B, K):
    """B around the 512 slabs (511: one row per slab and an empty one; 513 and 1025: rows per slab rounded up, a ragged last
    slab and empty ones behind it), K around the 256 columns of a block."""
    what = f'option sums B={B} K={K}'
    ctx = installed(designs.random_design(K, B), B)
    try:
        P = random_posteriors(ctx, K, B, what)
        got = ctx.get_option_sums()
        fio.assert_bitwise(got, restated_option_sums(P), what)
        # math.fsum of a column is its exact sum rounded once; a term of the device's sum passes through at most ceil(B / 512) + 512
        # <= B + 512 float64 additions of non-negative numbers, each within 2^-53 of its result
        exact = np.array([math.fsum(P[:, k].tolist()) for k in range(K)])
        assert (exact > 0).all() and (np.abs(got - exact) <= (B + 512) * 2.0 ** -53 * exact).all(), (what, np.abs(got - exact).max())
    finally:
        ctx.close()


@pytest.mark.parametrize('B,K', [(255, 65), (256, 3), (256, 65), (257, 65)])
def test_allowed_mass_at_the_block_boundary(B, K):
    """One thread per barcode, 256 per block; lists of 0 .. 3 options with and without the row's arg-max, repeats included."""
    what = f'allowed mass B={B} K={K}'
    ctx = installed(designs.random_design(K, B, seed=1), B)
    try:
        P = random_posteriors(ctx, K, B, what)
        top = np.argmax(P, axis=1)
        lists = []
        for b in range(B):
            other = [(int(top[b]) + s) % K for s in (1, 2, 3)]
            lists.append([[], [int(top[b])], [other[0]], [other[0], int(top[b]), other[1]], other, [other[2], other[2], other[0]],
                          [int(top[b])] * 3, [other[1], other[0]]][(b + 3) % 8])
        assert {len(x) for x in lists} == {0, 1, 2, 3} and all(len(x) > 0 for x in lists[254:])  # the threads at the boundary have work
        start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        options = np.asarray([k for x in lists for k in x], dtype=np.int32)
        mass, hit = ctx.get_allowed_mass(start, options)
        want_mass, want_hit = restated.allowed_mass(P, start, options)
        fio.assert_bitwise(mass, want_mass, what)
        assert hit.dtype == np.int32 and np.array_equal(hit, want_hit), what
        assert 0 < hit.sum() < B
    finally:
        ctx.close()


@pytest.mark.parametrize('K', [63, 65, 257])
def test_blocks_at_odd_widths(K):
    """dmx_get_block copies with a pitch of K floats: single elements, the last row and column, strips, empty and refused blocks."""
    from demuxalot_amd import _lib
    from demuxalot_amd.demux import DevicePosteriors
    B = 37
    what = f'blocks K={K}'
    ctx = installed(designs.random_design(K, B, seed=2), B)
    dev = DevicePosteriors(ctx, [f'bc{b}' for b in range(B)], [f'o{k}' for k in range(K)], pooled=False)
    try:
        whole = {'probs': random_posteriors(ctx, K, B, what), 'logits': ctx.get_logits()}
        assert np.isfinite(whole['logits']).all() and not np.array_equal(whole['logits'], whole['probs'])
        blocks = [(17, 18, K // 2, K // 2 + 1), (0, 1, 0, 1), (B - 1, B, K - 1, K),      # single elements
                  (B - 1, B, 0, K), (0, B, K - 1, K), (0, B, 0, 1), (0, B, K // 2, K // 2 + 1),  # the last row; one-column strips
                  (3, 11, 5, K - 2), (0, B, 1, K), (1, B, 0, K - 1), (0, B, 0, K),
                  (5, 5, 0, K), (0, B, 7, 7), (B, B, K, K), (0, 0, 0, 0)]                 # empty
        for name, matrix in whole.items():
            for b0, b1, k0, k1 in blocks:
                got = ctx.get_block(name, b0, b1, k0, k1)
                assert got.shape == (b1 - b0, k1 - k0)
                fio.assert_bitwise(got, matrix[b0:b1, k0:k1], f'{what}: {name}[{b0}:{b1}, {k0}:{k1}]')
            for lo, hi in ((0, 1), (B - 1, B), (7, 20), (0, B), (4, 4)):
                rows = dev.rows(lo, hi, name)
                assert list(rows.index) == dev.barcodes[lo:hi] and list(rows.columns) == dev.columns
                fio.assert_bitwise(rows.values, matrix[lo:hi], f'{what}: rows({lo}, {hi}, {name})')
            for b0, b1, k0, k1 in ((0, B + 1, 0, K), (0, B, 0, K + 1), (-1, B, 0, K), (0, B, -1, K), (B, B + 1, 0, K), (0, 1, K, K + 1)):
                with pytest.raises(_lib.DemuxHipError, match='outside'):
                    ctx.get_block(name, b0, b1, k0, k1)
            for b0, b1, k0, k1 in ((5, 3, 0, K), (0, B, 9, 2)):  # reversed ranges, asked of the library itself
                out = np.empty(B * K, dtype=np.float32)
                with pytest.raises(_lib.DemuxHipError, match='outside'):
                    _lib.check(ctx._lib.dmx_get_block(ctx._h, {'logits': 0, 'probs': 1}[name], b0, b1, k0, k1, _lib.ptr(out)))
        fio.assert_bitwise(ctx.get_block('probs'), whole['probs'], f'{what}: after the refusals')
    finally:
        dev.close()


@pytest.mark.parametrize('K', [3, 65, 321, 2080])
def test_a_row_without_a_non_nan_posterior_gets_one_answer(K):
    """A NaN in one barcode's float32 prior logits: the softmax leaves that row all NaN.  Every read-out answers it alike: option -1,
    probability NaN, not counted, absent from assignments(), None in best() and top_options().  Finite rows are as ever."""
    from demuxalot_amd.demux import DevicePosteriors
    B, row = 5, 2
    design = designs.nan_design(K, B, row, K // 2)
    what = f'NaN row K={K}'
    ctx = installed(design, B)
    dev = DevicePosteriors(ctx, [f'bc{b}' for b in range(B)], [f'o{k}' for k in range(K)], pooled=False, n_donors=design[0])
    try:
        P = ctx.get_probs()
        assert np.isnan(P[row]).all() and np.isfinite(np.delete(P, row, axis=0)).all(), f'{what}: {P[row][:8]}'  # the precondition
        designs.structure(P, design[3], what)
        finite = np.arange(B) != row
        top, peak = np.argmax(P[finite], axis=1), P[finite].max(axis=1)

        best, prob = ctx.get_assignments()
        assert best[row] == -1 and np.isnan(prob[row]), (what, best, prob)
        assert np.array_equal(best[finite], top)
        fio.assert_bitwise(prob[finite], peak, f'{what}: get_assignments on the finite rows')
        for t in (-1.0, 0.0, float(np.nextafter(peak.min(), F32(-1))), float(peak.min())):
            above, prob_t, n = ctx.get_assignments_above(t)
            assert above[row] == -1 and np.isnan(prob_t[row]), (what, t)
            assert np.array_equal(above[finite], np.where(peak > F32(t), top, -1)) and n == int((peak > F32(t)).sum()), (what, t)
            fio.assert_bitwise(prob_t[finite], peak, f'{what}: get_assignments_above({t}) on the finite rows')
        for k in (1, 2, 3, 4):
            options, probs = ctx.get_top_options(k)
            assert (options[row] == -1).all() and np.isnan(probs[row]).all(), (what, k)
            want_options, want_probs = stable_top(P[finite], k)
            assert np.array_equal(options[finite], want_options)
            fio.assert_bitwise(probs[finite], want_probs, f'{what}: top {k} on the finite rows')
        donors = ctx.get_donor_readout()
        assert donors['best_singlet'][row] == -1 and np.isnan(donors['best_singlet_prob'][row])
        assert donors['best_pair'][row] == -1 and np.isnan(donors['best_pair_prob'][row])

        names = np.asarray(dev.columns, dtype=object)
        for t in (0.0, 0.5):
            assigned = dev.assignments(t)
            keep = np.flatnonzero(finite)[peak > F32(t)]
            assert list(assigned.index) == [dev.barcodes[b] for b in keep] and dev.barcodes[row] not in assigned.index
            assert list(assigned.values) == list(names[top[peak > F32(t)]])
        frame = dev.best()
        assert frame['option'].iloc[row] is None and np.isnan(frame['probability'].iloc[row])
        assert list(frame['option'][finite]) == list(names[top])
        tops = dev.top_options(4)
        for j in range(4):
            assert tops[f'option_{j + 1}'].iloc[row] is None and np.isnan(tops[f'probability_{j + 1}'].iloc[row])
    finally:
        dev.close()
