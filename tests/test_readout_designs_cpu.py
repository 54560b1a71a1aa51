"""The designed posteriors of tests/readout_designs.py, pushed through the oracle's E-step arithmetic and float32 softmax on the CPU:
the reference alone delivers every edge the GPU tests of the read-outs (tests/test_gpu_readout_shapes.py) rely on - the bit-equal
ties, the exact zeros, the all-NaN row - and ranks the columns each placement is meant to rank first."""
import numpy as np
import pytest

from tests import readout_designs as designs


def posteriors(oracle, design, B):
    return designs.flat_evidence_posteriors(oracle, *design, B)


def stable_top(P, k=4):
    return np.argsort(-P, axis=-1, kind='stable')[..., :k]


def test_the_catalogue_covers_the_widths_and_barcode_counts():
    cases = designs.catalogue()
    assert len(set(cases)) == len(cases)
    assert {K for K, _, _ in cases} == set(designs.WIDTHS)
    for K in designs.WIDTHS:
        assert {B for k, _, B in cases if k == K} == set(designs.BARCODES if K < 8256 else (1, 4, 5)), K
    wide = {name for K, name, _ in cases if K == 321}
    assert wide == set(designs.PLACEMENTS)  # every placement has room at 321 columns
    assert {name for K, name, _ in cases if K == 1} == {'flat'}
    for K in designs.WIDTHS:
        G, with_doublets = designs.shape_for(K)
        assert (G * (G + 1) // 2 if with_doublets else G) == K


def test_the_placements_are_where_the_kernels_edges_are():
    """Columns, lanes (column % 64) and arrival order of the placements, stated outright."""
    for lane in (0, 5, 63):
        for order in ('asc', 'desc'):
            values = designs.placement(f'one_lane_{order}_l{lane}', 321)
            assert sorted(values) == [lane + 64 * j for j in range(5)] and {c % 64 for c in values} == {lane}
            by_arrival = [values[c] for c in sorted(values)]
            assert by_arrival == sorted(by_arrival, reverse=order == 'desc') and len(set(by_arrival)) == 5
    assert designs.placement('one_lane_asc_l63', 319) is not None and len(designs.placement('one_lane_asc_l63', 319)) == 4
    assert list(designs.placement('edges', 321)) == [320, 0, 63] and list(designs.placement('edges', 64)) == [63, 0]
    for name, (a, b) in {'tie_63_64': (63, 64), 'tie_0_64': (0, 64), 'tie_1_64': (1, 64)}.items():
        values = designs.placement(name, 321)
        assert values[a] == values[b] == max(values.values()) and designs.placement(name, 64) is None
    assert (63 % 64, 64 % 64) == (63, 0) and 0 % 64 == 64 % 64 and 1 % 64 > 64 % 64  # other lanes; one lane; lower column, higher lane
    tie3 = designs.placement('tie3_lane2', 131)
    assert tie3[2] == tie3[66] == tie3[130] == max(tie3.values()) and {2 % 64, 66 % 64, 130 % 64} == {2}
    for K in (5, 64, 65, 321):
        values = designs.placement('tie_4th_5th', K)
        ranked = sorted(values.values(), reverse=True)
        assert len(values) == 5 and ranked[3] == ranked[4] and len(set(ranked[:4])) == 4
    assert designs.placement('tie_4th_5th', 4) is None and designs.placement('two_nonzero', 1) is None
    assert designs.placement('two_nonzero', 2) == {1: 0.0, 0: -1.0}


def test_the_issues_own_example(oracle):
    """K = 321: descending values in columns 5, 69, 133, 197, 261, a tie between columns 1 and 64, -200 elsewhere."""
    design = designs.design('tie_1_64_second', 321, 1)
    assert design[:2] == (321, False) and design[3] is None
    row = design[2]
    assert sorted(np.flatnonzero(row != designs.ZERO_LOGIT).tolist()) == [1, 5, 64, 69, 133, 197, 261]
    P = posteriors(oracle, design, 1)
    assert int((P[0] == 0).sum()) == 314 and P[0, 1] == P[0, 64] and P[0, 1] > 0
    assert stable_top(P[0]).tolist() == [5, 1, 64, 69]
    # numpy's own float32 softmax of the penalties, without the E-step's common term
    plain = np.exp(row - row.max())
    plain /= plain.sum()
    assert plain.dtype == np.float32 and int((plain == 0).sum()) == 314 and plain[1] == plain[64]
    assert stable_top(plain).tolist() == [5, 1, 64, 69]


@pytest.mark.parametrize('K,name,B', designs.catalogue())
def test_designs_through_the_oracles_softmax(oracle, K, name, B):
    design = designs.design(name, K, B)
    G, with_doublets, penalties, prior = design
    assert penalties.dtype == np.float32 and penalties.shape == (K,)
    assert (prior is None) == (B == 1) and (prior is None or (prior.dtype == np.float32 and prior.shape == (B, K)))
    L = designs.designed_logits(name, K, B)
    assert L.shape == (B, K) and np.array_equal(L, penalties[None, :] + (0 if prior is None else prior))
    P = posteriors(oracle, design, B)
    designs.structure(P, L, f'{name} K={K} B={B}')
    top = stable_top(P)
    k = min(4, K)
    assert top[0].tolist() == designs.intended_top(name, K)[:k]
    shifts = designs.shifts(K, B)
    assert shifts[0] == 0 and (B == 1 or K == 1 or len(set(shifts.tolist())) > 1)
    for b in range(B):  # a rotated row ranks the rotated columns wherever the rotation keeps the order of the tied and zero columns
        values = designs.placement(name, K)
        moved = {(c + int(shifts[b])) % K: v for c, v in values.items()}
        ranked = sorted(moved, key=lambda c: (-moved[c], c))
        want = (ranked + [c for c in range(K) if c not in moved])[:k]
        assert top[b].tolist() == want, (b, top[b], want)
    if name == 'flat':
        assert (P == P[:, :1]).all() and top[0].tolist() == list(range(k))
    if name == 'two_nonzero':
        assert int((P[0] > 0).sum()) == 2 and (K < 4 or top[0][2:].tolist() == [c for c in range(K) if P[0, c] == 0][:2])
    if name.startswith('one_lane') and K > 256 + int(name.rsplit('l', 1)[1]):
        assert len({int(c) % 64 for c in top[0]}) == 1 and int((P[0] > 0).sum()) == 5  # a lane holds five, the top four are all its own
    if name == 'tie_4th_5th':
        fifth = np.argsort(-P[0], kind='stable')[4]
        assert P[0, top[0][3]] == P[0, fifth] and top[0][3] < fifth


@pytest.mark.parametrize('K', [3, 65, 321, 2080])
def test_a_nan_prior_logit_leaves_a_row_without_posteriors(oracle, K):
    """One NaN in a barcode's prior logits: the oracle's softmax (np.amax and np.sum propagate it) returns that row all NaN and
    leaves the others alone."""
    B, row = 5, 2
    design = designs.nan_design(K, B, row, K // 2)
    prior = design[3]
    assert int(np.isnan(prior).sum()) == 1 and np.isnan(prior[row, K // 2])
    P = posteriors(oracle, design, B)
    assert np.isnan(P[row]).all() and np.isfinite(np.delete(P, row, axis=0)).all()
    designs.structure(P, prior, f'NaN K={K}')
    clean = posteriors(oracle, designs.design('two_nonzero', K, B), B)
    assert np.array_equal(np.delete(P, row, axis=0), np.delete(clean, row, axis=0))


def test_structure_refuses_matrices_without_the_edge():
    L = designs.designed_logits('tie_1_64', 65, 4)
    P = np.exp(L - L.max(axis=1, keepdims=True))
    P /= P.sum(axis=1, keepdims=True)
    designs.structure(P, L)
    for spoil in (lambda Q: Q.__setitem__((0, 1), np.nextafter(Q[0, 1], np.float32(1))),     # the tie broken by one bit
                  lambda Q: Q.__setitem__((1, int(np.flatnonzero(Q[1] == 0)[0])), 1e-45),  # a zero that is not exact
                  lambda Q: Q.__setitem__((2, int(np.argmax(Q[2]))), 0.0),                   # a missing value
                  lambda Q: Q.__setitem__((3, 0), np.nan)):
        Q = P.copy()
        spoil(Q)
        with pytest.raises(AssertionError):
            designs.structure(Q, L)
    nan_row = L.copy()
    nan_row[2, 7] = np.nan
    with pytest.raises(AssertionError):
        designs.structure(P, nan_row)  # a finite row where an all-NaN one is designed
