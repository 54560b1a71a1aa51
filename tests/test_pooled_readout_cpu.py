"""The restatement of the pooled read-outs (tests/pooled_readout_restatement.py) against what it must agree with, without a GPU:
inside one pool it is the dense donor-level restatement (tests/donor_readout_restatement.py) on that pool's frame, its masses are
within the dense contract's bound of numpy's sums, and its slab rule is the plain loop of dmx_get_option_sums."""
import numpy as np
import pytest

from tests import donor_readout_restatement as dense
from tests import pooled_readout_restatement as pooled


def softmax_rows(rng, pool_sizes, pool_of, with_doublets):
    row_ptr = pooled.row_pointer(pool_sizes, pool_of, with_doublets)
    probs = np.zeros(int(row_ptr[-1]), dtype=np.float32)
    for b in range(len(pool_of)):
        n = int(row_ptr[b + 1] - row_ptr[b])
        if n:
            x = rng.normal(size=n).astype(np.float32) * np.float32(3)
            e = np.exp(x - x.max())
            probs[row_ptr[b]:row_ptr[b + 1]] = e / e.sum()
    return row_ptr, probs


def designed():
    """Random rows plus designed ones: ties across singlets and inside the pair block, exact zeros, a singlet-heavy and a pair-heavy row."""
    rng = np.random.default_rng(11)
    pool_sizes = [3, 1, 7, 12]
    pool_of = np.array([0, 3, -1, 1, 2, 0, 3, 2, -1, 0, 1, 3, 2, 2], dtype=np.int32)
    out = {}
    for with_doublets in (True, False):
        row_ptr, probs = softmax_rows(rng, pool_sizes, pool_of, with_doublets)

        def row(b):
            return probs[row_ptr[b]:row_ptr[b + 1]]
        row(0)[:] = 0
        row(0)[[1, 2]] = 0.5  # a tie of two singlets, zeros elsewhere
        if with_doublets:
            row(4)[:] = 0
            row(4)[[9, 20]] = np.float32(0.375)  # a tie inside the pair block
            row(4)[2] = np.float32(0.25)
            row(6)[:] = np.float32(1.0 / len(row(6)))  # everything ties
        out[with_doublets] = (pool_sizes, pool_of, row_ptr, probs)
    return out


DESIGNED = designed()


@pytest.mark.parametrize('with_doublets', [True, False])
def test_one_pool_is_the_dense_readout_on_its_frame(with_doublets):
    pool_sizes, pool_of, row_ptr, probs = DESIGNED[with_doublets]
    r = pooled.readout(probs, row_ptr, pool_of, pool_sizes, with_doublets)
    assert np.array_equal(np.diff(r['marg_ptr']), [pool_sizes[p] if p >= 0 else 0 for p in pool_of])
    for p, g in enumerate(pool_sizes):
        rows = pooled.rows_of(pool_of, p)
        frame = pooled.pool_frame(probs, row_ptr, pool_of, p)
        want = dense.readout(frame, g)
        for key in ('best_singlet', 'best_singlet_prob', 'best_pair', 'best_pair_prob'):
            assert r[key][rows].tobytes() == want[key].tobytes(), (p, key)
        assert np.array_equal(r['best_option'][rows], frame.argmax(axis=1))
        assert r['best_prob'][rows].tobytes() == frame.max(axis=1).tobytes()
        marginals = np.stack([r['donor_marginals'][r['marg_ptr'][b]:r['marg_ptr'][b + 1]] for b in rows])
        assert marginals.tobytes() == want['donor_marginals'].tobytes(), p
        # the masses are sequential sums: within the dense contract's bound of numpy's pairwise ones
        K = frame.shape[1]
        for key in ('singlet_mass', 'doublet_mass'):
            assert np.all(np.abs(r[key][rows] - want[key]) <= (K - 1) * 2.0 ** -53 * np.abs(want[key])), (p, key)
        if not with_doublets:
            assert not r['doublet_mass'][rows].any() and (r['best_pair'][rows] == -1).all()
    none = pool_of < 0
    assert np.isnan(r['singlet_mass'][none]).all() and np.isnan(r['doublet_mass'][none]).all()
    assert (r['best_option'][none] == -1).all() and np.isnan(r['best_prob'][none]).all()


@pytest.mark.parametrize('with_doublets', [True, False])
def test_allowed_mass_of_one_pool_is_the_dense_one(with_doublets):
    pool_sizes, pool_of, row_ptr, probs = DESIGNED[with_doublets]
    rng = np.random.default_rng(5)
    start, options = [0], []
    for b, p in enumerate(pool_of):
        K = int(row_ptr[b + 1] - row_ptr[b])
        if p >= 0 and b % 5 != 4:  # (every fifth list is empty)
            options.extend(rng.integers(0, K, size=int(rng.integers(1, 6))))  # duplicates happen
        start.append(len(options))
    start, options = np.asarray(start, np.int64), np.asarray(options, np.int32)
    mass, hit = pooled.allowed_mass(probs, row_ptr, pool_of, start, options)
    for p in range(len(pool_sizes)):
        rows = pooled.rows_of(pool_of, p)
        frame = pooled.pool_frame(probs, row_ptr, pool_of, p)
        local_start = np.concatenate([[0], np.cumsum([start[b + 1] - start[b] for b in rows])])
        local_options = np.concatenate([options[start[b]:start[b + 1]] for b in rows] + [np.zeros(0, np.int32)])
        want_mass, want_hit = dense.allowed_mass(frame, local_start, local_options)
        assert mass[rows].tobytes() == want_mass.tobytes() and np.array_equal(hit[rows], want_hit), p
    assert np.isnan(mass[pool_of < 0]).all() and not hit[pool_of < 0].any()


@pytest.mark.parametrize('with_doublets', [True, False])
@pytest.mark.parametrize('threshold', [0.9, 0.3])
def test_calls_and_summary_per_pool_are_the_dense_ones(with_doublets, threshold):
    pool_sizes, pool_of, row_ptr, probs = DESIGNED[with_doublets]
    names = [f'pool{p}' for p in range(len(pool_sizes))]
    donors = [[f'p{p}d{i}' for i in range(g)] for p, g in enumerate(pool_sizes)]
    r = pooled.readout(probs, row_ptr, pool_of, pool_sizes, with_doublets)
    frame = pooled.calls(r, pool_of, names, donors, with_doublets, threshold)
    sums, counts = pooled.option_sums(probs, row_ptr, pool_of, pool_sizes, with_doublets)
    got_summary = pooled.summary(frame, sums, names, donors, with_doublets)
    first = 0
    for p, g in enumerate(pool_sizes):
        rows = pooled.rows_of(pool_of, p)
        dense_frame = pooled.pool_frame(probs, row_ptr, pool_of, p)
        assert counts[p] == len(rows)
        want = dense.calls(dense_frame, donors[p], threshold)
        got = frame.iloc[rows].drop(columns='pool').reset_index(drop=True)
        # (the masses of the dense restatement are numpy's pairwise sums: the statuses agree wherever no mass sits within an ulp of
        # the threshold, which no designed row does; probabilities are compared within the sums' bound)
        assert list(got['status']) == list(want['status']) and list(got['donor_1']) == list(want['donor_1']) and list(got['donor_2']) == list(want['donor_2'])
        K = dense_frame.shape[1]
        for column in ('probability', 'doublet_probability'):
            assert np.allclose(got[column].values.astype(float), want[column].values.astype(float), rtol=(K - 1) * 2.0 ** -53, atol=0)
        want_summary = dense.summary(dense_frame, donors[p], threshold)
        mine = got_summary.loc[names[p]]
        assert list(mine.index) == donors[p]
        assert np.array_equal(mine['n_singlets'].values, want_summary['n_singlets'].values)
        assert np.array_equal(mine['n_doublets'].values, want_summary['n_doublets'].values)
        # expected cells: slab sums against numpy's column sums, n_p (K - 1) terms at most per donor
        bound = (len(rows) * K) * 2.0 ** -53
        assert np.allclose(mine['expected_cells'].values, want_summary['expected_cells'].values.astype(float), rtol=bound, atol=0)
        first += K
    assert first == len(sums)
    none = frame[pool_of < 0]
    assert (none['status'] == 'unassigned').all() and none['pool'].isna().all() and none['probability'].isna().all()


@pytest.mark.parametrize('n', [0, 1, 511, 512, 513, 1300])
def test_slab_rule_is_the_plain_loop(n):
    """dmx_get_option_sums' order on a list of n values (results.hip: k_option_partial / k_option_final), restated as the two
    plain loops."""
    rng = np.random.default_rng(n)
    values = rng.random(n).astype(np.float32)
    per = (n + 511) // 512
    partial = []
    for j in range(512):
        lo = j * per
        hi = min(lo + per, n)
        s = np.float64(0)
        for i in range(lo, hi):
            s += np.float64(values[i])
        partial.append(s)
    total = np.float64(0)
    for s in partial:
        total += s
    assert pooled.slab_sum(values).tobytes() == total.tobytes()
    # one value per slab up to 512: the sequential sum; beyond, slabs of 2 and 3
    if n <= 512:
        assert pooled.slab_sum(values).tobytes() == pooled.sequential(values).tobytes()
    assert per == {0: 0, 1: 1, 511: 1, 512: 1, 513: 2, 1300: 3}[n]


def test_top_options_and_nan_rows():
    row_ptr = np.array([0, 3, 3, 8, 9], dtype=np.int64)
    nan = np.float32(np.nan)
    probs = np.array([0.25, 0.5, 0.25, nan, 0.5, 0.5, nan, 0.0, nan], dtype=np.float32)
    options, values = pooled.top_options(probs, row_ptr, 4)
    assert options.tolist() == [[1, 0, 2, -1], [-1] * 4, [1, 2, 4, -1], [-1] * 4]
    assert values[0].tolist()[:3] == [0.5, 0.25, 0.25] and np.isnan(values[0, 3]) and np.isnan(values[3]).all()
    r = pooled.readout(probs, row_ptr, np.array([0, -1, 1, 2], np.int32), [3, 5, 1], False)
    assert r['best_option'].tolist() == [1, -1, 1, -1] and np.isnan(r['best_prob'][3])
