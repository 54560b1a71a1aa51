"""The restatement of learning from doublets of unequal shares (tests/doublet_shares_learning_restatement.py) on the CPU:
what the GPU tests compare with bit for bit is itself pinned here -
  * D1: at the grid {0.5} with the weight {0} to tests/doublet_learning_restatement.learn, bit for bit on every iteration;
  * D2: at that grid with a threshold above 1, and at any grid at doublet prior 0, to tests/pools_learning_restatement.learn;
  * D3: at the grid {1} a live pair credits its first donor its whole posterior where the table entry is above 0 and its second donor
    nothing; {0} is the mirror image;
  * to the contract written out call by call in scalar float32 on the smallest fixtures;
and the measurement of "does it help?" on the seeded simulation with doublets of share 0.8 and 0.5 is taken against the even loop's
error on the same problem."""
import numpy as np
import pytest

from tests import doublet_learning_restatement as even
from tests import doublet_shares_learning_restatement as learning
from tests import pooled_helpers as helpers
from tests import pools_learning_restatement as pooled

F1, F2, SMALL = helpers.F1, helpers.F2, helpers.F3_SMALL  # f1: G = 20, B = 1000
HALF, ZERO = np.array([0.5], np.float32), np.array([0.0], np.float32)
GRID = np.array([0.7, 0.1, 0.5, 1.0, 0.1, 0.0, 0.35], np.float32)  # unsorted, a duplicate, both ends


def assert_records(got, want, what):
    for it, (g, w) in enumerate(zip(got, want)):
        for key in w:
            assert g[key].tobytes() == w[key].tobytes(), f'{what}, iteration {it}: {key}'


@pytest.mark.parametrize('dp', [0.35, 0.0])
@pytest.mark.parametrize('name', SMALL + [F2, F1])
def test_d1_the_even_grid_is_the_even_loop(name, dp):
    problem = pooled.fixture_learning_problem(name)
    pools, pool_of = helpers.pools_of(name, problem['B'], problem['betas'].shape[1])
    n = 3
    want = even.learn(problem, pools, pool_of, n, 0.01, dp)
    for log_weights in (ZERO, None):
        got = learning.learn(problem, pools, pool_of, n, 0.01, dp, HALF, log_weights)
        assert_records(got, want, f'{name} dp {dp}')
        for rec in got:
            pair = ~rec['single']
            assert (rec['share_mean'][pair] == np.float32(0.5)).all() and np.isnan(rec['share_mean'][~pair]).all()
    if dp:
        assert even.live_pairs(want[1], pools, pool_of, True, 1e-3).any(), 'the fixture has live pairs: the credit is exercised'


@pytest.mark.parametrize('dp, threshold, shares', [(0.35, 2.0, HALF), (0.35, np.nextafter(np.float32(1), np.float32(2)), HALF), (0.0, 1e-3, HALF),
                                                   (0.0, 1e-3, GRID)])
@pytest.mark.parametrize('name', SMALL + [F2, F1])
def test_d2_no_credited_pair_is_the_pooled_loop(name, dp, threshold, shares):
    problem = pooled.fixture_learning_problem(name)
    pools, pool_of = helpers.pools_of(name, problem['B'], problem['betas'].shape[1])
    n = 3
    want = pooled.learn(problem, pools, pool_of, n, 0.01, dp)
    got = learning.learn(problem, pools, pool_of, n, 0.01, dp, shares, threshold=threshold)
    assert_records(got, want, f'{name} dp {dp} threshold {threshold}')
    if dp == 0:
        assert all((rec['share_index'] == -1).all() and np.isnan(rec['share_mean']).all() for rec in got)


@pytest.mark.parametrize('end', [1.0, 0.0])
@pytest.mark.parametrize('name', SMALL + [F2])
def test_d3_a_grid_of_one_end_credits_one_donor(name, end):
    problem = pooled.fixture_learning_problem(name)
    pools, pool_of = helpers.pools_of(name, problem['B'], problem['betas'].shape[1])
    donors, threshold = pools[0], 1e-3
    n = len(donors)
    history = learning.learn(problem, pools, pool_of, 2, 0.01, 0.35, np.array([end], np.float32), threshold=threshold)
    rec = history[0]
    pair = ~rec['single']
    assert (rec['share_mean'][pair] == np.float32(end)).all()
    v, cb, e = problem['v'], problem['cb'], problem['e']
    prob, V = rec['prob_table'], len(problem['betas'])
    want = np.zeros_like(problem['betas'])
    credited = False
    for at, g in enumerate(donors):
        d = rec['dense'][cb, g]
        credit = np.where(d <= learning.live_floor(2.), np.float32(0), d).astype(np.float32)
        for other in range(n):
            if other == at:
                continue
            whole = (at < other) == (end == 1.0)  # g holds the whole droplet: the first donor at share 1, the second at share 0
            if not whole:
                continue
            post = rec['probs'][rec['row_ptr'][cb] + learning.pair_index(n, min(at, other), max(at, other))]
            take = (post >= np.float32(threshold)) & (prob[v, g] > 0)
            credited = credited or take.any()
            credit = np.where(take, credit + post, credit)
        w = credit * (1 - e)
        want[:, g] = np.bincount(v, weights=w * w, minlength=V)
    assert credited and want.dtype == np.float32
    assert history[1]['addition'].tobytes() == want.tobytes(), f'{name}: shares {{{end}}}'


def scalar_addition(problem, rec, pools, pool_of, with_doublets, power, threshold):
    """The contract, a call and a column at a time, every float32 operation on numpy scalars."""
    f32 = np.float32
    v, cb, e = problem['v'], problem['cb'], problem['e']
    prob, dense, post, mean, row_ptr = rec['prob_table'], rec['dense'], rec['probs'], rec['share_mean'], rec['row_ptr']
    V, G = prob.shape
    floor = learning.live_floor(power)
    sums = np.zeros((V, G), dtype=np.float64)
    for c in range(len(v)):
        b, p = int(cb[c]), int(pool_of[cb[c]])
        keep = f32(1) - f32(e[c])
        for g in range(G):
            credit = dense[b, g] if dense[b, g] > floor else f32(0)
            if p >= 0 and with_doublets:
                donors, k = pools[p], len(pools[p])
                for i in range(len(donors)):
                    for j in range(i + 1, len(donors)):
                        pk, w = post[row_ptr[b] + k], mean[row_ptr[b] + k]
                        k += 1
                        if g not in (donors[i], donors[j]) or not pk >= f32(threshold):
                            continue
                        assert f32(0) <= w <= f32(1)
                        first = donors[i] == g
                        w_own, w_other = (w, f32(1) - w) if first else (f32(1) - w, w)
                        a = prob[v[c], g] * w_own
                        o = prob[v[c], donors[j] if first else donors[i]] * w_other
                        r = f32(0) if a == 0 else a / (a + o)
                        credit = credit + pk * r
                        assert all(isinstance(x, np.float32) for x in (w_own, w_other, a, o, r, credit))
            base = credit * keep
            w = base * base if power == 2 else f32(np.float64(base) ** np.float64(power))
            sums[v[c], g] += np.float64(w)
    return sums.astype(np.float32)


@pytest.mark.parametrize('power, threshold', [(2., 1e-3), (2., 1e-6), (1.5, 1e-3), (2., 0.25)])
@pytest.mark.parametrize('name', SMALL)
def test_the_contract_call_by_call(name, power, threshold):
    problem = pooled.fixture_learning_problem(name)
    B, G = problem['B'], problem['betas'].shape[1]
    pools = [list(range(G))] if G < 4 else [list(range(G - 1)), list(range(1, G)), [0, G - 1]]
    pool_of = np.zeros(B, np.int32) if G < 4 else ((np.arange(B) % 4) - 1).astype(np.int32)
    weights = np.linspace(-1.5, 0.5, len(GRID)).astype(np.float32)
    history = learning.learn(problem, pools, pool_of, 3, 0.01, 0.35, GRID, weights, threshold=threshold, power=power)
    assert learning.live_pairs(history[0], pools, pool_of, True, threshold).any()
    means = history[0]['share_mean'][~history[0]['single']]
    assert len(np.unique(means)) > 3, 'pairs of several posterior mean shares'
    for it in (0, 1):
        want = scalar_addition(problem, history[it], pools, pool_of, True, power, threshold)
        assert history[it + 1]['addition'].tobytes() == want.tobytes(), f'{name} power {power} threshold {threshold}: the addition after iteration {it}'


def test_by_items_summation_differs_in_rounding_ties_only():
    problem = pooled.fixture_learning_problem(F1)
    pools, pool_of = helpers.pools_of(F1, problem['B'], problem['betas'].shape[1])
    rec = learning.learn(problem, pools, pool_of, 1, 0.01, 0.35, GRID)[0]
    args = (problem['v'], problem['cb'], problem['e'], rec['dense'], rec, pools, pool_of, True, rec['prob_table'])
    in_order = learning.share_addition(*args)
    for item_calls in (64, 1 << 30):
        of_items = learning.share_addition_of_items(*args, item_calls=item_calls)
        one_ulp = np.abs(np.nextafter(in_order, np.float32(np.inf)) - in_order)
        assert (np.abs(of_items - in_order) <= one_ulp).all()
        if item_calls == 1 << 30:
            assert of_items.tobytes() == in_order.tobytes(), 'one item per variant is the in-order sum'


@pytest.mark.parametrize('share', [0.8, 0.5])
@pytest.mark.parametrize('seed', learning.SEEDS)
def test_learning_under_shares_on_the_simulation(seed, share):
    problem, sim, yardstick, history = learning.simulated(share, seed)
    assert (sim['second'] >= 0).sum() == 96 and (sim['second'] < 0).sum() == 96 and sim['prob'].shape == (1200, 8)
    assert 0.45 < sim['unknown'].mean() < 0.55
    yardstick_error = learning.table_error(yardstick[-1]['prob_table'], sim)
    error = learning.table_error(history[-1]['prob_table'], sim)
    learning.value_condition(share, yardstick_error, error, yardstick[-1]['best_option'], history[-1]['best_option'], sim)
    if share == 0.8:
        assert error / yardstick_error <= learning.WORST_MEASURED_RATIO + 5e-4, 'the recorded worst ratio is the measured one'
