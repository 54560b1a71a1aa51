"""The restatement of learning from doublet posteriors (tests/doublet_learning_restatement.py) on the CPU: what the GPU
tests compare with bit for bit is itself pinned here -
  * to tests/pools_learning_restatement.learn, bit for bit on every iteration, when no pair is credited (a threshold above 1 at doublet
    prior 0.35; doublet prior 0);
  * to the contract written out call by call in scalar float32 on the smallest fixtures;
  * to its own by-work-items summation up to float32 rounding ties;
and the measurement of "does it help?" on the seeded simulation with true doublets is taken against the plain loop's error."""
import numpy as np
import pytest

from tests import doublet_learning_restatement as learning
from tests import pooled_helpers as helpers
from tests import pools_learning_restatement as pooled

F1, SMALL = helpers.F1, helpers.F3_SMALL  # f1: G = 20, B = 1000


@pytest.mark.parametrize('dp, threshold', [(0.35, 2.0), (0.35, np.nextafter(np.float32(1), np.float32(2))), (0.0, 1e-3)])
@pytest.mark.parametrize('name', SMALL + ['f2_synthetic_g4.npz', F1])
def test_no_credited_pair_is_the_pooled_loop(name, dp, threshold):
    problem = pooled.fixture_learning_problem(name)
    pools, pool_of = helpers.pools_of(name, problem['B'], problem['betas'].shape[1])
    n = 3
    want = pooled.learn(problem, pools, pool_of, n, 0.01, dp)
    got = learning.learn(problem, pools, pool_of, n, 0.01, dp, threshold=threshold)
    for it in range(n):
        for key in want[it]:
            assert got[it][key].tobytes() == want[it][key].tobytes(), f'{name} dp {dp} threshold {threshold}, iteration {it}: {key}'
        assert not learning.live_pairs(got[it], pools, pool_of, dp != 0, threshold).any()


@pytest.mark.parametrize('name', SMALL + [F1])
def test_a_credited_run_differs_where_pairs_are_live(name):
    problem = pooled.fixture_learning_problem(name)
    pools, pool_of = helpers.pools_of(name, problem['B'], problem['betas'].shape[1])
    plain = pooled.learn(problem, pools, pool_of, 2, 0.01, 0.35)
    credited = learning.learn(problem, pools, pool_of, 2, 0.01, 0.35, threshold=1e-3)
    live = learning.live_pairs(credited[0], pools, pool_of, True, 1e-3)
    assert live.any(), 'the fixture has barcodes with a pair at or above the threshold'
    assert credited[0]['probs'].tobytes() == plain[0]['probs'].tobytes(), 'the first E-step is the same'
    differ = credited[1]['addition'] != plain[1]['addition']
    assert differ.any()
    assert (credited[1]['addition'] >= plain[1]['addition'])[np.isfinite(plain[1]['addition'])].all(), 'a credit only adds'
    # the variants no barcode with a live pair calls keep their sums
    touched = np.zeros(len(problem['betas']), dtype=bool)
    touched[problem['v'][live[problem['cb']] > 0]] = True
    assert not differ[~touched].any()


def scalar_addition(problem, rec, pools, pool_of, with_doublets, power, threshold):
    """The contract, a call and a column at a time, every float32 operation on numpy scalars."""
    f32 = np.float32
    v, cb, e = problem['v'], problem['cb'], problem['e']
    prob, dense, post, row_ptr = rec['prob_table'], rec['dense'], rec['probs'], rec['row_ptr']
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
                        pk = post[row_ptr[b] + k]
                        k += 1
                        if g not in (donors[i], donors[j]) or not pk >= f32(threshold):
                            continue
                        own, other = prob[v[c], g], prob[v[c], donors[j] if donors[i] == g else donors[i]]
                        r = f32(0) if own == 0 else own / (own + other)
                        credit = credit + pk * r
                        assert isinstance(credit, np.float32) and isinstance(r, np.float32)
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
    history = learning.learn(problem, pools, pool_of, 3, 0.01, 0.35, threshold=threshold, power=power)
    for it in (0, 1):
        want = scalar_addition(problem, history[it], pools, pool_of, True, power, threshold)
        assert history[it + 1]['addition'].tobytes() == want.tobytes(), f'{name} power {power} threshold {threshold}: the addition after iteration {it}'


def test_by_items_summation_differs_in_rounding_ties_only():
    problem = pooled.fixture_learning_problem(F1)
    pools, pool_of = helpers.pools_of(F1, problem['B'], problem['betas'].shape[1])
    rec = learning.learn(problem, pools, pool_of, 1, 0.01, 0.35)[0]
    args = (problem['v'], problem['cb'], problem['e'], rec['dense'], rec, pools, pool_of, True, rec['prob_table'])
    in_order = learning.doublet_addition(*args)
    for item_calls in (64, 1024, 1 << 30):
        of_items = learning.doublet_addition_of_items(*args, item_calls=item_calls)
        one_ulp = np.abs(np.nextafter(in_order, np.float32(np.inf)) - in_order)
        assert (np.abs(of_items - in_order) <= one_ulp).all()
        if item_calls == 1 << 30:
            assert of_items.tobytes() == in_order.tobytes(), 'one item per variant is the in-order sum'


@pytest.mark.parametrize('seed', learning.SEEDS)
def test_crediting_pairs_helps_on_the_simulation(seed):
    problem, sim, plain, credited = learning.simulated(seed)
    assert (sim['second'] >= 0).sum() == 96 and (sim['second'] < 0).sum() == 96 and sim['prob'].shape == (1200, 8)
    assert 0.45 < sim['unknown'].mean() < 0.55
    assert np.array_equal(plain[-1]['best_option'], sim['true_option']), 'the yardstick assigns every barcode'
    plain_error = learning.table_error(plain[-1]['prob_table'], sim)
    credited_error = learning.table_error(credited[-1]['prob_table'], sim)
    learning.value_condition(plain_error, credited_error, credited[-1]['best_option'], sim)
    assert credited_error / plain_error <= learning.WORST_MEASURED_RATIO + 5e-4, 'the recorded worst ratio is the measured one'
