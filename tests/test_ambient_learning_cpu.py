"""The proof of the checker of learning under ambient fractions (tests/ambient_learning_restatement.py): at fraction 0 it is the
pooled loop bit for bit, on the seeded simulation the weighted M-step brings the table closer to the truth, a droplet that is all soup
teaches nothing; and the host-side checks of Demultiplexer.learn_genotypes_with_ambient.  Runs without a GPU."""
import functools

import numpy as np
import pytest

from tests import ambient_learning_restatement as learning
from tests import ambient_restatement
from tests import fixture_io as fio
from tests import pools_learning_restatement as pooled

NAMES = ['f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz', 'f2_synthetic_g4.npz', 'f1_synthetic_default.npz']


def overlapping_pools(B, G):
    """Two or three pools that share donors; every fifth barcode in no pool."""
    half = max(G // 2, 1)
    pools = [list(range(0, min(half + 1, G))), list(range(max(half - 1, 0), G))]
    if G >= 3:
        pools.append([0, G - 1])
    pool_of = (np.arange(B) % len(pools)).astype(np.int32)
    pool_of[::5] = -1
    return pools, pool_of


@pytest.mark.parametrize('doublet_prior', [0., 0.35])
@pytest.mark.parametrize('name', NAMES)
def test_zero_fractions_give_the_pooled_loop_bit_for_bit(name, doublet_prior):
    problem = pooled.fixture_learning_problem(name)
    B, G = problem['B'], problem['betas'].shape[1]
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    zero = np.zeros(B, dtype=np.float32)
    n_it = 2 if name.startswith('f1') else 3
    for what, (pools, pool_of) in (('one pool', ([list(range(G))], np.zeros(B, np.int32))), ('overlapping', overlapping_pools(B, G))):
        want = pooled.learn(problem, pools, pool_of, n_it, 0.01, doublet_prior)
        got = learning.learn(problem, pools, pool_of, zero, soup, n_it, 0.01, doublet_prior)
        for it, (a, b) in enumerate(zip(got, want)):
            for key in ('logits', 'probs', 'dense', 'addition', 'prob_table'):
                fio.assert_bitwise(a[key], b[key], f'{name} {what} it {it}: {key}')
            assert np.array_equal(a['best_option'], b['best_option'])
        fio.assert_bitwise(learning.learnt_betas(problem, got), pooled.learnt_betas(problem, want), f'{name} {what}: learnt betas')


@functools.lru_cache(maxsize=None)
def value_run(seed):
    """(sim, plain loop's error, E-step-only error, weighted error, the weighted loop's history): computed once per seed."""
    problem, sim = learning.simulated_problem(seed)
    B, G = sim['B'], sim['prob'].shape[1]
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    alpha = sim['truth'].astype(np.float32)
    plain = pooled.learn(problem, pools, pool_of, 5, 0.01, 0.)
    estep_only = learning.learn(problem, pools, pool_of, alpha, sim['soup'], 5, 0.01, 0., weighted=False)
    weighted = learning.learn(problem, pools, pool_of, alpha, sim['soup'], 5, 0.01, 0.)
    for history in (plain, estep_only):
        assert np.array_equal(history[-1]['best_option'], sim['donor1'])
    return sim, learning.table_error(plain, sim), learning.table_error(estep_only, sim), learning.table_error(weighted, sim), weighted


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_weighted_m_step_brings_the_table_closer_to_the_truth(seed):
    sim, plain, estep_only, weighted, history = value_run(seed)
    print(f'seed {seed}: plain {plain:.5f}, ambient E-step with the plain M-step {estep_only:.5f}, weighted {weighted:.5f}')
    learning.value_condition(plain, weighted, history[-1]['best_option'], sim)


def test_a_droplet_that_is_all_soup_teaches_nothing_and_leaves_finite_sums():
    problem = pooled.fixture_learning_problem('f3_small_1.npz')
    B, (V, G) = problem['B'], problem['betas'].shape
    v, cb, e = problem['v'], problem['cb'], problem['e']
    alpha = np.ones(B, dtype=np.float32)
    alpha[1::2] = 0.25
    soup = np.zeros(V, dtype=np.float32)  # alpha == 1 and ambient == 0: mix == 0, 0 / 0 without the own == 0 branch
    history = learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), alpha, soup, 3, 0.01, 0.)
    for it, rec in enumerate(history):
        assert np.isfinite(rec['addition']).all(), f'iteration {it}'
    # the calls of the barcodes at alpha == 1 removed: every M-step sum is the same
    dense, prob = history[1]['dense'], history[1]['prob_table']
    kept = alpha[cb] != 1
    assert 0 < kept.sum() < len(kept)
    full = learning.ambient_addition(v, cb, e, dense, prob, alpha, soup)
    part = np.zeros_like(full)
    part[:] = learning.ambient_addition(v[kept], cb[kept], e[kept], dense, prob, alpha, soup)
    fio.assert_bitwise(full, part, 'alpha == 1 contributes +0')
    fio.assert_bitwise(full, history[2]['addition'], 'the loop used that addition')
    assert full.any()


def test_the_sum_of_item_partials_is_the_sequential_sum_up_to_a_rounding_tie():
    problem = pooled.fixture_learning_problem('f3_small_2.npz')
    B, (V, G) = problem['B'], problem['betas'].shape
    alpha = (np.arange(B) % 3 * np.float32(0.2)).astype(np.float32)
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    rec = learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), alpha, soup, 1, 0.01, 0.)[0]
    args = (problem['v'], problem['cb'], problem['e'], rec['dense'], rec['prob_table'], alpha, soup)
    seq = learning.ambient_addition(*args)
    fio.assert_bitwise(learning.ambient_addition_of_items(*args, item_calls=1 << 30), seq, 'one item per variant')
    cut = learning.ambient_addition_of_items(*args, item_calls=3)
    ulp = np.spacing(np.maximum(np.abs(seq), np.float32(1e-30)))
    assert (np.abs(cut - seq) <= ulp).all()


def test_another_power_is_the_float64_power_rounded_once():
    """Power 2 is numpy's own float32 square; another power is within one float32 ulp of whatever numpy's float32 `**` is on this host
    (libm's powf or a vector library's: not a reference of bits) and equals the float64 power rounded to float32."""
    problem = pooled.fixture_learning_problem('f3_small_1.npz')
    B, G = problem['B'], problem['betas'].shape[1]
    alpha = (np.arange(B) % 3 * np.float32(0.2)).astype(np.float32)
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    rec = learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), alpha, soup, 1, 0.01, 0.)[0]
    args = (problem['v'], problem['cb'], problem['e'], rec['dense'], rec['prob_table'], alpha, soup)
    for g in range(G):
        base = learning.weights(*args, g, 1.0)
        assert base.dtype == np.float32 and (base >= 0).all()
        square = base.copy()
        square **= 2.
        fio.assert_bitwise(learning.weights(*args, g, 2.), square, 'power 2')
        got = learning.weights(*args, g, 1.5)
        fio.assert_bitwise(got, (base.astype(np.float64) ** 1.5).astype(np.float32), 'power 1.5')
        host = base.copy()
        host **= 1.5
        assert (np.abs(got - host) <= np.spacing(np.maximum(got, host))).all()


def test_learn_genotypes_with_ambient_validates_before_it_touches_a_device():
    """The argument errors come first: they raise without a GPU (and without a library call)."""
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    names, barcodes = ['d0', 'd1', 'd2', 'd3'], ['b0', 'b1', 'b2']
    genotypes = ProbabilisticGenotypes(names)
    handler = BarcodeHandler(barcodes)
    everybody = {b: 'A' for b in barcodes}
    fractions = {'b0': 0.2}
    with pytest.raises(AssertionError, match='n_iterations'):
        Demultiplexer.learn_genotypes_with_ambient({}, genotypes, handler, fractions, n_iterations=0)
    with pytest.raises(ValueError, match='not one of the barcode handler'):
        Demultiplexer.learn_genotypes_with_ambient({}, genotypes, handler, {'nobody': 0.1})
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        Demultiplexer.learn_genotypes_with_ambient({}, genotypes, handler, {'b0': 1.5})
    with pytest.raises(AssertionError, match='come together'):
        Demultiplexer.learn_genotypes_with_ambient({}, genotypes, handler, fractions, barcode2pool=everybody)
    with pytest.raises(ValueError, match='unknown donor'):
        Demultiplexer.learn_genotypes_with_ambient({}, genotypes, handler, fractions, barcode2pool=everybody, pool2donors={'A': ['d0', 'nobody']})
    with pytest.raises(ValueError, match='missing from barcode2pool'):
        Demultiplexer.learn_genotypes_with_ambient({}, genotypes, handler, fractions, barcode2pool={'b0': 'A'}, pool2donors={'A': ['d0']})
    staged = Demultiplexer.staged_genotype_learning_with_ambient({}, genotypes, handler, {'b0': 1.5})
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        next(staged)
