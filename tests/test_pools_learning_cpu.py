"""The proof of the checker of learning within pools (tests/pools_learning_restatement.py) against the reference's own captured EM runs,
its two zero rules, and the host-side checks of Demultiplexer.learn_genotypes_in_pools: runs without a GPU."""
import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pools_learning_restatement as learning

NAMES = ['f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz', 'f2_synthetic_g4.npz', 'f1_synthetic_default.npz']


@pytest.mark.parametrize('name', NAMES)
def test_restatement_with_one_all_donor_pool_is_the_reference(name):
    fx = fio.load(name)
    problem = learning.fixture_learning_problem(name)
    B, G = problem['B'], problem['betas'].shape[1]
    runs = 0
    for i in range(int(fx['n_em'])):
        if f'em{i}_prior_logits' in fx:
            continue
        n_it, dp, clip = int(fx[f'em{i}_n_iterations']), float(fx[f'em{i}_dp']), float(fx[f'em{i}_clip'])
        history = learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), n_it, clip, dp)
        for it, rec in enumerate(history):
            K = fx[f'em{i}_it{it}_probs'].shape[1]
            fio.assert_bitwise(rec['logits'].reshape(B, K), fx[f'em{i}_it{it}_logits'], f'{name} run {i} it {it}: logits')
            fio.assert_bitwise(rec['probs'].reshape(B, K), fx[f'em{i}_it{it}_probs'], f'{name} run {i} it {it}: probs')
            fio.assert_bitwise(rec['addition'], fx[f'em{i}_it{it}_addition'], f'{name} run {i} it {it}: addition')
            fio.assert_bitwise(rec['dense'], fx[f'em{i}_it{it}_probs'][:, :G], f'{name} run {i} it {it}: the singlet columns')
        fio.assert_bitwise(learning.learnt_betas(problem, history), fx[f'em{i}_learnt_betas'], f'{name} run {i}: learnt betas')
        runs += 1
    assert runs >= 1, 'a run without prior logits'


def test_a_donor_in_no_pool_keeps_a_zero_column_and_a_barcode_in_no_pool_changes_no_sum():
    name = 'f3_small_3.npz'
    problem = learning.fixture_learning_problem(name)
    B, G = problem['B'], problem['betas'].shape[1]
    assert G >= 5 and B >= 8
    pools = [[0, 2], [1, 2, G - 1]]  # donor 3 (and every donor between 3 and G - 2) is in no pool
    pool_of = (np.arange(B) % 3 - 1).astype(np.int32)  # -1, 0, 1, ...
    outside = sorted(set(range(G)) - {0, 1, 2, G - 1})
    history = learning.learn(problem, pools, pool_of, 3, 0.01, 0.35)
    for it, rec in enumerate(history):
        assert not rec['addition'][:, outside].any() and not np.signbit(rec['addition'][:, outside]).any(), f'iteration {it}: +0 columns'
        assert not rec['dense'][pool_of < 0].any() and not rec['dense'][:, outside].any()
    assert history[-1]['addition'][:, [0, 1, 2, G - 1]].any(axis=0).all(), 'the donors of the pools do learn'
    # the same problem with the calls of the barcodes of no pool removed: every sum is the same
    kept = pool_of[problem['cb']] >= 0
    assert 0 < kept.sum() < len(kept)
    without = dict(problem, v=problem['v'][kept], cb=problem['cb'][kept], e=problem['e'][kept])
    for it, (a, b) in enumerate(zip(history, learning.learn(without, pools, pool_of, 3, 0.01, 0.35))):
        for key in ('logits', 'probs', 'dense', 'addition', 'prob_table'):
            fio.assert_bitwise(a[key], b[key], f'iteration {it}: {key}')


def test_learn_genotypes_in_pools_validates_before_it_touches_a_device():
    """resolve_pools's ValueErrors and the n_iterations assertion come first: they raise without a GPU (and without a library call)."""
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    names, barcodes = ['d0', 'd1', 'd2', 'd3'], ['b0', 'b1', 'b2']
    genotypes = ProbabilisticGenotypes(names)
    handler = BarcodeHandler(barcodes)
    everybody = {b: 'A' for b in barcodes}
    with pytest.raises(ValueError, match='unknown donor'):
        Demultiplexer.learn_genotypes_in_pools({}, genotypes, handler, everybody, {'A': ['d0', 'nobody']})
    with pytest.raises(ValueError, match='more than once'):
        Demultiplexer.learn_genotypes_in_pools({}, genotypes, handler, everybody, {'A': ['d0', 'd0']})
    with pytest.raises(ValueError, match='missing from barcode2pool'):
        Demultiplexer.learn_genotypes_in_pools({}, genotypes, handler, {'b0': 'A'}, {'A': ['d0']})
    with pytest.raises(ValueError, match='unknown pool'):
        Demultiplexer.learn_genotypes_in_pools({}, genotypes, handler, dict(everybody, b2='C'), {'A': ['d0']})
    with pytest.raises(AssertionError, match='n_iterations'):
        Demultiplexer.learn_genotypes_in_pools({}, genotypes, handler, everybody, {'A': ['d0', 'd1']}, n_iterations=0)
    staged = Demultiplexer.staged_genotype_learning_in_pools({}, genotypes, handler, everybody, {'A': []})
    with pytest.raises(ValueError, match='no donors'):
        next(staged)
