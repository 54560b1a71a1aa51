"""The proof of the checker of learning the soup's profile (tests/soup_learning_restatement.py): with every fraction 0 the counts are +0
and the loop is the pooled loop bit for bit; with the profile held fixed its additions are the ambient loop's; a droplet that is all
soup counts every call in full; on the seeded simulation with a soup dominated by one donor three updates bring the profile closer to
the truth; and the host-side checks of the Python entries.  Runs without a GPU."""
import functools

import numpy as np
import pytest

from tests import ambient_learning_restatement as learning
from tests import ambient_restatement
from tests import fixture_io as fio
from tests import pools_learning_restatement as pooled
from tests import soup_learning_restatement as soup_learning

NAMES = ['f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz', 'f2_synthetic_g4.npz', 'f1_synthetic_default.npz']


def one_pool(B, G):
    return [list(range(G))], np.zeros(B, np.int32)


@pytest.mark.parametrize('doublet_prior', [0., 0.35])
@pytest.mark.parametrize('name', NAMES)
def test_zero_fractions_count_nothing_and_give_the_pooled_loop_bit_for_bit(name, doublet_prior):
    problem = pooled.fixture_learning_problem(name)
    B, (V, G) = problem['B'], problem['betas'].shape
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    zero = np.zeros(B, dtype=np.float32)
    n_it = 2 if name.startswith('f1') else 3
    pools, pool_of = one_pool(B, G)
    want = pooled.learn(problem, pools, pool_of, n_it, 0.01, doublet_prior)
    got = soup_learning.learn(problem, pools, pool_of, zero, soup, n_it, 0.01, doublet_prior)
    uniform = soup_learning.profile_from_totals(np.zeros(V, np.float32), problem['v2snp'], 1., 0.01)
    for it, (a, b) in enumerate(zip(got, want)):
        for key in ('logits', 'probs', 'dense', 'addition', 'prob_table'):
            fio.assert_bitwise(a[key], b[key], f'{name} it {it}: {key}')
        assert np.array_equal(a['best_option'], b['best_option'])
        assert not a['counts'].any() and not np.signbit(a['counts']).any(), f'{name} it {it}: every total is +0'
        fio.assert_bitwise(a['next_ambient'], uniform, f'{name} it {it}: the pseudo-counts\' uniform share')
    count, _total = soup_learning.soup_counts(problem['v'], problem['cb'], problem['e'], got[-1]['dense'], got[-1]['prob_table'], zero, soup)
    assert not count.any() and not np.signbit(count).any(), 'every count is +0'
    fio.assert_bitwise(soup_learning.learnt_betas(problem, got), pooled.learnt_betas(problem, want), f'{name}: learnt betas')


@pytest.mark.parametrize('name, doublet_prior', [('f3_small_1.npz', 0.), ('f3_small_2.npz', 0.35), ('f2_synthetic_g4.npz', 0.)])
def test_a_fixed_profile_gives_the_ambient_loop_bit_for_bit(name, doublet_prior):
    problem = pooled.fixture_learning_problem(name)
    B, G = problem['B'], problem['betas'].shape[1]
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    alpha = (np.arange(B) % 4 * np.float32(0.25)).astype(np.float32)  # 0 .. 0.75
    pools, pool_of = one_pool(B, G)
    want = learning.learn(problem, pools, pool_of, alpha, soup, 3, 0.01, doublet_prior)
    fixed = soup_learning.learn(problem, pools, pool_of, alpha, soup, 3, 0.01, doublet_prior, fixed=True)
    moving = soup_learning.learn(problem, pools, pool_of, alpha, soup, 3, 0.01, doublet_prior)
    for it, (a, b) in enumerate(zip(fixed, want)):
        for key in ('logits', 'probs', 'dense', 'addition', 'prob_table', 'ambient'):
            fio.assert_bitwise(a[key], b[key], f'{name} it {it}: {key}')
        assert a['counts'].any() and not np.array_equal(a['next_ambient'], soup), 'the update that was ignored is one'
    fio.assert_bitwise(moving[0]['next_ambient'], fixed[0]['next_ambient'], 'the first update reads the same E-step')
    fio.assert_bitwise(moving[1]['ambient'], moving[0]['next_ambient'], 'the update takes effect in the next iteration')
    fio.assert_bitwise(moving[1]['addition'], fixed[1]['addition'], 'the genotype M-step reads the profile its E-step read')
    assert not np.array_equal(moving[2]['addition'], fixed[2]['addition']), 'a learnt profile changes what the genotypes learn'


def test_a_droplet_that_is_all_soup_counts_every_call_in_full():
    """alpha == 1 and ambient != 0: own == 0, s == 1, t == dense keep.  With one-hot posteriors count[v, g] is the float32 of the
    float64 sum of keep over the calls of the barcodes whose donor is g; total[v] is the sum of those float32 values, so it is
    f32(sum over all calls of f64(keep)) bit for bit where the calls of a variant share one column (the contract rounds every column
    once: with several columns the identity holds up to those roundings, one half ulp of a column each)."""
    problem = pooled.fixture_learning_problem('f3_small_1.npz')
    B, (V, G) = problem['B'], problem['betas'].shape
    v, cb, e = problem['v'], problem['cb'], problem['e']
    rng = np.random.default_rng(5)
    hot = rng.integers(0, G, size=B)
    prob = rng.uniform(0.01, 0.99, size=(V, G)).astype(np.float32)
    soup = rng.uniform(0.01, 1.0, size=V).astype(np.float32)  # no zeros
    keep = 1 - e
    assert keep.dtype == np.float32
    in_all = np.bincount(v, weights=keep, minlength=V)  # float64, in call order
    for column in (0, G - 1):
        dense = np.zeros((B, G), dtype=np.float32)
        dense[:, column] = 1.0  # one-hot, everybody the same donor
        count, total = soup_learning.soup_counts(v, cb, e, dense, prob, np.ones(B, np.float32), soup)
        fio.assert_bitwise(total, in_all.astype(np.float32), 'total[v] == f32(sum of f64(keep))')
        fio.assert_bitwise(count[:, column], total, 'the one column holds everything')
        assert total.any() and not np.delete(count, column, axis=1).any()
    dense = np.zeros((B, G), dtype=np.float32)
    dense[np.arange(B), hot] = 1.0  # one-hot, every barcode its own donor
    count, total = soup_learning.soup_counts(v, cb, e, dense, prob, np.ones(B, np.float32), soup)
    for g in range(G):
        mine = hot[cb] == g
        fio.assert_bitwise(count[:, g], np.bincount(v[mine], weights=keep[mine], minlength=V).astype(np.float32), f'column {g}')
    fio.assert_bitwise(total, soup_learning.totals(count), 'the columns added in ascending order')
    assert (np.abs(total.astype(np.float64) - in_all) <= (G + 1) * 0.5 * np.spacing(in_all.astype(np.float32))).all()
    # a tiny posterior is live: nothing is dropped below 2^-80
    tiny = dense.copy()
    tiny[tiny == 0] = np.float32(2.0 ** -100)
    count_tiny, _ = soup_learning.soup_counts(v, cb, e, tiny, prob, np.ones(B, np.float32), soup)
    assert (count_tiny[(count == 0) & (np.bincount(v, minlength=V) > 0)[:, None]] > 0).all()
    # the split into items is the same sum up to a float32 rounding boundary
    alpha = (np.arange(B) % 3 * np.float32(0.2)).astype(np.float32)
    args = (v, cb, e, tiny, prob, alpha, soup)
    seq, seq_total = soup_learning.soup_counts(*args)
    whole, whole_total = soup_learning.soup_counts_of_items(*args, item_calls=1 << 30)
    fio.assert_bitwise(whole, seq, 'one item per variant')
    fio.assert_bitwise(whole_total, seq_total, 'one item per variant: totals')
    cut, _ = soup_learning.soup_counts_of_items(*args, item_calls=3)
    assert (np.abs(cut - seq) <= np.spacing(np.maximum(np.abs(seq), np.float32(1e-30)))).all()


@functools.lru_cache(maxsize=None)
def recovery(seed):
    sim, derived, history = soup_learning.recovery_run(seed)
    return sim, soup_learning.profile_error(derived, sim), [soup_learning.profile_error(rec['next_ambient'], sim) for rec in history]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_three_updates_bring_the_profile_closer_to_the_soup(seed):
    """A soup weighted 8 : 1 : ... : 1 over 8 donors, 600 SNPs, 384 barcodes of 256 calls, the true table and the true fractions:
    the restatement measures 0.126 -> 0.078, 0.120 -> 0.078, 0.127 -> 0.079, ratios 0.620, 0.645 and 0.619 (seeds 0, 1, 2)."""
    sim, derived_error, errors = recovery(seed)
    assert len(errors) == 3 and np.unique(sim['soup']).size > 3
    soup_learning.recovery_condition(derived_error, errors[-1], f'seed {seed}: after updates {[round(x, 5) for x in errors]}: ')


def test_the_python_entries_validate_before_they_touch_a_device():
    """The argument errors come first: they raise without a GPU (and without a library call)."""
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    names, barcodes = ['d0', 'd1', 'd2', 'd3'], ['b0', 'b1', 'b2']
    genotypes = ProbabilisticGenotypes(names)
    handler = BarcodeHandler(barcodes)
    fractions = {'b0': 0.2}
    for entry in (Demultiplexer.learn_ambient_profile, Demultiplexer.learn_genotypes_and_ambient):
        with pytest.raises(AssertionError, match='n_iterations'):
            entry({}, genotypes, handler, fractions, n_iterations=0)
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(AssertionError, match='pseudo_count'):
                entry({}, genotypes, handler, fractions, pseudo_count=bad)
        with pytest.raises(ValueError, match='not one of the barcode handler'):
            entry({}, genotypes, handler, {'nobody': 0.1})
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            entry({}, genotypes, handler, {'b0': 1.5})
        with pytest.raises(AssertionError, match='come together'):
            entry({}, genotypes, handler, fractions, barcode2pool={b: 'A' for b in barcodes})
    staged = Demultiplexer.staged_genotype_learning_and_ambient({}, genotypes, handler, {'b0': 1.5})
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        next(staged)
    with pytest.raises(AssertionError, match='pseudo_count'):
        next(Demultiplexer.staged_genotype_learning_and_ambient({}, genotypes, handler, fractions, pseudo_count=0.0))
    with pytest.raises(AssertionError, match='n_iterations'):
        next(Demultiplexer.staged_genotype_learning_and_ambient({}, genotypes, handler, fractions, n_iterations=0))
