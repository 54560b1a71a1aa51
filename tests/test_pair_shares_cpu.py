"""Doublets over a grid of mixing shares, without a GPU (Demultiplexer.predict_posteriors_with_doublet_shares;
include/demux_hip_debug.h: dmx_estep_pair_shares).

1. The checker of the GPU tests, tests/pair_shares_restatement.py, is pinned: with the one share 0.5 it is tests/pools_restatement.py -
   the reference on a pool's columns - bit for bit (S1), its singlet sums give the reference's singlet logits, and S3, S4, S5 and a
   pair penalty of -inf hold on it.
2. The value conditions on the seeded simulation of doublets of unequal shares.
3. The Python side that needs no device: the declaration and binding of the entry, the grid's resolution, the result class.
(The validation of the entry point: tests/test_pair_shares_plan_cpu.py.)"""
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import pair_shares_restatement as restated
from tests import pools_restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_FIXTURES = ['f1_synthetic_default.npz', 'f2_synthetic_g4.npz', 'f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz']
SMALL = ['f2_synthetic_g4.npz', 'f3_small_2.npz']


def pools_of(G, B):
    """The one pool of everybody, and two pools with a barcode in five in none."""
    yield [list(range(G))], np.zeros(B, np.int32)
    if G >= 4:
        yield [[0, 2, 3], list(range(1, G))], np.where(np.arange(B) % 5 == 4, -1, np.arange(B) % 2).astype(np.int32)


# ---- 1. the restatement, pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_s1_the_one_share_of_a_half_is_the_pooled_pass(name, doublet_prior):
    v, cb, e, prob, B = pools_restatement.fixture_problem(name)
    nonzero = prob[prob != 0]
    assert nonzero.min() >= 2.0 ** -125, 'S1 holds where no halved table entry is subnormal'
    pooled = pools_restatement.Restatement(v, cb, e, prob, B, doublet_prior)
    for pools, pool_of in pools_of(prob.shape[1], B):
        want = pooled(pools, pool_of)
        penalty = pooled.pair_penalty(pools)
        for weights in (None, [0.0]):
            out = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, doublet_prior != 0, [0.5], weights)
            pools_restatement.assert_same(out, want, f'{name} {doublet_prior}, {len(pools)} pools')
            pairs = ~out['single']
            assert pairs.any() == (doublet_prior != 0)
            restated.same_bits(out['share_mean'][pairs], np.full(int(pairs.sum()), 0.5, np.float32), 'share_mean is the one share')
            assert not out['share_index'][pairs].any() and (out['share_index'][~pairs] == -1).all() and np.isnan(out['share_mean'][~pairs]).all()
            # the singlet sums of the restatement are the reference's singlet logits: f32(f64(0) + S)
            restated.same_bits(out['S'][~pairs, 0].astype(np.float32), out['logits'][~pairs], 'singlet sums')
            # the read-outs at the best option
            found = out['best_option'] >= 0
            at = out['row_ptr'][:-1][found] + out['best_option'][found]
            assert np.array_equal(out['best_share_index'][found], out['share_index'][at]) and (out['best_share_index'][~found] == -1).all()
            assert np.array_equal(np.isnan(out['best_share_mean'][found]), out['single'][at]) and np.isnan(out['best_share_mean'][~found]).all()


@pytest.mark.parametrize('name', SMALL)
def test_s2_without_doublets_there_is_nothing_to_say_about_shares(name):
    v, cb, e, prob, B = pools_restatement.fixture_problem(name)
    pooled = pools_restatement.Restatement(v, cb, e, prob, B, 0)
    for pools, pool_of in pools_of(prob.shape[1], B):
        out = restated.restate(v, cb, e, prob, B, pools, pool_of, np.zeros(len(pools), np.float32), False, restated.DEFAULT_SHARES,
                               restated.uniform_log_weights(9))
        pools_restatement.assert_same(out, pooled(pools, pool_of), f'{name}: no pairs')
        assert (out['share_index'] == -1).all() and np.isnan(out['share_mean']).all()
        assert (out['best_share_index'] == -1).all() and np.isnan(out['best_share_mean']).all()


def singlet_sum_of_pairs(out, pools, pool_of, which):
    """float64[n pairs]: for every pair option the S of its first (which = 0) or second donor's singlet option in the same row."""
    from tests import ambient_scoring_restatement as scoring
    want = np.full(len(out['pen']), np.nan)
    for p, donors in enumerate(pools):
        d1, d2 = scoring.pool_options(list(range(len(donors))), True)  # positions in the pool's list = its singlet options
        for b in np.flatnonzero(np.asarray(pool_of) == p):
            first = out['row_ptr'][b]
            want[first:first + len(d1)] = out['S'][first + (d1, d2)[which], 0]
    return want[~out['single']]


@pytest.mark.parametrize('name', SMALL)
def test_s3_a_share_of_one_is_the_first_donor_alone_and_zero_the_second(name):
    v, cb, e, prob, B = pools_restatement.fixture_problem(name)
    for pools, pool_of in pools_of(prob.shape[1], B):
        penalty = np.linspace(-1.5, 0.5, len(pools)).astype(np.float32)
        for share, which in ((1.0, 0), (0.0, 1)):
            out = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, [share])
            pairs = ~out['single']
            want = (out['pen'][pairs] + singlet_sum_of_pairs(out, pools, pool_of, which)).astype(np.float32)
            restated.same_bits(out['logits'][pairs], want, f'{name}: share {share}')
            restated.same_bits(out['share_mean'][pairs], np.full(len(want), share, np.float32), 'the mean is the one share')
        # with a penalty of 0 a pair's logit is the singlet's own
        out = restated.restate(v, cb, e, prob, B, pools, pool_of, np.zeros(len(pools), np.float32), True, [1.0])
        restated.same_bits(out['logits'][~out['single']], singlet_sum_of_pairs(out, pools, pool_of, 0).astype(np.float32), 'penalty 0')


@pytest.mark.parametrize('name', SMALL)
def test_s4_s5_and_a_pair_penalty_without_end(name):
    v, cb, e, prob, B = pools_restatement.fixture_problem(name)
    log_two = restated.log32(np.array([2.0], np.float32))[0]
    for pools, pool_of in pools_of(prob.shape[1], B):
        penalty = np.linspace(-1.5, 0.5, len(pools)).astype(np.float32)
        # S4: a share twice adds log 2 to the float64 sum - on the pairs; a singlet knows no grid
        out = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, [0.3, 0.3])
        once = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, [0.3])
        pairs = ~out['single']
        restated.same_bits(out['logits'][pairs], (out['pen'][pairs] + (out['S'][pairs, 0] + np.float64(log_two))).astype(np.float32), 'S4')
        restated.same_bits(out['logits'][~pairs], once['logits'][~pairs], 'S4: singlets')
        restated.same_bits(out['share_mean'][pairs], np.full(int(pairs.sum()), 0.3, np.float32), 'the mean of a share with itself')
        assert not out['share_index'][pairs].any()
        # S5: zeros are no weights; a constant on every weight moves the pairs against the singlets
        grid = np.array([0.9, 0.0, 0.5, 1.0, 0.5], np.float32)
        plain = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, grid)
        zeros = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, grid, np.zeros(5, np.float32))
        restated.assert_same(zeros, plain, f'{name}: log_weights of zeros')
        uniform = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, grid, restated.uniform_log_weights(5))
        assert (uniform['logits'][pairs] < plain['logits'][pairs]).all(), 'the normalisation matters: singlets do not go through the grid'
        restated.same_bits(uniform['logits'][~pairs], plain['logits'][~pairs], 'singlets take no weights')
        assert ((plain['share_mean'][pairs] >= 0) & (plain['share_mean'][pairs] <= 1)).all()
        # a pair penalty of -inf: every pair's logit is -inf, every grid point counts once, the singlets are untouched
        endless = restated.restate(v, cb, e, prob, B, pools, pool_of, np.full(len(pools), -np.inf, np.float32), True, grid)
        assert (endless['logits'][pairs] == -np.inf).all() and np.isfinite(endless['logits'][~pairs]).all()
        restated.same_bits(endless['logits'][~pairs], plain['logits'][~pairs], '-inf: singlets')
        f = np.float32
        mean = ((((f(0.9) + f(0.0)) + f(0.5)) + f(1.0)) + f(0.5)) / f(5)
        restated.same_bits(endless['share_mean'][pairs], np.full(int(pairs.sum()), mean, f), '-inf == -inf: the grid in float32 order')
        assert not endless['share_index'][pairs].any() and not (endless['probs'][pairs] != 0).any()


@pytest.mark.parametrize('n', [1, 3, 5])
def test_shares_of_a_half_are_the_ambient_marginal_without_ambient(n):
    """What the two grid-summed passes have in one home (csrc/estep_grid_device.h), pinned on the restatements: with
    n shares of 0.5 and n ambient fractions of 0 every grid point has the same lambda - p1 0.5 + p2 0.5 and (p1 + p2) 0.5 round alike,
    q 1 + a 0 is q - so under the same log weights the two folds see the same t: the pair options' logits agree bit for bit and the
    share index is the alpha index.  (tests/test_gpu_pair_shares.py asserts the same of the device.)"""
    from tests import ambient_marginal_restatement as marginal
    v, cb, e, prob, B, _lengths, _v2snp = restated.designed_problem()
    f = np.float32
    assert prob[prob != 0].min() >= 2.0 ** -125, 'no halved table entry is subnormal'
    a, b = prob[:, :512], prob[:, 512:]
    restated.same_bits(a * f(0.5) + b * f(0.5), (a + b) * f(0.5), 'the two halvings')
    restated.same_bits(a * (f(1) - f(0)) + b[:, :1] * f(0), a, 'q 1 + a 0 is q')
    pools, pool_of, penalty, shares, alphas, ambient, weights = restated.half_shares_against_no_ambient([2, 11, 16, 23, 44], n)
    shared = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, shares, weights)
    summed = marginal.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, alphas, ambient, weights)
    assert np.array_equal(shared['row_ptr'], summed['row_ptr'])
    pairs = ~shared['single']
    restated.same_bits(shared['S'][pairs], summed['S'][pairs], 'every grid point has the same float64 sum')
    restated.same_bits(shared['logits'][pairs], summed['logits'][pairs], f'{n} grid points: the logits of the pair options')
    assert np.array_equal(shared['share_index'][pairs], summed['alpha_index'][pairs])
    assert (shared['logits'][pairs] == -np.inf).any() and np.isfinite(shared['logits'][pairs]).any()
    if n > 1:
        assert len(np.unique(shared['share_index'][pairs])) > 1, 'the weights and the penalty of -inf move the largest term'


# ---- 2. the value conditions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('share', [0.8, 0.5])
def test_the_value_conditions_hold_on_the_restated_simulation(share):
    sim, fixed, grid, out = restated.simulated(share, 128, 0)
    assert sim['B'] == 144 and int((sim['second'] < 0).sum()) == 96
    restated.value_conditions(share, fixed, grid)
    pairs = out['best_option'] >= sim['prob'].shape[1]
    assert not np.isnan(out['best_share_mean'][pairs]).any() and np.isnan(out['best_share_mean'][~pairs]).all()


# ---- 3. the Python side ----------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_and_bound():
    from demuxalot_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'demux_hip_debug.h')).read()
    assert re.search(r'^int\s+dmx_estep_pair_shares\s*\(', header, flags=re.M)
    assert 'dmx_estep_pair_shares' in _lib.DEBUG_SIGNATURES and 'dmx_estep_pair_shares' not in _lib.SIGNATURES
    assert len(_lib.DEBUG_SIGNATURES['dmx_estep_pair_shares'][1]) == 20
    contract = header[header.index('csrc/estep_pair_shares.hip'):header.index('int dmx_estep_pair_shares')]
    assert '2^-125' in contract, 'the header states the bound S1 holds on'
    assert 'normalisation of the weights matters' in contract


def test_the_grid_is_resolved_before_a_gpu_is_needed():
    import demuxalot_amd
    from demuxalot_amd.doublet_shares import resolve_shares
    assert demuxalot_amd.default_shares().dtype == np.float32
    assert demuxalot_amd.default_shares().tobytes() == restated.DEFAULT_SHARES.tobytes() and len(restated.DEFAULT_SHARES) == 9
    grid, weights = resolve_shares(None, None)
    assert grid.tobytes() == restated.DEFAULT_SHARES.tobytes() and weights.tobytes() == restated.uniform_log_weights(9).tobytes()
    grid, weights = resolve_shares([1, 0, 0.5, 0.5], [0, -1, -2, 3])
    assert grid.tolist() == [1, 0, 0.5, 0.5] and weights.dtype == np.float32 and weights.tolist() == [0, -1, -2, 3]
    for bad in ([], np.linspace(0, 1, 65), [0.5, np.nan], [-0.1], [1.5], [np.inf]):
        with pytest.raises(ValueError, match='shares'):
            resolve_shares(bad, None)
    for bad in ([0.0], [0.0, np.nan], [0.0, -np.inf], [0, 0, 0]):
        with pytest.raises(ValueError, match='share_log_weights'):
            resolve_shares([0.2, 0.8], bad)


def test_the_result_class_names_shares_and_major_donors():
    from demuxalot_amd import DoubletSharePosteriors
    # two pools: donors (a, b+c, d) with doublets - 6 options - and (b+c,) - one option; four barcodes, the third in no pool
    names = [['a', 'b+c', 'd', 'a+b+c', 'a+d', 'b+c+d'], ['b+c']]
    row_ptr = np.array([0, 6, 7, 7, 13])
    nan = np.nan
    share_mean = np.array([nan, nan, nan, 0.5, 0.8, 0.25, nan, nan, nan, nan, 0.5, 0.25, 0.75], np.float32)
    share_index = np.where(np.isnan(share_mean), -1, 1).astype(np.int32)
    result = DoubletSharePosteriors(['B0', 'B1', 'B2', 'B3'], names, [['a', 'b+c', 'd'], ['b+c']], [0, 1, -1, 0], row_ptr, [0.2, 0.8], [0.0, 0.0],
                                    share_index, share_mean, [4, 0, -1, 5], [0.9, 1.0, nan, 0.6], [0.95, 0.0, nan, 0.7], [1, -1, -1, 1],
                                    np.array([0.8, nan, nan, 0.75], np.float32), posteriors=None)
    assert result.option_shares.dtype == np.float64 and result.option_share_index.dtype == np.int32
    summary = result.summary()
    assert list(summary.columns) == ['option', 'probability', 'doublet_probability', 'share', 'major_donor'] and summary.index.name == 'BARCODE'
    assert summary['option'].tolist() == ['a+d', 'b+c', None, 'b+c+d']
    assert summary['major_donor'].tolist() == ['a', None, None, 'b+c']
    assert summary['share'].values[0] == np.float64(np.float32(0.8)) and np.isnan(summary['share'].values[1:3]).all()
    flipped = DoubletSharePosteriors(['B0'], names[:1], [['a', 'b+c', 'd']], [0], [0, 6], [0.8, 0.2], [0.0, 0.0], share_index[:6], share_mean[:6], [4], [0.9],
                                     [0.95], [0], np.array([0.2], np.float32), posteriors=None)
    assert flipped.summary()['major_donor'].tolist() == ['d']
    shares = result.shares_of('B3')
    assert isinstance(shares, pd.Series) and list(shares.index) == names[0] and shares['a+d'] == 0.25 and np.isnan(shares['a'])
    assert len(result.shares_of('B2')) == 0
