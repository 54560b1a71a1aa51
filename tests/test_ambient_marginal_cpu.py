"""The grid of ambient fractions summed instead of searched, without a GPU (Demultiplexer.predict_posteriors_joint_ambient with
over_grid='marginal'; include/demux_hip_debug.h: dmx_estep_ambient_grid_marginal).

1. The checker of the GPU tests, tests/ambient_marginal_restatement.py, is pinned: its float64 sums give the max mode's profile bit
   for bit, and the identities M1 .. M5 of the contract hold on it.
2. The recurrence on hand-made rows: NaN skipped, -inf meeting a number and -inf, the order of the sums.
3. The Python side: the keywords, the result class.
4. The simulation with true doublets: the marginal finds more of them among droplets with few calls.
(The validation of the entry point: tests/test_ambient_marginal_plan_cpu.py.)"""
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import ambient_grid_restatement as grid_restated
from tests import ambient_marginal_restatement as restated
from tests import ambient_restatement as profile_restated
from tests import fixture_io as fio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_FIXTURES = ['f1_synthetic_default.npz', 'f2_synthetic_g4.npz', 'f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz']
GRID = np.array([0.0, 1.0, 0.01, 0.37, 0.63], dtype=np.float32)


def all_donors(name, doublet_prior):
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name)
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    return (v, cb, e, prob, B, doublet_prior), soup


# ---- 1. the sums, and M1 .. M5 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
@pytest.mark.parametrize('doublet_prior', [0.0, 0.35])
def test_the_float64_sums_give_the_max_modes_profile_and_m2_m3_m5_hold(name, doublet_prior):
    problem, soup = all_donors(name, doublet_prior)
    _l, _p, maximum = grid_restated.restate_all_donors(*problem, GRID, soup)
    _l, _p, out = restated.restate_all_donors(*problem, GRID, soup)
    restated.same_bits(out['lam'], maximum['profile'], f'{name} {doublet_prior}: f32(f64(pen) + S)')
    # M2: the grid point of the largest term is the max mode's
    # (best_alpha_index is that entry at best_option, which is the max mode's wherever the two modes choose the same option)
    assert np.array_equal(out['alpha_index'], maximum['alpha_index'])
    same_choice = out['best_option'] == maximum['best_option']
    assert same_choice.any() and np.array_equal(out['best_alpha_index'][same_choice], maximum['best_alpha_index'][same_choice])
    assert np.array_equal(out['best_alpha_index'], out['alpha_index'][out['row_ptr'][:-1] + out['best_option']])
    # M3: no logit below the max mode's, NaN with NaN
    assert np.array_equal(np.isnan(out['logits']), np.isnan(maximum['logits']))
    assert (out['logits'] >= maximum['logits'])[~np.isnan(maximum['logits'])].all()
    assert (out['logits'] > maximum['logits']).any(), 'five grid values add something somewhere'
    # the mean lies inside the grid's range
    assert ((out['alpha_mean'] >= 0) & (out['alpha_mean'] <= 1)).all()
    # M5: zeros are no weights
    _l, _p, zeros = restated.restate_all_donors(*problem, GRID, soup, np.zeros(len(GRID), np.float32))
    restated.assert_same(zeros, out, f'{name} {doublet_prior}: log_weights of zeros')
    # ... and under a prior the grid point is the first maximum of lambda + log_weights, in float32
    weights = np.array([0, -50, 0.5, -50, -3], np.float32)
    _l, _p, steep = restated.restate_all_donors(*problem, GRID, soup, weights)
    index, _value = profile_restated.first_maximum(out['lam'] + weights[None, :])
    assert np.array_equal(steep['alpha_index'], index)


@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
def test_m1_one_grid_value_is_the_max_mode_and_zero_is_the_reference(name):
    fx = fio.load(name)
    for i in range(int(fx['n_predict'])):
        clip, doublet_prior = float(fx[f'predict{i}_clip']), float(fx[f'predict{i}_dp'])
        v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name, clip)
        soup = profile_restated.derived_ambient(v, v2snp, clip)
        for weights in (None, [0.0]):
            logits, probs, out = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, [0.0], soup, weights)
            fio.assert_bitwise(logits, fx[f'predict{i}_logits'], f'{name} predict {i}: logits')
            fio.assert_bitwise(probs, fx[f'predict{i}_probs'], f'{name} predict {i}: posteriors')
            assert not out['alpha_index'].any() and not out['alpha_mean'].any()
        for value in (-0.0, 0.37):
            _l, _p, one = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, [value], soup)
            _l, _p, want = grid_restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, [value], soup)
            for key in restated.SHARED + ('alpha_index', 'best_alpha_index'):
                restated.same_bits(one[key], want[key], f'{name} predict {i}, alpha {value}: {key}')
            restated.same_bits(one['alpha_mean'], np.full(len(one['logits']), value, np.float32), 'alpha_mean is the one grid value')


@pytest.mark.parametrize('name', ['f2_synthetic_g4.npz', 'f3_small_2.npz'])
def test_m4_the_grid_of_one_value_twice_adds_log_two(name):
    problem, soup = all_donors(name, 0.35)
    _l, _p, out = restated.restate_all_donors(*problem, [0.25, 0.25], soup)
    log_two = restated.log32(np.array([2.0], np.float32))[0]
    want = (out['pen'] + (out['S'][:, 0] + np.float64(log_two))).astype(np.float32)
    restated.same_bits(out['logits'], want, f'{name}: f32(f64(pen) + (S + f64(log 2)))')
    assert not out['alpha_index'].any()
    restated.same_bits(out['alpha_mean'], np.full(len(want), 0.25, np.float32), 'the mean of a value with itself')


# ---- 2. the recurrence on hand-made rows -------------------------------------------------------------------------------------------
def test_the_recurrence_skips_nan_and_meets_infinities():
    nan, inf = np.nan, np.inf
    alphas = np.array([0.0, 0.5, 1.0], np.float32)
    S = np.array([[nan, nan, nan],     # the state stays empty
                  [nan, -3.0, nan],    # one value
                  [-inf, -inf, -inf],  # -inf == -inf: counted, the logit -inf
                  [-inf, -2.0, -inf],  # a number after -inf, -inf after a number
                  [-1.0, -1.0, -1.0],  # equal values
                  [-1.0, -2.0, -0.5]])
    logits, jm, mean, lam = restated.over_the_grid(S, np.zeros(len(S)), alphas)
    assert jm.tolist() == [-1, 1, 0, 1, 0, 2]
    assert np.isnan(logits[0]) and np.isnan(mean[0])
    assert logits[1] == np.float32(-3) and mean[1] == np.float32(0.5)
    assert logits[2] == -inf and mean[2] == np.float32(0.5)  # s = 3, u = 0 + 0.5 + 1
    assert logits[3] == np.float32(-2) and mean[3] == np.float32(0.5)  # exp(-inf) = 0 on both sides
    log_three = restated.log32(np.array([3.0], np.float32))[0]
    assert logits[4] == np.float32(np.float64(-1) + np.float64(log_three)) and mean[4] == np.float32(1.5) / np.float32(3)
    # the last row, step by step in float32
    f = np.float32
    x = restated.exp32(np.array([-1.0], f))[0]           # t = -2 below m = -1
    s, u = f(1) + x, f(0) + f(0.5) * x
    r = restated.exp32(np.array([-0.5], f))[0]           # t = -0.5 above m = -1
    s, u = f(s * r) + f(1), f(u * r) + f(1)
    assert logits[5] == f(np.float64(-0.5) + np.float64(restated.log32(np.array([s], f))[0])) and mean[5] == u / s
    # log weights: the largest term moves, the correction carries the weight of its grid point
    logits_w, jm_w, _mean, _lam = restated.over_the_grid(S[5:], np.zeros(1), alphas, np.array([0.0, 0.0, -4.0], f))
    assert jm_w.tolist() == [0] and logits_w[0] > f(-1) and logits_w[0] < logits[5]


# ---- 3. the Python side ----------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_bound_and_stubbed():
    from demuxalot_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'demux_hip_debug.h')).read()
    assert re.search(r'^int\s+dmx_estep_ambient_grid_marginal\s*\(', header, flags=re.M)
    assert 'dmx_estep_ambient_grid_marginal' in _lib.DEBUG_SIGNATURES and 'dmx_estep_ambient_grid_marginal' not in _lib.SIGNATURES
    assert len(_lib.DEBUG_SIGNATURES['dmx_estep_ambient_grid_marginal'][1]) == 24
    assert len(_lib.DEBUG_SIGNATURES['dmx_estep_ambient_grid'][1]) == 22, 'the max entry keeps its declaration'


def test_the_front_door_refuses_before_it_needs_a_gpu():
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    genotypes = ProbabilisticGenotypes([f'd{i:02d}' for i in range(4)])
    handler = BarcodeHandler(['AAAC-1', 'AAAG-1'])
    with pytest.raises(ValueError, match="over_grid='max'"):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, over_grid='marginal', keep_profile=True)
    with pytest.raises(ValueError, match="'max' or 'marginal'"):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, over_grid='mean')
    with pytest.raises(ValueError, match='alpha_log_weights'):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, alpha_log_weights=[0.0])
    with pytest.raises(ValueError, match='one finite value per grid value'):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, alphas=[0.0, 0.1], over_grid='marginal', alpha_log_weights=[0.0])
    with pytest.raises(ValueError, match='one finite value per grid value'):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, alphas=[0.0, 0.1], over_grid='marginal',
                                                       alpha_log_weights=[0.0, -np.inf])


def test_the_result_class_carries_the_mode_and_the_means():
    from demuxalot_amd import JointAmbientPosteriors
    barcodes = [f'BC{i}' for i in range(3)]
    alphas = np.array([0.5, 0.0], dtype=np.float32)
    options = [['d0', 'd1', 'd0+d1']]
    pool_of, row_ptr = np.array([0, -1, 0], np.int32), np.array([0, 3, 3, 6], np.int64)
    alpha_index = np.array([1, 0, 0, -1, 1, 1], np.int32)
    mean = np.array([0.125, 0.5, 0.25, np.nan, 0.0, 0.375], np.float32)
    args = (barcodes, options, pool_of, row_ptr, alphas, np.zeros(4, np.float32), alpha_index, np.array([2, -1, 1], np.int32),
            np.array([0.75, np.nan, 1.0], np.float32), np.array([0.75, np.nan, 0.0]), np.array([0, -1, 1], np.int32),
            (pd.DataFrame(np.zeros((3, 1))), pd.DataFrame(np.zeros((3, 1)))))
    result = JointAmbientPosteriors(*args, over_grid='marginal', alpha_mean=mean, best_alpha_mean=np.array([0.25, np.nan, 0.0], np.float32))
    assert result.over_grid == 'marginal' and result.option_alpha_means.dtype == result.option_alphas.dtype == np.float64
    assert result.option_alpha_means.shape == result.option_alphas.shape == (6,)
    assert result.option_alpha_means[[0, 1, 2, 4, 5]].tolist() == [0.125, 0.5, 0.25, 0.0, 0.375] and np.isnan(result.option_alpha_means[3])
    summary = result.summary()
    assert list(summary.columns) == ['option', 'probability', 'alpha', 'doublet_probability', 'at_grid_edge', 'alpha_mean']
    assert summary['alpha_mean'].values.dtype == np.float64
    assert summary['alpha_mean'].values[[0, 2]].tolist() == [0.25, 0.0] and np.isnan(summary['alpha_mean'].values[1])
    plain = JointAmbientPosteriors(*args)
    assert plain.over_grid == 'max' and plain.option_alpha_means is None
    assert list(plain.summary().columns) == ['option', 'probability', 'alpha', 'doublet_probability', 'at_grid_edge']
    with pytest.raises(AssertionError):
        JointAmbientPosteriors(*args, over_grid='marginal')


# ---- 4. the simulation with true doublets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('calls_per_barcode', [256, 64])
def test_the_marginal_finds_more_of_the_true_doublets(calls_per_barcode):
    """96 singlets and 48 true doublets, seed 0, default grid, derived profile, doublet_prior 0.35; "doublet" is pair mass above 0.5.
    Measured on this restatement (max -> marginal): 64 calls - 27 -> 34 of 48 doublets called, 4 -> 5 of 96 singlets called
    doublets, 91 -> 91 singlets right; 256 calls - 42 -> 45, 0 -> 0, 96 -> 96."""
    sim, maximum, marginal = restated.simulated(calls_per_barcode)
    # the max mode built from this file's sums is tests/ambient_grid_restatement.py's
    _sim, pinned = grid_restated.simulated(calls_per_barcode)
    restated.same_bits(maximum['logits'], pinned['logits'], 'the max mode from the same sums')
    restated.same_bits(maximum['doublet_mass'], pinned['doublet_mass'], 'the max mode from the same sums: pair mass')
    max_counts = restated.counts_of(sim, maximum['doublet_mass'], maximum['best_option'])
    counts = restated.counts_of(sim, marginal['doublet_mass'], marginal['best_option'])
    restated.marginal_conditions(calls_per_barcode, sim, max_counts, counts)
