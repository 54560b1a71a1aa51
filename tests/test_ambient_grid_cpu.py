"""Every option at its own best ambient fraction, without a GPU (Demultiplexer.predict_posteriors_joint_ambient;
include/demux_hip_debug.h: dmx_estep_ambient_grid).

1. The checker of the GPU tests, tests/ambient_grid_restatement.py, is pinned: with one grid value it is the per-barcode-fraction
   restatement with that fraction everywhere (G1), and at alphas = {0} the reference's own predict_posteriors (the fixtures' captures),
   bit for bit; with penalty 0 an option's values over the grid are the ambient profile's log-likelihoods and its index their best (G3).
2. Duplicates in the grid resolve to the lower index.
3. The validation of the entry point is a pure host function (csrc/ambient_grid_plan.h): tests/ambient_grid_plan_check.cpp walks it,
   built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program.
4. The Python side: the grid's resolution, the result class.
5. The simulation with true doublets: the joint pass calls them doublets, and leaves the contaminated singlets alone."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from demuxalot_amd import ambient as amb
from tests import ambient_grid_restatement as restated
from tests import ambient_restatement as profile_restated
from tests import ambient_scoring_restatement as scoring_restated
from tests import check_program
from tests import fixture_io as fio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_FIXTURES = ['f1_synthetic_default.npz', 'f2_synthetic_g4.npz', 'f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz']
SHARED = ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass')


# ---- 1. G1 and G3 for the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
def test_one_grid_value_is_the_scoring_with_that_fraction_and_zero_is_the_reference(name):
    fx = fio.load(name)
    assert int(fx['n_predict']) >= 1
    for i in range(int(fx['n_predict'])):
        clip, doublet_prior = float(fx[f'predict{i}_clip']), float(fx[f'predict{i}_dp'])
        v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name, clip)
        soup = profile_restated.derived_ambient(v, v2snp, clip)
        logits, probs, out = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, [0.0], soup)
        fio.assert_bitwise(logits, fx[f'predict{i}_logits'], f'{name} predict {i}: logits')
        fio.assert_bitwise(probs, fx[f'predict{i}_probs'], f'{name} predict {i}: posteriors')
        assert np.array_equal(out['best_option'], fx[f'predict{i}_probs'].argmax(axis=1))
        assert not out['alpha_index'].any() and not out['best_alpha_index'].any() and out['profile'].shape == (logits.size, 1)
        for value in (-0.0, 0.37):
            _l, _p, one = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, [value], soup)
            _l, _p, want = scoring_restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, np.full(B, value, np.float32), soup)
            for key in SHARED:
                assert one[key].dtype == want[key].dtype and one[key].tobytes() == want[key].tobytes(), f'{name} predict {i}, alpha {value}: {key}'


@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
def test_options_with_penalty_zero_are_the_profile_log_likelihoods(name):
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name)
    G = prob.shape[1]
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    grid = np.array([0.0, 1.0, 0.01, 0.37, 0.63], dtype=np.float32)
    out = restated.restate(v, cb, e, prob, B, [list(range(G))], np.zeros(B, np.int32), np.zeros(1, np.float32), True, grid, soup)
    K = G * (G + 1) // 2
    profile, index = out['profile'].reshape(B, K, len(grid)), out['alpha_index'].reshape(B, K)
    d1, d2 = scoring_restated.pool_options(list(range(G)), True)
    for k in range(0, K, 1 if K <= 16 else 13):  # singlets (d, -1) and pairs all over the triangle
        a, b = d1[k], d2[k]
        want = profile_restated.restate(v, cb, e, prob, B, grid, np.full(B, a), np.full(B, -1 if a == b else b), soup)
        fio.assert_bitwise(np.ascontiguousarray(profile[:, k, :]), want['loglik'], f'{name}: option {k}')
        assert np.array_equal(index[:, k], want['best']), f'{name}: option {k}: the grid point'
        fio.assert_bitwise(np.ascontiguousarray(out['logits'].reshape(B, K)[:, k]), want['ll_best'], f'{name}: option {k}: the logit')


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------
def test_duplicates_in_the_grid_resolve_to_the_lower_index():
    name = 'f3_small_2.npz'
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name)
    G = prob.shape[1]
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    args = (v, cb, e, prob, B, [list(range(G))], np.zeros(B, np.int32), np.array([-0.5], np.float32), True)
    grid = np.array([0.3, 0.0, 0.1, 0.0, 0.3, 0.1, 0.3], dtype=np.float32)
    first_of = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0, 5: 2, 6: 0}
    out = restated.restate(*args, grid, soup)
    assert set(out['alpha_index']) <= {0, 1, 2} and len(set(out['alpha_index'])) > 1, 'only the first of equal values wins'
    single = restated.restate(*args, grid[:3], soup)
    for key in SHARED + ('alpha_index', 'best_alpha_index'):
        assert out[key].tobytes() == single[key].tobytes(), key
    for j, first in first_of.items():
        fio.assert_bitwise(np.ascontiguousarray(out['profile'][:, j]), np.ascontiguousarray(out['profile'][:, first]), f'column {j}')
    # a barcode without calls: every value is the penalty, the first grid point wins
    empty = restated.restate(v[:0], cb[:0], e[:0], prob, 2, [[0, 1]], np.zeros(2, np.int32), np.array([-0.25], np.float32), True, grid, soup)
    assert not empty['alpha_index'].any() and not empty['best_alpha_index'].any()
    fio.assert_bitwise(empty['logits'], np.array([0, 0, -0.25] * 2, np.float32))
    # NaN never wins; an option whose every value is NaN has no grid point
    nan = np.float32('nan')
    index, value = profile_restated.first_maximum(np.array([[nan, 1, 1], [nan, nan, nan], [2, nan, 3]], np.float32))
    assert index.tolist() == [1, -1, 2] and np.isnan(value[1]) and value[0] == 1 and value[2] == 3


# ---- 3. the validation header ------------------------------------------------------------------------------------------------
def test_validation_over_every_refusal(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'ambient_grid_plan_check')
    walked = re.search(r'ambient grid plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == 245, stdout  # (every EXPECT the program walks: one added or lost changes the count)


def test_the_entry_point_is_declared_bound_and_stubbed():
    from demuxalot_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'demux_hip_debug.h')).read()
    assert re.search(r'^int\s+dmx_estep_ambient_grid\s*\(', header, flags=re.M)
    assert 'dmx_estep_ambient_grid' in _lib.DEBUG_SIGNATURES and 'dmx_estep_ambient_grid' not in _lib.SIGNATURES
    assert len(_lib.DEBUG_SIGNATURES['dmx_estep_ambient_grid'][1]) == 22
    assert 'run_estep_ambient_grid' in open(os.path.join(ROOT, 'demuxalot_amd', 'csrc', 'host_stubs.cpp')).read()


# ---- 4. the Python side ---------------------------------------------------------------------------------------------------------
BARCODES = [f'BC{i}' for i in range(5)]


def test_the_grid_resolves_to_float32_values_in_the_unit_range():
    fio.assert_bitwise(amb.resolve_grid(None), np.linspace(0, 0.63, 64, dtype=np.float32))
    grid = amb.resolve_grid([0.5, 0, 1, 0.5])
    assert grid.dtype == np.float32 and grid.tolist() == [0.5, 0.0, 1.0, 0.5]
    assert amb.resolve_grid(np.float64(0.25)).tolist() == [0.25]
    assert len(amb.resolve_grid(np.zeros(64))) == 64
    for bad, message in (([], '1 .. 64'), (np.zeros(65), '1 .. 64'), ([0.1, 1.5], 'outside'), ([-0.01], 'outside'), ([float('nan')], 'outside'),
                         ([float('inf')], 'outside'), ([1.0 + 1e-6], 'outside')):
        with pytest.raises(ValueError, match=message):
            amb.resolve_grid(bad)


def test_the_result_class_composes_option_alphas_and_the_summary():
    from demuxalot_amd import JointAmbientPosteriors
    alphas = np.array([0.5, 0.0, 0.25], dtype=np.float32)
    options = [['d0', 'd1', 'd0+d1'], ['d2']]
    pool_of = np.array([0, -1, 1, 0, 0], np.int32)
    row_ptr = np.array([0, 3, 3, 4, 7, 10], np.int64)
    alpha_index = np.array([1, 2, 0, 0, 2, -1, 1, 1, 1, 1], np.int32)
    best_option = np.array([2, -1, 0, 0, -1], np.int32)
    best_prob = np.array([0.75, np.nan, 1.0, 0.5, np.nan], np.float32)
    mass = np.array([0.75, np.nan, 0.0, 0.125, np.nan])
    best_alpha_index = np.array([0, -1, 0, 2, -1], np.int32)
    frames = (pd.DataFrame(np.zeros((5, 1))), pd.DataFrame(np.zeros((5, 1))))
    result = JointAmbientPosteriors(BARCODES, options, pool_of, row_ptr, alphas, np.zeros(4, np.float32), alpha_index, best_option, best_prob, mass,
                                    best_alpha_index, frames, profile=np.zeros((10, 3), np.float32))
    assert result is not None and result.posteriors is frames and result.profile.shape == (10, 3)
    assert result.option_alphas.dtype == np.float64 and result.option_alphas.shape == (10,)
    want = np.array([0.0, 0.25, 0.5, 0.5, 0.25, np.nan, 0.0, 0.0, 0.0, 0.0])
    assert np.array_equal(np.isnan(result.option_alphas), np.isnan(want)) and np.array_equal(result.option_alphas[~np.isnan(want)], want[~np.isnan(want)])
    of_three = result.alphas_of('BC3')
    assert list(of_three.index) == options[0] and of_three.values[0] == 0.25 and np.isnan(of_three.values[1]) and of_three.values[2] == 0.0
    assert len(result.alphas_of('BC1')) == 0 and list(result.alphas_of('BC2').index) == ['d2']
    summary = result.summary()
    assert list(summary.columns) == ['option', 'probability', 'alpha', 'doublet_probability', 'at_grid_edge']
    assert list(summary.index) == BARCODES and summary.index.name == 'BARCODE'
    assert list(summary['option']) == ['d0+d1', None, 'd2', 'd0', None]
    assert summary['alpha'].values.dtype == np.float64 and summary['doublet_probability'].values.dtype == np.float64
    assert summary['alpha'].values[[0, 2, 3]].tolist() == [0.5, 0.5, 0.25] and np.isnan(summary['alpha'].values[[1, 4]]).all()
    assert summary['at_grid_edge'].tolist() == [True, False, True, False, False]  # (0.5 is the largest value of this grid)
    assert summary['probability'].values.dtype == np.float32
    without = JointAmbientPosteriors(BARCODES, options, pool_of, row_ptr, alphas, np.zeros(4, np.float32), alpha_index, best_option, best_prob, mass,
                                     best_alpha_index, frames)
    assert without.profile is None
    with pytest.raises(AssertionError, match='row_ptr'):
        JointAmbientPosteriors(BARCODES, options, np.array([0, 0, 1, 0, 0], np.int32), row_ptr, alphas, np.zeros(4, np.float32), alpha_index, best_option,
                               best_prob, mass, best_alpha_index, frames)


def test_the_front_door_refuses_before_it_needs_a_gpu():
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    genotypes = ProbabilisticGenotypes([f'd{i:02d}' for i in range(45)])
    handler = BarcodeHandler(['AAAC-1', 'AAAG-1'])
    with pytest.raises(ValueError, match='1035 options.*barcode2pool / pool2donors'):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler)
    with pytest.raises(ValueError, match='outside'):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, alphas=[0.2, 1.2])
    with pytest.raises(AssertionError, match='come together'):
        Demultiplexer.predict_posteriors_joint_ambient({}, genotypes, handler, barcode2pool={})


# ---- 5. the simulation with true doublets -------------------------------------------------------------------------------------
@pytest.mark.parametrize('calls_per_barcode', [256, 64])
def test_true_doublets_are_called_doublets_and_singlets_are_left_alone(calls_per_barcode):
    """96 singlets and 48 true doublets, true fractions 0 / 0.2 / 0.4, seed 0, default grid, derived profile, doublet_prior 0.35.
    Measured on this restatement: 256 calls - 0 of 96 singlets called doublets, 96 right, 42 of 48 doublets called (16 / 15 / 11, all
    with the right pair), median fraction of the clean doublets 0.01; 64 calls - 27 of 48 (11 / 10 / 6), 22 with the right pair, 4 of 96
    singlets called doublets, 91 right.  The three-pass workflow calls 1 of the 48 a doublet at 64 calls."""
    sim, out = restated.simulated(calls_per_barcode)
    assert np.bincount(sim['cb'], minlength=sim['B']).tolist() == [calls_per_barcode] * 144
    best_alpha = np.where(out['best_alpha_index'] >= 0, restated.DEFAULT_GRID[np.maximum(out['best_alpha_index'], 0)], np.nan)
    restated.joint_conditions(calls_per_barcode, sim, out['doublet_mass'], out['best_option'], best_alpha)
