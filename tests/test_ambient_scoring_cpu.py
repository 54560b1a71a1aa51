"""Posteriors under per-barcode ambient fractions without a GPU (Demultiplexer.predict_posteriors_with_ambient /
predict_posteriors_decontaminated; include/demux_hip_debug.h: dmx_estep_ambient).

1. The checker of the GPU tests, tests/ambient_scoring_restatement.py, is pinned to the reference: with every fraction 0 it gives the
   logits and posteriors the reference's own predict_posteriors produced (the fixtures' captures), bit for bit.
2. Its singlet columns, with penalty 0, are tests/ambient_restatement.py's log-likelihoods of the same donor and fraction, bit for bit.
3. The validation of the entry point is a pure host function (csrc/ambient_scoring_plan.h): tests/ambient_scoring_plan_check.cpp walks
   it, built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program.
4. The Python side: fractions from a Series or mapping, AmbientEstimate.fractions(), the best singlet.
5. The three-pass workflow on the seeded simulation: contaminated singlets are no longer called doublets."""
import re

import numpy as np
import pandas as pd
import pytest

from demuxalot_amd import ambient as amb
from tests import ambient_restatement as profile_restated
from tests import ambient_scoring_restatement as restated
from tests import check_program
from tests import fixture_io as fio

REFERENCE_FIXTURES = ['f1_synthetic_default.npz', 'f2_synthetic_g4.npz', 'f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz']


# ---- 1. at alpha = 0 the restatement is the reference -------------------------------------------------------------------------
@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
def test_all_zero_fractions_give_the_reference_posteriors(name):
    fx = fio.load(name)
    assert int(fx['n_predict']) >= 1
    for i in range(int(fx['n_predict'])):
        clip, doublet_prior = float(fx[f'predict{i}_clip']), float(fx[f'predict{i}_dp'])
        v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name, clip)
        soup = profile_restated.derived_ambient(v, v2snp, clip)
        logits, probs, out = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, np.zeros(B, np.float32), soup)
        fio.assert_bitwise(logits, fx[f'predict{i}_logits'], f'{name} predict {i}: logits')
        fio.assert_bitwise(probs, fx[f'predict{i}_probs'], f'{name} predict {i}: posteriors')
        assert np.array_equal(out['best_option'], fx[f'predict{i}_probs'].argmax(axis=1))
        # -0.0 is a zero too, and a profile of ones changes nothing at 0
        again, _probs, _out = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, np.full(B, -0.0, np.float32), np.ones_like(soup))
        fio.assert_bitwise(again, logits, 'alpha = -0, another profile')


# ---- 2. I2: the singlet columns are dmx_ambient_profile's log-likelihoods -------------------------------------------------------
@pytest.mark.parametrize('name', ['f2_synthetic_g4.npz', 'f3_small_2.npz'])
def test_options_with_penalty_zero_are_the_profile_log_likelihoods(name):
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(name)
    G = prob.shape[1]
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    values = np.array([0.0, 1.0, 0.01, 0.37, 0.63], dtype=np.float32)
    alpha = values[np.arange(B) % len(values)]
    out = restated.restate(v, cb, e, prob, B, [list(range(G))], np.zeros(B, np.int32), np.zeros(1, np.float32), True, alpha, soup)
    logits = out['logits'].reshape(B, -1)
    d1, d2 = restated.pool_options(list(range(G)), True)
    assert logits.shape[1] == G * (G + 1) // 2
    for k, (a, b) in enumerate(zip(d1, d2)):  # singlets (d, -1), then the pairs
        profile = profile_restated.restate(v, cb, e, prob, B, values, np.full(B, a), np.full(B, -1 if a == b else b), soup)
        fio.assert_bitwise(logits[:, k], np.ascontiguousarray(profile['loglik'][np.arange(B), np.arange(B) % len(values)]), f'{name}: option {k}')


# ---- 3. the validation header ------------------------------------------------------------------------------------------------
def test_validation_over_every_refusal(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'ambient_scoring_plan_check')
    walked = re.search(r'ambient scoring plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == 185, stdout  # (every EXPECT the program walks: one added or lost changes the count)


# ---- 4. the Python side ---------------------------------------------------------------------------------------------------------
BARCODES = [f'BC{i}' for i in range(8)]


def test_fractions_resolve_to_one_value_per_barcode():
    given = {'BC0': 0.25, 'BC1': None, 'BC2': float('nan'), 'BC3': 0, 'BC4': 1, 'BC5': np.float32(0.37), 'BC6': np.float64('nan')}  # BC7: missing
    alpha = amb.resolve_fractions(BARCODES, given)
    assert alpha.dtype == np.float32 and alpha.shape == (8,)
    fio.assert_bitwise(alpha, np.array([0.25, 0, 0, 0, 1, 0.37, 0, 0], dtype=np.float32))
    series = pd.Series({'BC7': 0.5, 'BC0': np.nan, 'BC3': 0.125})
    fio.assert_bitwise(amb.resolve_fractions(BARCODES, series), np.array([0, 0, 0, 0.125, 0, 0, 0, 0.5], dtype=np.float32))
    assert not amb.resolve_fractions(BARCODES, {}).any()
    for bad, message in (({'BC0': 1.5}, 'outside'), ({'BC0': -0.01}, 'outside'), ({'BC0': float('inf')}, 'outside'),
                         ({'BC0': 1.0 + 1e-12}, 'outside'), ({'BC9': 0.1}, 'not one of'), ({'BC0': 'much'}, 'not a number'),
                         ({'BC0': True}, 'not a number')):
        with pytest.raises(ValueError, match=message):
            amb.resolve_fractions(BARCODES, bad)


def test_estimate_fractions_and_best_singlets():
    alphas = np.array([0.5, 0.0, 0.25], dtype=np.float32)
    best = np.array([2, -1, 0, 1, 1, -1, 2, 0], dtype=np.int32)
    columns = np.where(best >= 0, 0, -1)
    nan = np.full(8, np.nan, np.float32)
    estimate = amb.AmbientEstimate(BARCODES, ['d0', 'd1', 'd0+d1'], columns, alphas, np.zeros(3, np.float32), best, nan, nan)
    fractions = estimate.fractions()
    assert isinstance(fractions, pd.Series) and list(fractions.index) == BARCODES and fractions.index.name == 'BARCODE'
    assert fractions.values.dtype == np.float64
    skipped = best < 0
    assert np.isnan(fractions.values[skipped]).all()
    assert np.array_equal(fractions.values[~skipped], alphas[best[~skipped]].astype(np.float64))
    assert np.array_equal(fractions.values[~skipped], estimate.summary()['alpha'].values[~skipped])
    # what the re-scoring reads of it: NaN -> 0
    fio.assert_bitwise(amb.resolve_fractions(BARCODES, fractions), np.where(skipped, 0, alphas[np.maximum(best, 0)]).astype(np.float32))
    # the best singlet: the first maximum over the first G columns, whatever the pair columns say
    logits = np.array([[-5, -3, -4, 0], [-2, -2, -9, -1], [-7, -8, -6, -100], [np.nan, -3, -1, 0], [np.nan] * 4], dtype=np.float32)
    assert amb.best_singlets(logits, 3).tolist() == [1, 0, 2, 2, -1]
    assert restated.best_singlets(logits[:3], 3).tolist() == [1, 0, 2]


# ---- 5. the workflow ------------------------------------------------------------------------------------------------------------
def test_contaminated_singlets_are_not_called_doublets():
    """ambient_restatement.simulate() with its defaults (8 donors, 96 singlets of 256 calls, true fractions 0 / 0.2 / 0.4),
    doublet_prior 0.35: plain scoring calls the heavily contaminated barcodes doublets; predict -> estimate (best singlet) -> re-score
    does not, and finds the true donor."""
    flow = restated.workflow()
    sim = flow['sim']
    assert np.bincount(sim['cb'], minlength=sim['B']).tolist() == [256] * 96
    restated.workflow_conditions(sim, flow['plain']['doublet_mass'], flow['rescored']['doublet_mass'], flow['rescored']['best_option'])
    truth = sim['truth']
    print('true donor is the best singlet of the plain pass for', int((flow['singlet'] == sim['donor1']).sum()), 'of 96')
    print('medians of the estimated fractions at true 0 / 0.2 / 0.4:', [float(np.median(flow['fractions'][truth == t])) for t in (0.0, 0.2, 0.4)])
    print('plain scoring, barcodes called doublets per group:', [int((flow['plain']['doublet_mass'][truth == t] > 0.5).sum()) for t in (0.0, 0.2, 0.4)])
