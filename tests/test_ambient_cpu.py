"""Ambient RNA fractions without a GPU (Demultiplexer.estimate_ambient; include/demux_hip_debug.h: dmx_ambient_profile).

1. The checker of the GPU tests, tests/ambient_restatement.py, is pinned to the reference: its alpha = 0 column of a singlet is the
   donor's column of the logits the reference's own predict_posteriors produced (the fixtures' captures), bit for bit.
2. The validation of the entry point is a pure host function (csrc/ambient_plan.h): tests/ambient_plan_check.cpp walks it, built with
   AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program.
3. The Python side - assignments to table columns, the summary frame - on the restatement's outputs.
4. The model recovers known contamination on a seeded simulation."""
import re

import numpy as np
import pandas as pd
import pytest

from demuxalot_amd import ambient as amb
from demuxalot_amd.demux import _option_names
from tests import ambient_restatement as restated
from tests import check_program
from tests import fixture_io as fio

REFERENCE_FIXTURES = ['f1_synthetic_default.npz', 'f2_synthetic_g4.npz', 'f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz']


# ---- 1. the restatement against the reference's captured logits ---------------------------------------------------------------
@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
def test_alpha_zero_of_a_singlet_is_the_reference_logit(name):
    fx = fio.load(name)
    G = len(fx['genotype_names'])
    assert int(fx['n_predict']) >= 1
    for i in range(int(fx['n_predict'])):
        clip = float(fx[f'predict{i}_clip'])
        v, cb, e, prob, B, v2snp = restated.fixture_problem(name, clip)
        soup = restated.derived_ambient(v, v2snp, clip)
        alphas = np.array([0.3, 0.0, 1.0], dtype=np.float32)  # (the zero is not the first column)
        for d in range(G):
            got = restated.restate(v, cb, e, prob, B, alphas, np.full(B, d), np.full(B, -1), soup)
            fio.assert_bitwise(got['loglik'][:, 1], np.ascontiguousarray(fx[f'predict{i}_logits'][:, d]), f'{name} predict {i} donor {d}')
            fio.assert_bitwise(got['ll_zero'], got['loglik'][:, 1], 'll_zero is that column')


def test_derived_profile_is_the_share_of_calls_within_the_snp():
    name = 'f1_synthetic_default.npz'
    v, _cb, _e, _prob, _B, v2snp = restated.fixture_problem(name)
    soup = restated.derived_ambient(v, v2snp, 0.01)
    assert soup.dtype == np.float32 and soup.shape == v2snp.shape and (soup >= np.float32(0.01)).all() and (soup <= np.float32(0.99)).all()
    count = np.bincount(v, minlength=len(v2snp)) + 1.0
    share = count / np.bincount(v2snp, weights=count)[v2snp]
    np.testing.assert_allclose(soup, share.clip(0.01, 0.99), rtol=1e-6)
    # a SNP nobody called comes out uniform
    nobody = restated.derived_ambient(np.zeros(0, dtype=np.int32), np.array([0, 0, 1, 1, 1], dtype=np.int32), 0.01)
    fio.assert_bitwise(nobody, np.array([1 / 2, 1 / 2, 1 / 3, 1 / 3, 1 / 3], dtype=np.float32))


# ---- 2. the validation header ------------------------------------------------------------------------------------------------
def test_validation_over_every_refusal(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'ambient_plan_check')
    walked = re.search(r'ambient plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == 42253, stdout  # (every EXPECT the program walks: one added or lost changes the count)


# ---- 3. the Python side ---------------------------------------------------------------------------------------------------------
DONORS = ['d0', 'a+b', 'd2', 'b']  # (a donor whose name contains '+', and 'a+b' + 'b' next to it)
BARCODES = [f'BC{i}' for i in range(8)]


def test_assignments_resolve_to_table_columns():
    options = _option_names(DONORS, 1)
    assert options[:4] == DONORS and options[4:] == ['d0+a+b', 'd0+d2', 'd0+b', 'a+b+d2', 'a+b+b', 'd2+b']
    assignments = {'BC0': 'd0', 'BC1': 'a+b', 'BC2': 'a+b+b', 'BC3': 5, 'BC4': None, 'BC5': float('nan'), 'BC6': -1}  # BC7: not mentioned
    columns = amb.resolve_assignments(options, BARCODES, assignments)
    assert columns.tolist() == [0, 1, 8, 5, -1, -1, -1, -1]
    d1, d2 = amb.assigned_donors(len(DONORS), columns)
    assert d1.dtype == np.int32 and d2.dtype == np.int32
    assert d1.tolist() == [0, 1, 1, 0, -1, -1, -1, -1] and d2.tolist() == [-1, -1, 3, 2, -1, -1, -1, -1]  # 'a+b' the donor, ('a+b', 'b') the pair
    # a Series, as DevicePosteriors.assignments() and PooledPosteriors.assignments() return it; numpy integers are columns too
    series = pd.Series({'BC7': 'd2+b', 'BC0': np.int64(3), 'BC1': np.int32(-1), 'BC2': np.float64('nan')})
    assert amb.resolve_assignments(options, BARCODES, series).tolist() == [3, -1, -1, -1, -1, -1, -1, 9]
    for bad, message in (({'BC0': 'b+a+b'}, 'not an option'), ({'BC0': 'nobody'}, 'not an option'), ({'BC0': 10}, 'outside'),
                         ({'BC0': -2}, 'outside'), ({'BC9': 'd0'}, 'not one of'), ({'BC0': 1.5}, 'not an option')):
        with pytest.raises(ValueError, match=message):
            amb.resolve_assignments(options, BARCODES, bad)


def test_default_grid():
    grid = amb.default_alphas()
    fio.assert_bitwise(grid, restated.DEFAULT_GRID)
    assert grid.dtype == np.float32 and grid.shape == (64,) and grid[0] == 0 and grid[-1] == np.float32(0.63) and (np.diff(grid) > 0).all()


def test_summary_columns_on_restated_outputs():
    name = 'f3_small_2.npz'  # G = 5
    v, cb, e, prob, B, v2snp = restated.fixture_problem(name)
    fx = fio.load(name)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = [str(s) for s in fx['barcodes']]
    options = _option_names(donors, 1)
    assignments = {bc: (None if b % 4 == 3 else options[(3 * b) % len(options)]) for b, bc in enumerate(barcodes)}
    columns = amb.resolve_assignments(options, barcodes, assignments)
    d1, d2 = amb.assigned_donors(len(donors), columns)
    alphas = np.array([0.5, 0.0, 0.25, 0.5], dtype=np.float32)  # (the largest value twice: the edge is a value, not a position)
    out = restated.restate(v, cb, e, prob, B, alphas, d1, d2, restated.derived_ambient(v, v2snp, 0.01))
    estimate = amb.AmbientEstimate(barcodes, options, columns, alphas, out['ambient'], out['best'], out['ll_best'], out['ll_zero'],
                                   loglik=out['loglik'])
    summary = estimate.summary()
    assert list(summary.columns) == ['option', 'alpha', 'log_likelihood_ratio', 'at_grid_edge']
    assert list(summary.index) == barcodes and summary.index.name == 'BARCODE'
    skipped = columns < 0
    assert skipped.any() and (~skipped).any()
    assert summary['option'][skipped].isna().all() and summary['alpha'][skipped].isna().all()
    assert summary['log_likelihood_ratio'][skipped].isna().all() and not summary['at_grid_edge'][skipped].any()
    assert list(summary['option'][~skipped]) == [assignments[bc] for bc, s in zip(barcodes, skipped) if not s]
    best = out['best'][~skipped]
    assert (best != 3).all(), 'the first maximum: never the second 0.5'
    assert np.array_equal(summary['alpha'].values[~skipped], alphas[best].astype(np.float64))
    ratio = out['ll_best'].astype(np.float64) - out['ll_zero'].astype(np.float64)
    assert summary['log_likelihood_ratio'].values.dtype == np.float64
    assert np.array_equal(summary['log_likelihood_ratio'].values[~skipped], ratio[~skipped]) and (ratio[~skipped] >= 0).all()
    assert np.array_equal(summary['at_grid_edge'].values[~skipped], alphas[best] == np.float32(0.5))
    assert estimate.profile.shape == (B, 4) and estimate.profile.values.dtype == np.float32 and list(estimate.profile.index) == barcodes
    fio.assert_bitwise(estimate.profile.values[~skipped], out['loglik'][~skipped])
    assert amb.AmbientEstimate(barcodes, options, columns, alphas, out['ambient'], out['best'], out['ll_best'], out['ll_zero']).profile is None
    # a grid without 0: no ratio
    no_zero = restated.restate(v, cb, e, prob, B, alphas[[0, 2]], d1, d2, out['ambient'])
    assert np.isnan(no_zero['ll_zero']).all()
    lone = amb.AmbientEstimate(barcodes, options, columns, alphas[[0, 2]], out['ambient'], no_zero['best'], no_zero['ll_best'], no_zero['ll_zero'])
    assert lone.summary()['log_likelihood_ratio'].isna().all() and not lone.summary()['alpha'][~skipped].isna().any()


# ---- 4. recovery ----------------------------------------------------------------------------------------------------------------
def test_known_contamination_is_recovered():
    """8 donors, 600 biallelic SNPs, 96 barcodes of 256 calls, true fractions 0 / 0.2 / 0.4, the soup the mean genotype: the median
    estimate of every group lies within 0.1 of its truth, and the three medians are strictly ordered."""
    sim, out = restated.simulated()
    assert np.bincount(sim['cb'], minlength=sim['B']).tolist() == [256] * 96
    medians = restated.recovery_condition(amb.default_alphas(), out['best'], sim['truth'])
    print('medians of the estimates at true fractions 0 / 0.2 / 0.4:', medians)
    # no tied maxima: the estimate does not hang on the tie rule
    top = out['loglik'] == out['ll_best'][:, None]
    assert (top.sum(axis=1) == 1).all()
