"""The grid of ambient fractions summed instead of searched, on the GPU (include/demux_hip_debug.h: dmx_estep_ambient_grid_marginal;
csrc/estep_ambient_grid.hip: the MARGINAL forms; Demultiplexer.predict_posteriors_joint_ambient(over_grid='marginal')).

No tolerances: everything is compared bit for bit with tests/ambient_marginal_restatement.py (pinned on the CPU in
tests/test_ambient_marginal_cpu.py) and with the max entry through the identities M1 .. M5.  The shapes are the smallest at which the
kernels can go wrong: option counts on either side of every slot boundary, so that every form runs, grid lengths on either side of
the grid points a form takes per walk, unsorted grids with duplicates, a barcode without calls, barcodes in no pool."""
import functools

import numpy as np
import pytest

from tests import ambient_marginal_restatement as restated
from tests import ambient_restatement as profile_restated
from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests.pooled_helpers import at, designed_grid, exact_mode, same_bytes, spread_columns  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1, F2, SMALL = helpers.F1, helpers.F2, helpers.F3_SMALL[2]  # G = 20, 4, 5
SHARED = restated.SHARED
GRID = np.array([0.0, 1.0, 0.01, 0.37, 0.63], dtype=np.float32)
WEIGHTS = np.array([-0.5, -7.0, 0.25, -1.0, -2.5], dtype=np.float32)
resident = functools.lru_cache(maxsize=None)(helpers.new_resident)  # (ctx, v, cb, e, prob, B, v2snp), the contexts this module's own


def marginal(ctx, *args, **kwargs):
    return ctx.estep_ambient_grid(*args, over_grid='marginal', **kwargs)


# ---- 1. M1 on the fixtures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [F1, F2])
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_m1_one_grid_value_is_the_max_entry_and_the_pass_with_that_fraction(name, doublet_prior):
    from oracle import demux_oracle
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    penalty = np.array([demux_oracle.doublet_penalties(G, doublet_prior)[-1]], np.float32)
    for value in (0.0, 0.37):
        grid = ctx.estep_ambient_grid(pools, pool_of, doublet_prior != 0, penalty, [value])
        scored = ctx.estep_ambient(pools, pool_of, doublet_prior != 0, penalty, np.full(B, value, np.float32))
        for weights in (None, [0.0]):
            got = marginal(ctx, pools, pool_of, doublet_prior != 0, penalty, [value], log_weights=weights)
            same_bytes(got, grid, SHARED + ('ambient', 'alpha_index', 'best_alpha_index'), f'{name} {doublet_prior} alpha {value}: the max entry')
            same_bytes(got, scored, SHARED + ('ambient',), f'{name} {doublet_prior} alpha {value}: dmx_estep_ambient')
            assert not np.isnan(got['logits']).any()
            fio.assert_bitwise(got['alpha_mean'], np.full(len(got['logits']), value, np.float32), 'alpha_mean is the one grid value')
            fio.assert_bitwise(got['best_alpha_mean'], np.full(B, value, np.float32), 'best_alpha_mean is the one grid value')
    same_bytes(marginal(ctx, pools, pool_of, doublet_prior != 0, penalty, [0.0]), ctx.estep_pools(pools, pool_of, doublet_prior != 0, penalty), SHARED,
               f'{name} {doublet_prior}: alphas = {{0}} is the pooled pass')


# ---- 2. the designed problem ------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 40, 5]  # calls of a barcode: none, either side of the 8-call padding
ONE_SLOT_SINGLETS, TWO_SLOT_SINGLETS = [1, 63, 64], [65, 127, 128]
WIDE_SINGLETS = [129, 255, 256, 257, 511, 512, 513, 1024]
ONE_SLOT_DOUBLETS, TWO_SLOT_DOUBLETS, WIDE_DOUBLETS = [2, 10], [11, 15], [16, 22, 23, 31, 32, 44]


DESIGNED = dict(lengths=LENGTHS, V=48, B=48, seed=23, zero_share=0.05)


@functools.lru_cache(maxsize=None)
def designed():
    """48 barcodes, barcode i with LENGTHS[i % 12] calls (barcode 0 has none), on 1024 donors and 24 biallelic SNPs (48 variants);
    error probabilities at both ends of their range and table entries of exactly 0 and 1 among them."""
    assert LENGTHS[0] == 0
    return helpers.install_arrays(*helpers.designed_arrays(**DESIGNED))


def designed_weights(n):
    """A non-uniform prior in logs: both signs, a value that all but removes its grid point."""
    weights = np.random.default_rng(200 + n).uniform(-3, 1, size=n).astype(np.float32)
    weights[n // 2] = -60.0
    return weights


def check_designed(pools, with_doublets, penalty, grid, what, priors=('null', 'zeros', 'prior'), derived=False):
    """The device against the restatement under each prior, and M2, M3, M5 against the max entry; returns the call without a prior."""
    ctx, v, cb, e, prob, B, v2snp, soup, lengths = designed()
    pool_of = (np.arange(B) % (len(pools) + 1)).astype(np.int32)
    pool_of[pool_of == len(pools)] = -1
    assert (pool_of < 0).any() and pool_of[0] == 0, 'barcodes in no pool; the barcode without calls is in one'
    profile = profile_restated.derived_ambient(v, v2snp, 0.01) if derived else soup
    supplied = None if derived else soup
    args = (pools, pool_of, with_doublets, penalty, grid)
    plain = None
    for prior in priors:
        weights = {'null': None, 'zeros': np.zeros(len(grid), np.float32), 'prior': designed_weights(len(grid))}[prior]
        got = marginal(ctx, *args, ambient=supplied, log_weights=weights)
        if prior == 'zeros' and plain is not None:  # M5
            same_bytes(got, plain, SHARED + ('ambient',) + restated.OWN, f'{what}: zeros are no weights')
            continue
        want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, with_doublets, grid, profile, weights)
        restated.assert_same(got, want, f'{what}, {prior}')
        none = pool_of < 0
        assert (got['best_option'][none] == -1).all() and np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all()
        assert (got['best_alpha_index'][none] == -1).all() and np.isnan(got['best_alpha_mean'][none]).all()
        some = got['best_option'] >= 0
        at = got['row_ptr'][:-1][some] + got['best_option'][some]
        assert np.array_equal(got['best_alpha_index'][some], got['alpha_index'][at])
        fio.assert_bitwise(got['best_alpha_mean'][some], got['alpha_mean'][at], f'{what}: best_alpha_mean is alpha_mean at the best option')
        if prior == 'null':
            plain = got
            maximum = ctx.estep_ambient_grid(*args, ambient=supplied)
            assert np.array_equal(got['alpha_index'], maximum['alpha_index']), f'{what}: M2'
            same_choice = got['best_option'] == maximum['best_option']
            assert np.array_equal(got['best_alpha_index'][same_choice], maximum['best_alpha_index'][same_choice]), f'{what}: M2, best'
            assert np.array_equal(np.isnan(got['logits']), np.isnan(maximum['logits'])), f'{what}: M3, NaN goes with NaN'
            assert (got['logits'] >= maximum['logits'])[~np.isnan(maximum['logits'])].all(), f'{what}: M3'
            # the barcode without calls: lambda = pen at every grid point, so s = n and the mean is the grid's mean in float32 order
            row = slice(got['row_ptr'][0], got['row_ptr'][1])
            assert lengths[0] == 0 and not got['alpha_index'][row].any()
    return plain


@pytest.mark.parametrize('n_alphas', [1, 3, 4, 5, 8, 9])
def test_one_slot_pools_with_grids_around_the_four_points_per_walk(n_alphas):
    grid = designed_grid(n_alphas)
    rng = np.random.default_rng(3)
    singlets = [spread_columns(rng, K) for K in ONE_SLOT_SINGLETS]
    check_designed(singlets, False, np.linspace(-1, 1, len(singlets)).astype(np.float32), grid, f'one-slot singlet pools, {n_alphas} grid values',
                   derived=n_alphas == 5)
    doublets = [spread_columns(rng, g) for g in ONE_SLOT_DOUBLETS]
    assert [g * (g + 1) // 2 for g in ONE_SLOT_DOUBLETS] == [3, 55]
    check_designed(doublets, True, np.array([-2.0, 1.5], np.float32), grid, f'one-slot doublet pools, {n_alphas} grid values', derived=n_alphas == 4)


@pytest.mark.parametrize('n_alphas', [1, 2, 3])
def test_two_slot_pools_with_grids_around_the_two_points_per_walk(n_alphas):
    grid = designed_grid(n_alphas)
    rng = np.random.default_rng(5)
    singlets = [spread_columns(rng, K) for K in TWO_SLOT_SINGLETS]
    check_designed(singlets, False, np.linspace(-1, 1, len(singlets)).astype(np.float32), grid, f'two-slot singlet pools, {n_alphas} grid values')
    doublets = [spread_columns(rng, g) for g in TWO_SLOT_DOUBLETS]
    assert [g * (g + 1) // 2 for g in TWO_SLOT_DOUBLETS] == [66, 120]
    check_designed(doublets, True, np.array([-2.0, 1.5], np.float32), grid, f'two-slot doublet pools, {n_alphas} grid values', derived=n_alphas == 2)


def test_wide_singlet_pools_on_either_side_of_every_slot_boundary():
    rng = np.random.default_rng(3)
    pools = [spread_columns(rng, K) for K in WIDE_SINGLETS]
    assert pools[-1] == list(range(1024))
    grid = np.array([0.37, 0.0, 1.0, 0.37], dtype=np.float32)
    check_designed(pools, False, np.linspace(-1, 1, len(pools)).astype(np.float32), grid, 'wide singlet pools')


def test_wide_doublet_pools_of_every_bucket():
    rng = np.random.default_rng(4)
    pools = [spread_columns(rng, g) for g in WIDE_DOUBLETS]
    assert [g * (g + 1) // 2 for g in WIDE_DOUBLETS] == [136, 253, 276, 496, 528, 990]
    grid = np.array([0.63, 0.0, 0.63], dtype=np.float32)
    check_designed(pools, True, np.linspace(-2, 1.5, len(pools)).astype(np.float32), grid, 'wide doublet pools', derived=True)


def test_a_grid_of_64_values_on_pools_of_several_forms():
    rng = np.random.default_rng(6)
    grid = designed_grid(64)
    check_designed([spread_columns(rng, K) for K in (63, 65)], False, np.array([0.5, -0.5], np.float32), grid, '64 grid values, singlets',
                   priors=('null', 'prior'))
    check_designed([spread_columns(rng, g) for g in (2, 10, 11, 16)], True, np.array([0.5, -0.5, 1.0, -1.0], np.float32), grid,
                   '64 grid values, doublets', priors=('null', 'prior'))
    check_designed([spread_columns(rng, g) for g in (10, 16)], True, np.array([0.5, -0.5], np.float32), np.linspace(0, 0.63, 64, dtype=np.float32),
                   'the default grid', priors=('null',))


def test_m4_and_table_entries_of_zero_and_penalties_without_end():
    """Table entries of exactly 0 under the grids {0, 0.1} and {0, 0} (the floor max(e, 1e-4) keeps every term finite, so lambda is a
    number there - the restatement says so too); a pair penalty of -inf is what makes t = -inf on the device: -inf == -inf counts, the
    logit is -inf, the mean the grid's.  M4 on the way: the grid {a, a} adds log_f32(2) to the float64 sum."""
    ctx, v, cb, e, prob, B, v2snp, soup, lengths = designed()
    assert (prob == 0).mean() > 0.03
    rng = np.random.default_rng(8)
    pools = [spread_columns(rng, g) for g in (3, 11, 16)]
    for grid in ([0.0, 0.1], [0.0, 0.0], [0.25, 0.25]):
        grid = np.array(grid, np.float32)
        got = check_designed(pools, True, np.array([-0.5, 0.5, 0.0], np.float32), grid, f'zeros in the table, grid {grid.tolist()}')
        assert np.isfinite(got['logits']).all()
        if grid[0] == grid[1]:  # M4
            pool_of = (np.arange(B) % 4).astype(np.int32)
            pool_of[pool_of == 3] = -1
            row_ptr, S, pen = restated.float64_sums(v, cb, e, prob, B, pools, pool_of, np.array([-0.5, 0.5, 0.0], np.float32), True, grid, soup)
            log_two = restated.log32(np.array([2.0], np.float32))[0]
            fio.assert_bitwise(got['logits'], (pen + (S[:, 0] + np.float64(log_two))).astype(np.float32), f'M4, grid {grid.tolist()}')
            fio.assert_bitwise(got['alpha_mean'], np.full(len(pen), grid[0], np.float32), 'the mean of a value with itself')
            assert not got['alpha_index'].any()
    endless = check_designed(pools, True, np.array([-np.inf, 0.5, -np.inf], np.float32), np.array([0.5, 0.0, 0.25], np.float32),
                             'pair penalties of -inf', priors=('null', 'prior'))
    pool_of = np.arange(B) % 4
    b = int(np.flatnonzero(pool_of == 2)[0])
    row = endless['logits'][endless['row_ptr'][b]:endless['row_ptr'][b + 1]]
    assert np.isfinite(row[:16]).all() and (row[16:] == -np.inf).all() and len(row) == 136
    means = endless['alpha_mean'][endless['row_ptr'][b]:endless['row_ptr'][b + 1]]
    fio.assert_bitwise(means[16:], np.full(120, np.float32(0.75) / np.float32(3), np.float32), '-inf == -inf: every grid point counts once')


def test_null_outputs_are_honoured():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)
    G = prob.shape[1]
    pools, pool_of, penalty = [list(range(G)), [1, 3]], (np.arange(B) % 2).astype(np.int32), np.array([-0.5, 0.25], np.float32)
    full = marginal(ctx, pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS)
    assert full['profile'] is None and full['alpha_mean'].dtype == np.float32 and full['best_alpha_mean'].shape == (B,)
    lean = marginal(ctx, pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS, fetch_logits=False, fetch_probs=False, fetch_alpha_index=False,
                    fetch_alpha_mean=False)
    assert lean['logits'] is None and lean['probs'] is None and lean['alpha_index'] is None and lean['alpha_mean'] is None
    same_bytes(lean, full, ('best_option', 'best_prob', 'doublet_mass', 'best_alpha_index', 'best_alpha_mean', 'ambient'), 'without the compact outputs')
    only_means = marginal(ctx, pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS, fetch_logits=False, fetch_probs=False, fetch_alpha_index=False)
    fio.assert_bitwise(only_means['alpha_mean'], full['alpha_mean'], 'the means alone')
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    restated.assert_same(full, restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, soup, WEIGHTS), 'a fixture under a prior')
    with pytest.raises(ValueError, match="over_grid='max'"):
        marginal(ctx, pools, pool_of, True, penalty, GRID, fetch_profile=True)
    with pytest.raises(ValueError, match='log_weights'):
        ctx.estep_ambient_grid(pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, with_doublets, pool_start, donors, penalty, pool_of, row_ptr, alphas, ambient=None, weights=None, n_pools=None, n_alphas=None,
             B=None, V=None):
    """dmx_estep_ambient_grid_marginal with the arrays as given: (status, message, whether an output was written)."""
    from demuxalot_amd import _lib
    pool_start, donors = np.asarray(pool_start, np.int64), np.asarray(donors, np.int32)
    penalty, pool_of, row_ptr = np.asarray(penalty, np.float32), np.asarray(pool_of, np.int32), np.asarray(row_ptr, np.int64)
    alphas = None if alphas is None else np.asarray(alphas, np.float32)
    ambient = None if ambient is None else np.asarray(ambient, np.float32)
    weights = None if weights is None else np.asarray(weights, np.float32)
    B, V = ctx.B if B is None else B, ctx.V if V is None else V
    n = max(int(row_ptr.max(initial=0)), 0) + 1
    A = (0 if alphas is None else len(alphas)) if n_alphas is None else n_alphas
    outputs = [np.full(n, 7, np.float32), np.full(n, 7, np.float32), np.full(B, 7, np.int32), np.full(B, 7, np.float32), np.full(B, 7, np.float64),
               np.full(V, 7, np.float32), np.full(n, 7, np.int32), np.full(B, 7, np.int32), np.full(n, 7, np.float32), np.full(B, 7, np.float32)]
    status = ctx._lib.dmx_estep_ambient_grid_marginal(ctx._h, with_doublets, len(pool_start) - 1 if n_pools is None else n_pools, _lib.ptr(pool_start),
                                                      _lib.ptr(donors), _lib.ptr(penalty), _lib.ptr(pool_of), _lib.ptr(row_ptr),
                                                      *[_lib.ptr(o) for o in outputs[:5]], 0.01, 0.99, A, _lib.ptr(alphas), _lib.ptr(ambient),
                                                      *[_lib.ptr(o) for o in outputs[5:8]], _lib.ptr(weights), *[_lib.ptr(o) for o in outputs[8:]])
    return status, _lib.load().dmx_last_error().decode(), any((o != 7).any() for o in outputs)


def test_refusals_return_their_code_and_write_nothing():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)  # G = 5
    pools = [[0, 1], [1, 2, 4]]
    pool_of = np.where(np.arange(B) % 5 == 4, -1, np.arange(B) % 2).astype(np.int32)
    penalty = np.array([0.25, -0.5], np.float32)
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, soup, WEIGHTS)
    good = dict(with_doublets=1, pool_start=[0, 2, 5], donors=[0, 1, 1, 2, 4], penalty=penalty, pool_of=pool_of, row_ptr=want['row_ptr'], alphas=GRID,
                weights=WEIGHTS)
    status, _text, written = raw_call(ctx, **good)
    assert status == 0 and written
    cases = helpers.pool_refusal_cases(good, pool_of) + [
        (dict(with_doublets=0), DMX_ERR_INVALID, 'row_ptr'),  # (the rows were laid out for the pairs)
        (dict(alphas=[], weights=None), DMX_ERR_INVALID, 'at least one value'),
        (dict(n_alphas=0), DMX_ERR_INVALID, 'at least one value'),
        (dict(n_alphas=-3), DMX_ERR_INVALID, 'at least one value'),
        (dict(alphas=None, n_alphas=5), DMX_ERR_INVALID, 'null alphas'),
        (dict(alphas=np.linspace(0, 1, 65), weights=np.zeros(65)), DMX_ERR_UNSUPPORTED, 'more than 64 values'),
        (dict(alphas=None, n_alphas=65), DMX_ERR_UNSUPPORTED, 'more than 64 values'),
        (dict(alphas=at(GRID, 2, np.nan)), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=at(GRID, 4, 1.5)), DMX_ERR_INVALID, 'grid value'),
        (dict(ambient=at(soup, 3, np.nan)), DMX_ERR_INVALID, 'ambient value'),
        (dict(weights=at(WEIGHTS, 0, np.nan)), DMX_ERR_INVALID, 'log weight is not finite (index 0)'),
        (dict(weights=at(WEIGHTS, 4, -np.inf)), DMX_ERR_INVALID, 'log weight is not finite (index 4)'),
        (dict(weights=at(WEIGHTS, 2, np.inf)), DMX_ERR_INVALID, 'log weight is not finite (index 2)'),
        (dict(weights=at(WEIGHTS, 2, np.inf), alphas=at(GRID, 1, -0.1)), DMX_ERR_INVALID, 'grid value'),  # (the grid comes first)
    ]
    launches = ctx.timings()['estep']['launches']
    for change, code, message in cases:
        status, text, written = raw_call(ctx, **{**good, **change})
        assert status == code and message in text and 'dmx_estep_ambient_grid_marginal' in text, (change, status, text)
        assert not written, (change, 'a refused call writes nothing')
        assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    status, _text, written = raw_call(ctx, **{**good, 'alphas': np.linspace(1, 0, 64), 'weights': np.full(64, np.finfo(np.float32).min)})
    assert status == 0 and written, '64 values are the most; every finite weight is one'
    assert ctx.timings()['estep']['launches'] == launches + 1, 'the pass is counted as one E-step'
    from demuxalot_amd._lib import DemuxHipError
    with pytest.raises(DemuxHipError, match=r'log weight.*status -1'):
        marginal(ctx, pools, pool_of, True, penalty, GRID, log_weights=at(WEIGHTS, 1, np.nan))
    restated.assert_same(marginal(ctx, pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS), want, 'a valid call after the refused ones')


def test_more_than_1024_options_a_missing_table_and_a_communicator_are_refused():
    ctx, *_rest, B, _v2snp, _soup, _lengths = designed()
    status, text, written = raw_call(ctx, 1, [0, 45], np.arange(45), [0.0], np.zeros(B, np.int32), np.arange(B + 1) * 1035, [0.5], weights=[0.0])
    assert status == DMX_ERR_UNSUPPORTED and 'more than 1024 options' in text and 'dmx_estep_ambient_grid_marginal' in text and not written, (status, text)
    _v, _cb, _e, prob, B, _v2snp = profile_restated.fixture_problem('f3_small_0.npz')
    args = dict(with_doublets=1, pool_start=[0, 2], donors=[0, 1], penalty=[0.0], pool_of=np.zeros(B, np.int32), row_ptr=np.arange(B + 1) * 3,
                alphas=[0.25, 0.0], weights=[0.0, -1.0], B=B, V=len(prob))
    helpers.check_needs_problem_table_no_communicator(raw_call, 'dmx_estep_ambient_grid_marginal', args)


# ---- 4. the resident results of an E-step are none of this pass's business --------------------------------------------------------
def test_leaves_the_resident_results_alone():
    from oracle import demux_oracle
    ctx, v, cb, e, prob, B, v2snp = resident(F1)
    G = prob.shape[1]
    penalties = demux_oracle.doublet_penalties(G, 0.35)
    logits, probs = ctx.estep(penalties, True)
    pools, pool_of = [[0, 3, 5], list(range(G))], (np.arange(B) % 2).astype(np.int32)
    first = marginal(ctx, pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), GRID, log_weights=WEIGHTS)
    fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() after dmx_estep_ambient_grid_marginal')
    fio.assert_bitwise(ctx.get_logits(), logits, 'get_logits() after dmx_estep_ambient_grid_marginal')
    again = marginal(ctx, pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), GRID, log_weights=WEIGHTS)
    same_bytes(again, first, SHARED + ('ambient',) + restated.OWN, 'two runs')


# ---- 5. the front door (exact_mode: predict_posteriors in the exact arithmetic, what the new pass is compared with) ------------------
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_the_marginal_over_a_grid_of_zero_is_predict_posteriors(doublet_prior, exact_mode):
    from demuxalot_amd import Demultiplexer, JointAmbientPosteriors
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    plain_logits, plain_probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=doublet_prior)
    joint = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=[0.0], doublet_prior=doublet_prior, over_grid='marginal')
    assert isinstance(joint, JointAmbientPosteriors) and joint.profile is None and joint.over_grid == 'marginal'
    for frame, plain in ((joint.posteriors[0], plain_logits), (joint.posteriors[1], plain_probs)):
        assert list(frame.columns) == list(plain.columns) and list(frame.index) == handler.ordered_barcodes and frame.index.name == 'BARCODE'
        assert frame.values.dtype == np.float32 and list(frame.dtypes) == list(plain.dtypes)
        fio.assert_bitwise(frame.values, plain.values, f'doublet_prior {doublet_prior}')
    assert joint.option_alpha_means.shape == joint.option_alphas.shape and not joint.option_alpha_means.any()
    summary = joint.summary()
    assert list(summary.columns)[-1] == 'alpha_mean' and not summary['alpha_mean'].values.any()
    # a longer grid under a prior, against the restatement
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(F1)
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    want_logits, want_probs, want = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, GRID, soup, WEIGHTS)
    full = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, doublet_prior=doublet_prior, over_grid='marginal',
                                                          alpha_log_weights=WEIGHTS)
    fio.assert_bitwise(full.posteriors[0].values, want_logits, 'five grid values: logits')
    fio.assert_bitwise(full.posteriors[1].values, want_probs, 'five grid values: posteriors')
    assert np.array_equal(full.alpha_index, want['alpha_index']) and np.array_equal(full.best_alpha_index, want['best_alpha_index'])
    fio.assert_bitwise(full.option_alpha_means, want['alpha_mean'].astype(np.float64), 'five grid values: the means')
    fio.assert_bitwise(full.summary()['alpha_mean'].values, want['best_alpha_mean'].astype(np.float64), 'five grid values: the summary')
    with pytest.raises(ValueError, match="over_grid='max'"):
        Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, over_grid='marginal', keep_profile=True)


def test_the_default_is_the_max_mode_byte_for_byte():
    from demuxalot_amd import Demultiplexer
    fx = fio.load(F2)
    calls, genotypes, handler = fio.product_inputs(fx)
    default = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, keep_profile=True)
    named = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, keep_profile=True, over_grid='max')
    assert default.over_grid == named.over_grid == 'max' and default.option_alpha_means is None and named.option_alpha_means is None
    for one, other in zip(default.posteriors, named.posteriors):
        assert list(one.columns) == list(other.columns) and list(one.index) == list(other.index) and list(one.dtypes) == list(other.dtypes)
        assert one.values.tobytes() == other.values.tobytes()
    for key in ('alpha_index', 'best_alpha_index', 'best_option', 'best_prob', 'doublet_mass', 'profile', 'ambient', 'alphas'):
        assert getattr(default, key).tobytes() == getattr(named, key).tobytes(), key
    assert list(default.summary().columns) == list(named.summary().columns) == ['option', 'probability', 'alpha', 'doublet_probability', 'at_grid_edge']
    other = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, over_grid='marginal')
    assert (other.posteriors[0].values != default.posteriors[0].values).any()


@pytest.mark.parametrize('calls_per_barcode', [256, 64])
def test_the_marginal_on_the_simulation_with_true_doublets(calls_per_barcode):
    from demuxalot_amd import Demultiplexer
    sim, want_max, want = restated.simulated(calls_per_barcode)
    calls, genotypes, handler = helpers.user_inputs(sim, helpers.table_betas(sim), default_prior=1.0)
    counts = {}
    for mode in ('max', 'marginal'):
        joint = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, doublet_prior=0.35, over_grid=mode)
        summary = joint.summary()
        counts[mode] = restated.counts_of(sim, summary['doublet_probability'].values, joint.posteriors[1].values.argmax(axis=1))
        assert ('alpha_mean' in summary.columns) == (mode == 'marginal')
    # (the front door's table is probs_from_betas of the betas above, the simulation's own probabilities only up to the prior: the
    # counts are the restatement's, the bits are the designed problems' and the fixtures' above)
    assert counts['max'] == restated.counts_of(sim, want_max['doublet_mass'], want_max['best_option']), counts
    assert counts['marginal'] == restated.counts_of(sim, want['doublet_mass'], want['best_option']), counts
    restated.marginal_conditions(calls_per_barcode, sim, counts['max'], counts['marginal'])
    assert ((joint.option_alpha_means >= 0) & (joint.option_alpha_means <= np.float64(restated.DEFAULT_GRID.max()))).all()
