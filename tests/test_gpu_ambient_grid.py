"""Every option at its own best ambient fraction on the GPU (include/demux_hip_debug.h: dmx_estep_ambient_grid;
csrc/estep_ambient_grid.hip; Demultiplexer.predict_posteriors_joint_ambient).

The pass has no tolerance arithmetic: everything is compared bit for bit.  The checkers are the passes it is built from - with one
grid value it is dmx_estep_ambient with that fraction everywhere (G1), every column of its profile is dmx_estep_ambient's logits at
that grid value (G2), an option with penalty 0 is dmx_ambient_profile's row and best (G3) - and tests/ambient_grid_restatement.py,
pinned to the reference in tests/test_ambient_grid_cpu.py.  The shapes are the smallest at which the kernels can go wrong: option
counts on either side of every slot boundary, grid lengths on either side of the grid points a form takes per walk (4, 2 and 1),
rows on either side of the 8-call padding, pools of several buckets and barcodes in no pool in one call, barcodes without calls."""
import functools

import numpy as np
import pytest

from tests import ambient_grid_restatement as restated
from tests import ambient_restatement as profile_restated
from tests import ambient_scoring_restatement as scoring_restated
from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests import pools_restatement
from tests.pooled_helpers import at, designed_grid, exact_mode, same_bytes, spread_columns  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1, F2, SMALL = helpers.F1, helpers.F2, helpers.F3_SMALL[2]  # G = 20, 4, 5
GRID = np.array([0.0, 1.0, 0.01, 0.37, 0.63], dtype=np.float32)
SHARED = ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass')
POINTS_PER_WALK = (4, 2, 1)  # csrc/estep_grid_device.h: GridPoints - by option slots 1, 2, 4 and more
resident = functools.lru_cache(maxsize=None)(helpers.new_resident)  # (ctx, v, cb, e, prob, B, v2snp), the contexts this module's own


# ---- 1. G1: one grid value is dmx_estep_ambient with that fraction for every barcode ---------------------------------------------
@pytest.mark.parametrize('name', [F1, F2])
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_one_grid_value_is_the_pass_with_that_fraction_everywhere(name, doublet_prior):
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    penalty = np.array([scoring_restated.demux_oracle.doublet_penalties(G, doublet_prior)[-1]], np.float32)
    other = np.random.default_rng(1).uniform(0, 1, size=len(v2snp)).astype(np.float32)
    for value in (0.0, -0.0, 0.37):
        for ambient in (None, other):
            want = ctx.estep_ambient(pools, pool_of, doublet_prior != 0, penalty, np.full(B, value, np.float32), ambient=ambient)
            got = ctx.estep_ambient_grid(pools, pool_of, doublet_prior != 0, penalty, [value], ambient=ambient, fetch_profile=True)
            same_bytes(got, want, SHARED + ('ambient',), f'{name} {doublet_prior} alpha {value}')
            assert not got['alpha_index'].any() and not got['best_alpha_index'].any()
            fio.assert_bitwise(np.ascontiguousarray(got['profile'][:, 0]), got['logits'], 'the one column of the profile')
    # ... at 0 that is the pooled pass, and through it the reference's own posteriors
    plain = ctx.estep_pools(pools, pool_of, doublet_prior != 0, penalty)
    same_bytes(ctx.estep_ambient_grid(pools, pool_of, doublet_prior != 0, penalty, [0.0]), plain, SHARED, f'{name} {doublet_prior}: alphas = {{0}}')
    reference = pools_restatement.Restatement(v, cb, e, prob, B, doublet_prior)
    pools_restatement.assert_same(plain, reference(pools, pool_of), f'{name} {doublet_prior}: the pooled pass')


# ---- 2. G2 / G3: the profile's columns and rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [F2, F1])
def test_profile_columns_are_the_scoring_pass_and_rows_the_ambient_profile(name):
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    pools = [list(range(G)), [0, 2, 3], [1]]
    pool_of = np.where(np.arange(B) % 7 == 6, -1, np.arange(B) % 3).astype(np.int32)
    penalty = np.array([-0.75, 0.5, 0.0], dtype=np.float32)
    got = ctx.estep_ambient_grid(pools, pool_of, True, penalty, GRID, fetch_profile=True)
    assert got['profile'].shape == (got['row_ptr'][-1], len(GRID)) and got['profile'].dtype == np.float32
    for j, value in enumerate(GRID):  # G2
        column = ctx.estep_ambient(pools, pool_of, True, penalty, np.full(B, value, np.float32))
        fio.assert_bitwise(np.ascontiguousarray(got['profile'][:, j]), column['logits'], f'{name}: column {j}')
        fio.assert_bitwise(got['ambient'], column['ambient'], 'the same derived profile')
    index, value = profile_restated.first_maximum(got['profile'])
    assert np.array_equal(got['alpha_index'], index), 'the first maximum of the stored values'
    fio.assert_bitwise(got['logits'], value, 'the logit is the stored value at its grid point')
    # G3: one pool of everybody, penalty 0 - option k of every barcode is dmx_ambient_profile's row for k's donors
    everybody = ctx.estep_ambient_grid([list(range(G))], np.zeros(B, np.int32), True, np.zeros(1, np.float32), GRID, fetch_profile=True)
    d1, d2 = scoring_restated.pool_options(list(range(G)), True)
    K = len(d1)
    cube, chosen, logits = everybody['profile'].reshape(B, K, len(GRID)), everybody['alpha_index'].reshape(B, K), everybody['logits'].reshape(B, K)
    rows = np.arange(B)
    for shift in range(0, K, 1 if K <= 16 else 11):  # every barcode with another option per call; (barcode, option) pairs all over the triangle
        k = (rows + shift) % K
        donor1, donor2 = d1[k].astype(np.int32), np.where(d1[k] == d2[k], -1, d2[k]).astype(np.int32)
        profile = ctx.ambient_profile(donor1, donor2, GRID)
        fio.assert_bitwise(np.ascontiguousarray(cube[rows, k, :]), profile['loglik'], f'{name}: shift {shift}')
        assert np.array_equal(chosen[rows, k], profile['best']), f'{name}: shift {shift}: best'
        fio.assert_bitwise(np.ascontiguousarray(logits[rows, k]), profile['ll_best'], f'{name}: shift {shift}: the value there')


# ---- 3. kernel-shape edges ------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129]  # calls of a barcode: either side of the 8-call padding and of the 64-call chunk
NARROW_SINGLETS, NARROW_DOUBLETS = [1, 63, 64, 65], [1, 2, 10, 11]  # options 1, 63, 64 | 65 and 1, 3, 55 | 66: one slot, two slots
WIDE_SINGLETS = [128, 129, 256, 257, 512, 513, 1024]  # options of a pool without doublets: either side of every further slot boundary
WIDE_DOUBLETS = [16, 22, 23, 31, 32, 44]  # donors: 136, 253 | 276, 496 | 528, 990 options
GRID_LENGTHS = sorted({1, 2, 63, 64} | set(POINTS_PER_WALK) | {J + 1 for J in POINTS_PER_WALK})


DESIGNED = dict(lengths=LENGTHS, V=160, B=12 * len(LENGTHS), seed=11)


@functools.lru_cache(maxsize=None)
def designed():
    """144 barcodes, barcode i with LENGTHS[i % 12] calls, on 1024 donors and 80 biallelic SNPs; error probabilities at both ends of
    their range among them.  Group i // 12 of the barcodes is what the tests put into one pool (or into none)."""
    return helpers.install_arrays(*helpers.designed_arrays(**DESIGNED))


def check_designed(pools, with_doublets, penalty, grid, what, derived=False):
    ctx, v, cb, e, prob, B, v2snp, soup, lengths = designed()
    group = np.arange(B) // len(LENGTHS)
    pool_of = np.where(group < len(pools), group, -1).astype(np.int32)
    assert (pool_of < 0).any(), 'barcodes in no pool'
    profile = profile_restated.derived_ambient(v, v2snp, 0.01) if derived else soup
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, with_doublets, grid, profile)
    got = ctx.estep_ambient_grid(pools, pool_of, with_doublets, penalty, grid, ambient=None if derived else soup, fetch_profile=True)
    restated.assert_same(got, want, what)
    none = pool_of < 0
    assert (got['best_option'][none] == -1).all() and np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all()
    assert (got['best_alpha_index'][none] == -1).all()
    # best_alpha_index is alpha_index at the best option
    some = got['best_option'] >= 0
    assert np.array_equal(got['best_alpha_index'][some], got['alpha_index'][got['row_ptr'][:-1][some] + got['best_option'][some]])
    # barcodes without calls: logits = penalties at every grid point, so the first point wins
    assert ((lengths == 0) & ~none).any()
    for b in np.flatnonzero((lengths == 0) & ~none):
        p = pool_of[b]
        row = slice(got['row_ptr'][b], got['row_ptr'][b + 1])
        pen = np.zeros(row.stop - row.start, np.float32)
        pen[len(pools[p]):] = penalty[p]
        fio.assert_bitwise(got['logits'][row], pen, f'{what}: barcode {b} without calls')
        assert not got['alpha_index'][row].any() and got['best_alpha_index'][b] == 0
        fio.assert_bitwise(got['profile'][row], np.repeat(pen[:, None], len(grid), axis=1), f'{what}: barcode {b} without calls, the profile')
    # the form without the profile is another kernel: the same results; null outputs are honoured
    lean = ctx.estep_ambient_grid(pools, pool_of, with_doublets, penalty, grid, ambient=None if derived else soup)
    assert lean['profile'] is None
    same_bytes(lean, got, SHARED + ('ambient', 'alpha_index', 'best_alpha_index'), f'{what}: without the profile')
    return got, pool_of


@pytest.mark.parametrize('n_alphas', GRID_LENGTHS)
def test_narrow_pools_with_grids_on_either_side_of_the_points_per_walk(n_alphas):
    assert GRID_LENGTHS == [1, 2, 3, 4, 5, 63, 64]
    grid = designed_grid(n_alphas)
    if n_alphas >= 3:
        assert 0.0 in grid and 1.0 in grid and len(set(grid.tolist())) < n_alphas and (np.diff(grid) < 0).any()
    rng = np.random.default_rng(3)
    singlets = [spread_columns(rng, K, 1024) for K in NARROW_SINGLETS]
    check_designed(singlets, False, np.linspace(-1, 1, len(singlets)).astype(np.float32), grid, f'singlet pools, {n_alphas} grid values',
                   derived=n_alphas == 5)
    doublets = [spread_columns(rng, g, 1024) for g in NARROW_DOUBLETS]
    assert [g * (g + 1) // 2 for g in NARROW_DOUBLETS] == [1, 3, 55, 66]
    got, pool_of = check_designed(doublets, True, np.linspace(-2, 1.5, len(doublets)).astype(np.float32), grid, f'doublet pools, {n_alphas} grid values',
                                  derived=n_alphas == 4)
    if n_alphas >= 4:
        assert len(set(got['alpha_index'].tolist())) > 1, 'the options do not all choose the same grid point'


def test_wide_singlet_pools_on_either_side_of_every_slot_boundary():
    rng = np.random.default_rng(3)
    pools = [spread_columns(rng, K, 1024) for K in WIDE_SINGLETS]
    assert pools[-1] == list(range(1024))
    grid = np.array([0.37, 0.0, 1.0], dtype=np.float32)
    check_designed(pools, False, np.linspace(-1, 1, len(pools)).astype(np.float32), grid, 'wide singlet pools')


def test_wide_doublet_pools_of_every_bucket():
    rng = np.random.default_rng(4)
    pools = [spread_columns(rng, g, 1024) for g in WIDE_DOUBLETS]
    assert [g * (g + 1) // 2 for g in WIDE_DOUBLETS] == [136, 253, 276, 496, 528, 990]
    grid = np.array([0.63, 0.0, 0.63], dtype=np.float32)
    check_designed(pools, True, np.linspace(-2, 1.5, len(pools)).astype(np.float32), grid, 'wide doublet pools', derived=True)


def test_null_outputs_are_honoured():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)
    G = prob.shape[1]
    pools, pool_of, penalty = [list(range(G)), [1, 3]], (np.arange(B) % 2).astype(np.int32), np.array([-0.5, 0.25], np.float32)
    full = ctx.estep_ambient_grid(pools, pool_of, True, penalty, GRID, fetch_profile=True)
    lean = ctx.estep_ambient_grid(pools, pool_of, True, penalty, GRID, fetch_logits=False, fetch_probs=False, fetch_alpha_index=False)
    assert lean['logits'] is None and lean['probs'] is None and lean['alpha_index'] is None and lean['profile'] is None
    same_bytes(lean, full, ('best_option', 'best_prob', 'doublet_mass', 'best_alpha_index', 'ambient'), 'without the compact outputs')
    only_profile = ctx.estep_ambient_grid(pools, pool_of, True, penalty, GRID, fetch_logits=False, fetch_probs=False, fetch_alpha_index=False,
                                          fetch_profile=True)
    fio.assert_bitwise(only_profile['profile'], full['profile'], 'the profile alone')


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def raw_call(ctx, with_doublets, pool_start, donors, penalty, pool_of, row_ptr, alphas, ambient=None, n_pools=None, n_alphas=None, B=None, V=None):
    """dmx_estep_ambient_grid with the arrays as given: (status, message, whether an output was written)."""
    from demuxalot_amd import _lib
    pool_start, donors = np.asarray(pool_start, np.int64), np.asarray(donors, np.int32)
    penalty, pool_of, row_ptr = np.asarray(penalty, np.float32), np.asarray(pool_of, np.int32), np.asarray(row_ptr, np.int64)
    alphas = None if alphas is None else np.asarray(alphas, np.float32)
    ambient = None if ambient is None else np.asarray(ambient, np.float32)
    B, V = ctx.B if B is None else B, ctx.V if V is None else V
    n = max(int(row_ptr.max(initial=0)), 0) + 1
    A = (0 if alphas is None else len(alphas)) if n_alphas is None else n_alphas
    outputs = [np.full(n, 7, np.float32), np.full(n, 7, np.float32), np.full(B, 7, np.int32), np.full(B, 7, np.float32), np.full(B, 7, np.float64),
               np.full(V, 7, np.float32), np.full(n, 7, np.int32), np.full(B, 7, np.int32), np.full(n * min(max(A, 1), 64), 7, np.float32)]
    status = ctx._lib.dmx_estep_ambient_grid(ctx._h, with_doublets, len(pool_start) - 1 if n_pools is None else n_pools, _lib.ptr(pool_start),
                                             _lib.ptr(donors), _lib.ptr(penalty), _lib.ptr(pool_of), _lib.ptr(row_ptr), *[_lib.ptr(o) for o in outputs[:5]],
                                             0.01, 0.99, A, _lib.ptr(alphas), _lib.ptr(ambient), *[_lib.ptr(o) for o in outputs[5:]])
    return status, _lib.load().dmx_last_error().decode(), any((o != 7).any() for o in outputs)


def test_refusals_return_their_code_and_write_nothing():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)  # G = 5
    pools = [[0, 1], [1, 2, 4]]
    pool_of = np.where(np.arange(B) % 5 == 4, -1, np.arange(B) % 2).astype(np.int32)
    penalty = np.array([0.25, -0.5], np.float32)
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, soup)
    good = dict(with_doublets=1, pool_start=[0, 2, 5], donors=[0, 1, 1, 2, 4], penalty=penalty, pool_of=pool_of, row_ptr=want['row_ptr'], alphas=GRID)
    status, _text, written = raw_call(ctx, **good)
    assert status == 0 and written
    cases = helpers.pool_refusal_cases(good, pool_of) + [
        (dict(with_doublets=0), DMX_ERR_INVALID, 'row_ptr'),  # (the rows were laid out for the pairs)
        (dict(alphas=[]), DMX_ERR_INVALID, 'at least one value'),
        (dict(n_alphas=0), DMX_ERR_INVALID, 'at least one value'),
        (dict(n_alphas=-3), DMX_ERR_INVALID, 'at least one value'),
        (dict(alphas=None, n_alphas=5), DMX_ERR_INVALID, 'null alphas'),
        (dict(alphas=np.linspace(0, 1, 65)), DMX_ERR_UNSUPPORTED, 'more than 64 values'),
        (dict(alphas=None, n_alphas=65), DMX_ERR_UNSUPPORTED, 'more than 64 values'),
        (dict(alphas=at(GRID, 2, np.nan)), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=at(GRID, 0, np.inf)), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=at(GRID, 4, 1.5)), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=at(GRID, 1, -0.1)), DMX_ERR_INVALID, 'grid value'),
        (dict(ambient=at(soup, 3, np.nan)), DMX_ERR_INVALID, 'ambient value'),
        (dict(ambient=at(soup, len(soup) - 1, 2.0)), DMX_ERR_INVALID, 'ambient value'),
    ]
    launches = ctx.timings()['estep']['launches']
    for change, code, message in cases:
        status, text, written = raw_call(ctx, **{**good, **change})
        assert status == code and message in text and 'dmx_estep_ambient_grid' in text, (change, status, text)
        assert not written, (change, 'a refused call writes nothing')
        assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    status, _text, written = raw_call(ctx, **{**good, 'alphas': np.linspace(1, 0, 64)})
    assert status == 0 and written, '64 values are the most'
    assert ctx.timings()['estep']['launches'] == launches + 1, 'the pass is counted as one E-step'
    from demuxalot_amd._lib import DemuxHipError
    with pytest.raises(DemuxHipError, match=r'grid value.*status -1'):
        ctx.estep_ambient_grid(pools, pool_of, True, penalty, at(GRID, 0, 2.0))
    restated.assert_same(ctx.estep_ambient_grid(pools, pool_of, True, penalty, GRID, fetch_profile=True), want, 'a valid call after the refused ones')


def test_more_than_1024_options_are_refused():
    ctx, *_rest, B, _v2snp, _soup, _lengths = designed()
    # 45 donors with doublets: 1035 options (the table has 1024 columns: 1025 singlets are the CPU walk's)
    status, text, written = raw_call(ctx, 1, [0, 45], np.arange(45), [0.0], np.zeros(B, np.int32), np.arange(B + 1) * 1035, [0.5])
    assert status == DMX_ERR_UNSUPPORTED and 'more than 1024 options' in text and 'dmx_estep_ambient_grid' in text and not written, (status, text)


def test_needs_a_problem_a_table_and_no_communicator():
    _v, _cb, _e, prob, B, _v2snp = profile_restated.fixture_problem('f3_small_0.npz')
    args = dict(with_doublets=1, pool_start=[0, 2], donors=[0, 1], penalty=[0.0], pool_of=np.zeros(B, np.int32), row_ptr=np.arange(B + 1) * 3,
                alphas=[0.25, 0.0], B=B, V=len(prob))
    helpers.check_needs_problem_table_no_communicator(raw_call, 'dmx_estep_ambient_grid', args)


# ---- 5. the resident results of an E-step are none of this pass's business ------------------------------------------------------
def test_leaves_the_resident_results_alone():
    ctx, v, cb, e, prob, B, v2snp = resident(F1)
    G = prob.shape[1]
    penalties = scoring_restated.demux_oracle.doublet_penalties(G, 0.35)
    logits, probs = ctx.estep(penalties, True)
    pools, pool_of = [[0, 3, 5], list(range(G))], (np.arange(B) % 2).astype(np.int32)
    first = ctx.estep_ambient_grid(pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), GRID, fetch_profile=True)
    fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() after dmx_estep_ambient_grid')
    fio.assert_bitwise(ctx.get_logits(), logits, 'get_logits() after dmx_estep_ambient_grid')
    again = ctx.estep_ambient_grid(pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), GRID, fetch_profile=True)
    same_bytes(again, first, SHARED + ('ambient', 'alpha_index', 'best_alpha_index', 'profile'), 'two runs')


# ---- 6. the front door (exact_mode: predict_posteriors in the exact arithmetic, what the new pass is compared with) --------------
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_a_grid_of_zero_is_predict_posteriors(doublet_prior, exact_mode):
    from demuxalot_amd import Demultiplexer, JointAmbientPosteriors
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    barcodes = handler.ordered_barcodes
    plain_logits, plain_probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=doublet_prior)
    joint = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=[0.0], doublet_prior=doublet_prior)
    assert isinstance(joint, JointAmbientPosteriors) and joint.profile is None
    logits, probs = joint.posteriors
    for frame, plain in ((logits, plain_logits), (probs, plain_probs)):
        assert list(frame.columns) == list(plain.columns) and list(frame.index) == barcodes and frame.index.name == 'BARCODE'
        assert frame.values.dtype == np.float32 and list(frame.dtypes) == list(plain.dtypes)
        fio.assert_bitwise(frame.values, plain.values, f'doublet_prior {doublet_prior}')
    assert not np.isnan(joint.option_alphas).any() and not joint.option_alphas.any()
    summary = joint.summary()
    assert list(summary['option']) == list(plain_probs.idxmax(axis=1))
    # predict_posteriors afterwards, on the same context: unchanged
    after_logits, after_probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=doublet_prior)
    fio.assert_bitwise(after_logits.values, plain_logits.values, 'predict_posteriors after the joint pass: logits')
    fio.assert_bitwise(after_probs.values, plain_probs.values, 'predict_posteriors after the joint pass: posteriors')
    # a longer grid against the restatement, with the profile kept (the default grid: the simulation below)
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(F1)
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    want_logits, want_probs, want = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, GRID, soup)
    full = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, doublet_prior=doublet_prior, keep_profile=True)
    fio.assert_bitwise(full.posteriors[0].values, want_logits, 'five grid values: logits')
    fio.assert_bitwise(full.posteriors[1].values, want_probs, 'five grid values: posteriors')
    fio.assert_bitwise(full.profile, want['profile'], 'five grid values: the profile')
    assert np.array_equal(full.alpha_index, want['alpha_index']) and np.array_equal(full.best_alpha_index, want['best_alpha_index'])
    fio.assert_bitwise(full.alphas, GRID, 'the grid')
    assert (full.posteriors[0].values != plain_logits.values).any()


def test_joint_posteriors_in_pools():
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    name = 'f6_shipped_example.npz'
    fx = fio.load(name)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    B = len(barcodes)
    pool2donors = {'A': [donors[1], donors[0]], 'B': [donors[3], donors[1], donors[2]]}  # (any order)
    barcode2pool = {bc: (None if i % 5 == 4 else 'AB'[i % 2]) for i, bc in enumerate(barcodes)}
    joint = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=GRID, doublet_prior=0.35, barcode2pool=barcode2pool,
                                                           pool2donors=pool2donors)
    pooled = joint.posteriors
    assert isinstance(pooled, PooledPosteriors) and pooled.pools == ['A', 'B']
    v, cb, e, prob, n, v2snp = profile_restated.fixture_problem(name)
    assert n == B
    pools = [[0, 1], [1, 2, 3]]
    pool_of = np.array([-1 if i % 5 == 4 else i % 2 for i in range(B)], np.int32)
    penalty = pools_restatement.Restatement(v, cb, e, prob, B, 0.35).pair_penalty(pools)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, profile_restated.derived_ambient(v, v2snp, 0.01))
    raw = dict(row_ptr=pooled.row_ptr, logits=pooled.logits, probs=pooled.probs, best_option=pooled.best_option, best_prob=pooled.best_prob,
               doublet_mass=pooled.doublet_mass, ambient=joint.ambient, alpha_index=joint.alpha_index, best_alpha_index=joint.best_alpha_index)
    restated.assert_same(raw, want, 'pools end to end')
    for p, pool in enumerate('AB'):  # the frames of a pool are the restatement's rows of its barcodes
        logits_df, probs_df = pooled.to_dataframes(pool)
        rows = np.flatnonzero(pool_of == p)
        K = logits_df.shape[1]
        take = (want['row_ptr'][rows][:, None] + np.arange(K)[None, :]).reshape(-1)
        fio.assert_bitwise(logits_df.values, want['logits'][take].reshape(len(rows), K), f'pool {pool}: logits frame')
        fio.assert_bitwise(probs_df.values, want['probs'][take].reshape(len(rows), K), f'pool {pool}: posteriors frame')
        assert list(logits_df.index) == [barcodes[i] for i in rows]
    assert list(pooled.to_dataframes('B')[0].columns) == scoring_restated.demux_oracle.option_names([donors[g] for g in pools[1]], 0.35)
    summary = joint.summary()
    assert summary['option'].isna().values.tolist() == (pool_of < 0).tolist()
    grid_values = np.where(want['best_alpha_index'] >= 0, GRID[np.maximum(want['best_alpha_index'], 0)].astype(np.float64), np.nan)
    assert np.array_equal(np.isnan(summary['alpha'].values), np.isnan(grid_values))
    assert np.array_equal(summary['alpha'].values[pool_of >= 0], grid_values[pool_of >= 0])


@pytest.mark.parametrize('calls_per_barcode', [256, 64])
def test_joint_posteriors_on_the_simulation_with_true_doublets(calls_per_barcode):
    from demuxalot_amd import Demultiplexer
    sim, want = restated.simulated(calls_per_barcode)  # (genotypes whose betas are the allele probabilities times 1000)
    calls, genotypes, handler = helpers.user_inputs(sim, helpers.table_betas(sim), default_prior=1.0)
    joint = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, doublet_prior=0.35)
    logits, probs = joint.posteriors
    G, B = sim['prob'].shape[1], sim['B']
    assert logits.shape == probs.shape == (B, G * (G + 1) // 2) and probs.values.dtype == np.float32
    summary = joint.summary()
    # the conditions of the CPU test, on what the device computed
    restated.joint_conditions(calls_per_barcode, sim, summary['doublet_probability'].values, probs.values.argmax(axis=1), summary['alpha'].values)
    names = list(probs.columns)
    assert list(summary['option']) == [names[k] for k in joint.best_option]
    # (no bits against the restatement here: the front door's table is probs_from_betas of the betas above, the simulation's own
    # probabilities only up to the prior; the bits are the designed problems' and the fixtures' above)
    assert want['logits'].shape == (logits.size,)
    fio.assert_bitwise(joint.alphas, restated.DEFAULT_GRID, 'the default grid')
    assert joint.option_alphas.shape == (B * G * (G + 1) // 2,) and not np.isnan(joint.option_alphas).any()
