"""Doublets over a grid of mixing shares, on the GPU (include/demux_hip_debug.h: dmx_estep_pair_shares; csrc/estep_pair_shares.hip;
Demultiplexer.predict_posteriors_with_doublet_shares).

No tolerances: everything is compared bit for bit with tests/pair_shares_restatement.py (pinned on the CPU in
tests/test_pair_shares_cpu.py) and with the pooled pass through the identities S1 .. S5.  The shapes are the smallest at which the kernels
can go wrong: pools on either side of every slot boundary, so that all five forms run, grid lengths on either side of the grid points a
form takes per walk, unsorted grids with duplicates and both ends, a barcode without calls, barcodes in no pool."""
import functools

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pair_shares_restatement as restated
from tests import pooled_helpers as helpers
from tests import pools_restatement
from tests.pooled_helpers import at, exact_mode, same_bytes, spread_columns  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1, F2, SMALL = helpers.F1, helpers.F2, helpers.F3_SMALL[2]  # G = 20, 4, 5
SHARED, OWN = restated.SHARED, restated.OWN
GRID = np.array([1.0, 0.0, 0.2, 0.63, 0.2], dtype=np.float32)
WEIGHTS = np.array([-0.5, -7.0, 0.25, -1.0, -2.5], dtype=np.float32)
resident = functools.lru_cache(maxsize=None)(helpers.new_resident)  # (ctx, v, cb, e, prob, B, v2snp), the contexts this module's own


# ---- 1. S1 and S2 on the fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [F1, F2])
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_s1_s2_the_one_share_of_a_half_is_the_pooled_pass(name, doublet_prior):
    from oracle import demux_oracle
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    assert prob[prob != 0].min() >= 2.0 ** -125
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    penalty = np.array([demux_oracle.doublet_penalties(G, doublet_prior)[-1]], np.float32)
    pooled = ctx.estep_pools(pools, pool_of, doublet_prior != 0, penalty)
    for weights in (None, [0.0]):
        got = ctx.estep_pair_shares(pools, pool_of, doublet_prior != 0, penalty, [0.5], log_weights=weights)
        same_bytes(got, pooled, SHARED, f'{name} {doublet_prior}: the pooled pass')
        assert not np.isnan(got['logits']).any()
        single = np.tile(np.arange(len(got['logits']) // B) < G, B)
        fio.assert_bitwise(got['share_mean'][~single], np.full(int((~single).sum()), 0.5, np.float32), 'share_mean is the one share')
        assert not got['share_index'][~single].any() and (got['share_index'][single] == -1).all() and np.isnan(got['share_mean'][single]).all()
    if doublet_prior == 0:  # S2: any grid, any weights
        got = ctx.estep_pair_shares(pools, pool_of, False, penalty, GRID, log_weights=WEIGHTS)
        same_bytes(got, pooled, SHARED, f'{name}: without doublets')
        assert (got['share_index'] == -1).all() and np.isnan(got['share_mean']).all()
        assert (got['best_share_index'] == -1).all() and np.isnan(got['best_share_mean']).all()


# ---- 2. the designed problem ------------------------------------------------------------------------------------------------------------
LENGTHS = restated.DESIGNED_LENGTHS  # calls of a barcode: none, either side of the 8-call padding
ONE_SLOT, TWO_SLOTS, WIDE = [2, 10], [11, 15], [16, 22, 23, 31, 32, 44]


@functools.lru_cache(maxsize=None)
def designed():
    """48 barcodes, barcode i with LENGTHS[i % 12] calls (barcode 0 has none), on 1024 donors and 24 biallelic SNPs (48 variants);
    error probabilities at both ends of their range and table entries of exactly 0 and 1 among them."""
    from demuxalot_amd.device import DeviceContext
    v, cb, e, prob, B, lengths, v2snp = restated.designed_problem()  # (the CPU tests walk the same problem)
    ctx = DeviceContext(0)
    ctx.set_problem(B, prob.shape[0], prob.shape[1], v, cb, e, v2snp)
    ctx.set_probs(prob)
    return ctx, v, cb, e, prob, B, lengths


designed_grid = functools.partial(helpers.designed_grid, seed_base=300)  # n shares: a draw of its own, apart from the ambient grids'


def steep_weights(n):
    """A non-uniform prior in logs: both signs, a value that all but removes its grid point."""
    weights = np.random.default_rng(400 + n).uniform(-3, 1, size=n).astype(np.float32)
    weights[n // 2] = -60.0
    return weights


def designed_pools(sizes, seed):
    """(pools, pool_of): barcode i in pool i % (n + 1), the last class in no pool; the barcode without calls is in pool 0."""
    rng = np.random.default_rng(seed)
    pools = [spread_columns(rng, g) for g in sizes]
    B = designed()[5]
    pool_of = (np.arange(B) % (len(pools) + 1)).astype(np.int32)
    pool_of[pool_of == len(pools)] = -1
    assert (pool_of < 0).any() and pool_of[0] == 0
    return pools, pool_of


def check_designed(sizes, seed, penalty, grid, what, priors=('null', 'zeros', 'steep')):
    """The device against the restatement under each prior, and S5; returns the call without a prior."""
    ctx, v, cb, e, prob, B, lengths = designed()
    pools, pool_of = designed_pools(sizes, seed)
    penalty = np.asarray(penalty, np.float32)
    plain = None
    for prior in priors:
        weights = {'null': None, 'zeros': np.zeros(len(grid), np.float32), 'steep': steep_weights(len(grid))}[prior]
        got = ctx.estep_pair_shares(pools, pool_of, True, penalty, grid, log_weights=weights)
        if prior == 'zeros' and plain is not None:  # S5
            same_bytes(got, plain, SHARED + OWN, f'{what}: zeros are no weights')
            continue
        want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, grid, weights)
        restated.assert_same(got, want, f'{what}, {prior}')
        none = pool_of < 0
        assert (got['best_option'][none] == -1).all() and np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all()
        assert (got['best_share_index'][none] == -1).all() and np.isnan(got['best_share_mean'][none]).all()
        if prior == 'null':
            plain = got
    return plain


@pytest.mark.parametrize('n_shares', [1, 3, 4, 5, 8, 9])
def test_one_slot_pools_with_grids_around_the_four_points_per_walk(n_shares):
    assert [g * (g + 1) // 2 for g in ONE_SLOT] == [3, 55]
    check_designed(ONE_SLOT, 3, [-2.0, 1.5], designed_grid(n_shares), f'one-slot pools, {n_shares} shares')


@pytest.mark.parametrize('n_shares', [1, 2, 3])
def test_two_slot_pools_with_grids_around_the_two_points_per_walk(n_shares):
    assert [g * (g + 1) // 2 for g in TWO_SLOTS] == [66, 120]
    check_designed(TWO_SLOTS, 5, [-2.0, 1.5], designed_grid(n_shares), f'two-slot pools, {n_shares} shares')


def test_wide_pools_of_every_bucket():
    assert [g * (g + 1) // 2 for g in WIDE] == [136, 253, 276, 496, 528, 990]
    grid = np.array([0.63, 1.0, 0.0, 0.63], dtype=np.float32)
    check_designed(WIDE, 4, np.linspace(-2, 1.5, len(WIDE)), grid, 'wide pools')
    check_designed(WIDE[:2], 7, [0.5, -0.5], grid[:1], 'wide pools, one share', priors=('null',))


def test_a_grid_of_64_shares_on_pools_of_several_forms():
    check_designed([2, 10, 11, 16], 6, [0.5, -0.5, 1.0, -1.0], designed_grid(64), '64 shares', priors=('null', 'steep'))
    ctx, v, cb, e, prob, B, lengths = designed()
    pools, pool_of = designed_pools([10, 16], 9)
    weights = restated.uniform_log_weights(9)
    got = ctx.estep_pair_shares(pools, pool_of, True, np.array([0.5, -0.5], np.float32), restated.DEFAULT_SHARES, log_weights=weights)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, np.array([0.5, -0.5], np.float32), True, restated.DEFAULT_SHARES, weights)
    restated.assert_same(got, want, 'the default grid under the uniform prior')


def test_s3_s4_and_pair_penalties_without_end():
    """S3 on the device with a penalty of 0: under the one share 1 a pair's logit is its first donor's singlet logit of the same row,
    under 0 its second donor's.  S4: the grid {a, a} adds log_f32(2) to the float64 sum.  A pair penalty of -inf makes t = -inf:
    -inf == -inf counts, the logit is -inf, the mean the grid's."""
    from tests import ambient_scoring_restatement as scoring
    ctx, v, cb, e, prob, B, lengths = designed()
    sizes = [3, 11, 16]
    pools, pool_of = designed_pools(sizes, 8)
    for share, which in ((1.0, 0), (0.0, 1)):
        got = check_designed(sizes, 8, [0.0, 0.0, 0.0], np.array([share], np.float32), f'the one share {share}', priors=('null',))
        for p, g in enumerate(sizes):
            d = scoring.pool_options(list(range(g)), True)[which]
            for b in np.flatnonzero(pool_of == p):
                row = got['logits'][got['row_ptr'][b]:got['row_ptr'][b + 1]]
                fio.assert_bitwise(row[g:], row[d[g:]], f'S3: share {share}, barcode {b}')
    grid = np.array([0.25, 0.25], np.float32)
    penalty = np.array([-0.5, 0.5, 0.0], np.float32)
    got = check_designed(sizes, 8, penalty, grid, 'a share twice')
    row_ptr, S, pen, single = restated.float64_sums(v, cb, e, prob, B, pools, pool_of, penalty, True, grid)
    log_two = restated.log32(np.array([2.0], np.float32))[0]
    fio.assert_bitwise(got['logits'][~single], (pen[~single] + (S[~single, 0] + np.float64(log_two))).astype(np.float32), 'S4')
    fio.assert_bitwise(got['share_mean'][~single], np.full(int((~single).sum()), 0.25, np.float32), 'the mean of a share with itself')
    assert np.isfinite(got['logits']).all() and (prob == 0).mean() > 0.03, 'zeros in the table: the floor keeps every term finite'
    endless = check_designed(sizes, 8, [-np.inf, 0.5, -np.inf], np.array([0.5, 0.0, 0.25], np.float32), 'pair penalties of -inf',
                             priors=('null', 'steep'))
    b = int(np.flatnonzero(pool_of == 2)[0])
    row = endless['logits'][endless['row_ptr'][b]:endless['row_ptr'][b + 1]]
    assert np.isfinite(row[:16]).all() and (row[16:] == -np.inf).all() and len(row) == 136
    means = endless['share_mean'][endless['row_ptr'][b]:endless['row_ptr'][b + 1]]
    fio.assert_bitwise(means[16:], np.full(120, np.float32(0.75) / np.float32(3), np.float32), '-inf == -inf: every grid point counts once')
    assert np.isnan(means[:16]).all()


@pytest.mark.parametrize('n', [1, 3, 5])
def test_shares_of_a_half_are_the_ambient_marginal_without_ambient(n):
    """The one fold and finish of the two grid-summed passes (csrc/estep_grid_device.h), on the device: n shares of 0.5
    and n ambient fractions of 0 under the same steep log weights give every pair option the same logit and the same grid point, bit
    for bit, on pools of the 1-, 2-, 4-, 8- and 16-slot forms and grids on either side of 2 and 4 points per walk; one pool's pair
    penalty is -inf.  (tests/test_pair_shares_cpu.py holds the restatements to the same.)"""
    ctx, v, cb, e, prob, B, lengths = designed()
    sizes = [2, 11, 16, 23, 44]
    assert [g * (g + 1) // 2 for g in sizes] == [3, 66, 136, 276, 990]
    pools, pool_of, penalty, shares, alphas, ambient, weights = restated.half_shares_against_no_ambient(sizes, n)
    shared = ctx.estep_pair_shares(pools, pool_of, True, penalty, shares, log_weights=weights)
    summed = ctx.estep_ambient_grid(pools, pool_of, True, penalty, alphas, ambient=ambient, over_grid='marginal', log_weights=weights)
    assert np.array_equal(shared['row_ptr'], summed['row_ptr'])
    pairs = ~np.isnan(shared['share_mean'])  # (a singlet's mean is NaN, a pair's 0.5)
    assert int(pairs.sum()) == sum((g * (g - 1) // 2) * int((pool_of == p).sum()) for p, g in enumerate(sizes))
    fio.assert_bitwise(shared['logits'][pairs], summed['logits'][pairs], f'{n} grid points: the logits of the pair options')
    assert np.array_equal(shared['share_index'][pairs], summed['alpha_index'][pairs]), f'{n} grid points: the grid point of the largest term'
    assert (shared['logits'][pairs] == -np.inf).any() and np.isfinite(shared['logits'][pairs]).any()


def test_null_outputs_are_honoured():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)
    G = prob.shape[1]
    pools, pool_of, penalty = [list(range(G)), [1, 3]], (np.arange(B) % 2).astype(np.int32), np.array([-0.5, 0.25], np.float32)
    full = ctx.estep_pair_shares(pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS)
    restated.assert_same(full, restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, WEIGHTS), 'a fixture under a prior')
    lean = ctx.estep_pair_shares(pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS, fetch_logits=False, fetch_probs=False,
                                 fetch_share_index=False, fetch_share_mean=False)
    assert lean['logits'] is None and lean['probs'] is None and lean['share_index'] is None and lean['share_mean'] is None
    same_bytes(lean, full, ('best_option', 'best_prob', 'doublet_mass', 'best_share_index', 'best_share_mean'), 'without the compact outputs')
    only_means = ctx.estep_pair_shares(pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS, fetch_logits=False, fetch_probs=False,
                                       fetch_share_index=False)
    fio.assert_bitwise(only_means['share_mean'], full['share_mean'], 'the means alone')


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, with_doublets, pool_start, donors, penalty, pool_of, row_ptr, shares, weights=None, n_pools=None, n_shares=None, B=None):
    """dmx_estep_pair_shares with the arrays as given: (status, message, whether an output was written)."""
    from demuxalot_amd import _lib
    pool_start, donors = np.asarray(pool_start, np.int64), np.asarray(donors, np.int32)
    penalty, pool_of, row_ptr = np.asarray(penalty, np.float32), np.asarray(pool_of, np.int32), np.asarray(row_ptr, np.int64)
    shares = None if shares is None else np.asarray(shares, np.float32)
    weights = None if weights is None else np.asarray(weights, np.float32)
    B = ctx.B if B is None else B
    n = max(int(row_ptr.max(initial=0)), 0) + 1
    A = (0 if shares is None else len(shares)) if n_shares is None else n_shares
    outputs = [np.full(n, 7, np.float32), np.full(n, 7, np.float32), np.full(B, 7, np.int32), np.full(B, 7, np.float32), np.full(B, 7, np.float64),
               np.full(n, 7, np.int32), np.full(n, 7, np.float32), np.full(B, 7, np.int32), np.full(B, 7, np.float32)]
    status = ctx._lib.dmx_estep_pair_shares(ctx._h, with_doublets, len(pool_start) - 1 if n_pools is None else n_pools, _lib.ptr(pool_start),
                                            _lib.ptr(donors), _lib.ptr(penalty), _lib.ptr(pool_of), _lib.ptr(row_ptr),
                                            *[_lib.ptr(o) for o in outputs[:5]], A, _lib.ptr(shares), _lib.ptr(weights),
                                            *[_lib.ptr(o) for o in outputs[5:]])
    return status, _lib.load().dmx_last_error().decode(), any((o != 7).any() for o in outputs)


def test_refusals_return_their_code_and_write_nothing():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)  # G = 5
    pools = [[0, 1], [1, 2, 4]]
    pool_of = np.where(np.arange(B) % 5 == 4, -1, np.arange(B) % 2).astype(np.int32)
    penalty = np.array([0.25, -0.5], np.float32)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, WEIGHTS)
    good = dict(with_doublets=1, pool_start=[0, 2, 5], donors=[0, 1, 1, 2, 4], penalty=penalty, pool_of=pool_of, row_ptr=want['row_ptr'], shares=GRID,
                weights=WEIGHTS)
    status, _text, written = raw_call(ctx, **good)
    assert status == 0 and written
    long_grid = np.linspace(0, 1, 65)
    cases = helpers.pool_refusal_cases(good, pool_of) + [
        (dict(with_doublets=0), DMX_ERR_INVALID, 'row_ptr'),  # (the rows were laid out for the pairs)
        (dict(shares=[], weights=None), DMX_ERR_INVALID, 'at least one value'),
        (dict(n_shares=0), DMX_ERR_INVALID, 'at least one value'),
        (dict(n_shares=-3), DMX_ERR_INVALID, 'at least one value'),
        (dict(shares=None, n_shares=5), DMX_ERR_INVALID, 'null shares'),
        (dict(shares=None, weights=None, n_shares=65), DMX_ERR_INVALID, 'null shares'),  # (what is invalid comes first)
        (dict(shares=long_grid, weights=np.zeros(65)), DMX_ERR_UNSUPPORTED, 'more than 64 values'),
        (dict(shares=long_grid, weights=None), DMX_ERR_UNSUPPORTED, 'more than 64 values'),
        (dict(shares=at(long_grid, 64, 1.5), weights=None), DMX_ERR_INVALID, 'share is not finite or outside [0, 1] (index 64)'),
        (dict(shares=at(GRID, 2, np.nan)), DMX_ERR_INVALID, 'share is not finite or outside [0, 1] (index 2)'),
        (dict(shares=at(GRID, 4, 1.5)), DMX_ERR_INVALID, 'share is not finite or outside [0, 1] (index 4)'),
        (dict(shares=at(GRID, 0, -0.1)), DMX_ERR_INVALID, 'share is not finite or outside [0, 1] (index 0)'),
        (dict(weights=at(WEIGHTS, 0, np.nan)), DMX_ERR_INVALID, 'log weight is not finite (index 0)'),
        (dict(weights=at(WEIGHTS, 4, -np.inf)), DMX_ERR_INVALID, 'log weight is not finite (index 4)'),
        (dict(weights=at(WEIGHTS, 2, np.inf)), DMX_ERR_INVALID, 'log weight is not finite (index 2)'),
        (dict(weights=at(WEIGHTS, 2, np.inf), shares=at(GRID, 1, -0.1)), DMX_ERR_INVALID, 'share is not'),  # (the shares come first)
    ]
    launches = ctx.timings()['estep']['launches']
    for change, code, message in cases:
        status, text, written = raw_call(ctx, **{**good, **change})
        assert status == code and message in text and 'dmx_estep_pair_shares' in text, (change, status, text)
        assert not written, (change, 'a refused call writes nothing')
        assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    status, _text, written = raw_call(ctx, **{**good, 'shares': np.linspace(1, 0, 64), 'weights': np.full(64, np.finfo(np.float32).min)})
    assert status == 0 and written, '64 values are the most; every finite weight is one'
    assert ctx.timings()['estep']['launches'] == launches + 1, 'the pass is counted as one E-step'
    from demuxalot_amd._lib import DemuxHipError
    with pytest.raises(DemuxHipError, match=r'log weight.*status -1'):
        ctx.estep_pair_shares(pools, pool_of, True, penalty, GRID, log_weights=at(WEIGHTS, 1, np.nan))
    restated.assert_same(ctx.estep_pair_shares(pools, pool_of, True, penalty, GRID, log_weights=WEIGHTS), want, 'a valid call after the refused ones')


def test_more_than_1024_options_a_missing_table_and_a_communicator_are_refused():
    ctx, *_rest, B, _lengths = designed()
    status, text, written = raw_call(ctx, 1, [0, 45], np.arange(45), [0.0], np.zeros(B, np.int32), np.arange(B + 1) * 1035, [0.5], weights=[0.0])
    assert status == DMX_ERR_UNSUPPORTED and 'more than 1024 options' in text and 'dmx_estep_pair_shares' in text and not written, (status, text)
    B = pools_restatement.fixture_problem('f3_small_0.npz')[4]
    args = dict(with_doublets=1, pool_start=[0, 2], donors=[0, 1], penalty=[0.0], pool_of=np.zeros(B, np.int32), row_ptr=np.arange(B + 1) * 3,
                shares=[0.25, 1.0], weights=[0.0, -1.0], B=B)
    helpers.check_needs_problem_table_no_communicator(raw_call, 'dmx_estep_pair_shares', args)


# ---- 4. the resident results of an E-step are none of this pass's business ------------------------------------------------------------
def test_leaves_the_resident_results_alone():
    from oracle import demux_oracle
    ctx, v, cb, e, prob, B, v2snp = resident(F1)
    G = prob.shape[1]
    penalties = demux_oracle.doublet_penalties(G, 0.35)
    logits, probs = ctx.estep(penalties, True)
    pools, pool_of = [[0, 3, 5], list(range(G))], (np.arange(B) % 2).astype(np.int32)
    first = ctx.estep_pair_shares(pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), GRID, log_weights=WEIGHTS)
    fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() after dmx_estep_pair_shares')
    fio.assert_bitwise(ctx.get_logits(), logits, 'get_logits() after dmx_estep_pair_shares')
    again = ctx.estep_pair_shares(pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), GRID, log_weights=WEIGHTS)
    same_bytes(again, first, SHARED + OWN, 'two runs')


# ---- 5. the front door (exact_mode: predict_posteriors in the exact arithmetic, what the new pass is compared with) ----------------------
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_the_front_door_without_pools(doublet_prior, exact_mode):
    from demuxalot_amd import Demultiplexer, DoubletSharePosteriors
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    plain_logits, plain_probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=doublet_prior)
    half = Demultiplexer.predict_posteriors_with_doublet_shares(calls, genotypes, handler, shares=[0.5], share_log_weights=[0.0],
                                                                doublet_prior=doublet_prior)
    assert isinstance(half, DoubletSharePosteriors)
    for frame, plain in ((half.posteriors[0], plain_logits), (half.posteriors[1], plain_probs)):
        assert list(frame.columns) == list(plain.columns) and list(frame.index) == handler.ordered_barcodes and frame.index.name == 'BARCODE'
        assert frame.values.dtype == np.float32 and list(frame.dtypes) == list(plain.dtypes)
        fio.assert_bitwise(frame.values, plain.values, f'doublet_prior {doublet_prior}: S1 through the front door')
    # the default grid under the uniform prior, against the restatement
    v, cb, e, prob, B = pools_restatement.fixture_problem(F1)
    want_logits, want_probs, want = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, restated.DEFAULT_SHARES,
                                                                restated.uniform_log_weights(9))
    full = Demultiplexer.predict_posteriors_with_doublet_shares(calls, genotypes, handler, doublet_prior=doublet_prior)
    fio.assert_bitwise(full.posteriors[0].values, want_logits, 'the default grid: logits')
    fio.assert_bitwise(full.posteriors[1].values, want_probs, 'the default grid: posteriors')
    assert np.array_equal(full.option_share_index, want['share_index']) and np.array_equal(full.best_share_index, want['best_share_index'])
    assert np.array_equal(np.isnan(full.option_shares), np.isnan(want['share_mean']))
    pairs = ~np.isnan(want['share_mean'])
    fio.assert_bitwise(full.option_shares[pairs], want['share_mean'][pairs].astype(np.float64), 'the default grid: the means')
    summary = full.summary()
    assert list(summary.columns) == ['option', 'probability', 'doublet_probability', 'share', 'major_donor']
    assert np.array_equal(np.isnan(summary['share'].values), want['best_option'] < prob.shape[1])
    assert [('+' in name) for name in summary['option']] == [m is not None for m in summary['major_donor']]


def test_the_front_door_with_pools():
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    names = list(genotypes.genotype_names)
    barcodes = handler.ordered_barcodes
    pool2donors = {'few': [names[5], names[0], names[3]], 'many': names[2:14]}
    barcode2pool = {barcode: (None if i % 5 == 4 else ('few', 'many')[i % 2]) for i, barcode in enumerate(barcodes)}
    result = Demultiplexer.predict_posteriors_with_doublet_shares(calls, genotypes, handler, shares=GRID, share_log_weights=WEIGHTS,
                                                                  barcode2pool=barcode2pool, pool2donors=pool2donors)
    assert isinstance(result.posteriors, PooledPosteriors)
    v, cb, e, prob, B = pools_restatement.fixture_problem(F1)
    pools = [[0, 3, 5], list(range(2, 14))]
    pool_of = np.array([-1 if i % 5 == 4 else i % 2 for i in range(B)], np.int32)
    penalty = pools_restatement.Restatement(v, cb, e, prob, B, 0.35).pair_penalty(pools)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, GRID, WEIGHTS)
    got = dict(row_ptr=result.row_ptr, best_option=result.best_option, best_prob=result.best_prob, doublet_mass=result.doublet_mass,
               share_index=result.option_share_index, best_share_index=result.best_share_index, best_share_mean=result.best_share_mean)
    restated.assert_same(got, want, 'the front door with pools')
    for p, name in enumerate(('few', 'many')):
        logits, probs = result.posteriors.to_dataframes(name)
        rows = np.flatnonzero(pool_of == p)
        K = len(pools[p]) * (len(pools[p]) + 1) // 2
        take = (want['row_ptr'][rows][:, None] + np.arange(K)[None, :])
        fio.assert_bitwise(logits.values, want['logits'][take], f'pool {name}: logits')
        fio.assert_bitwise(probs.values, want['probs'][take], f'pool {name}: posteriors')
    summary = result.summary()
    assert summary['option'].isna().tolist() == (pool_of < 0).tolist()


@pytest.mark.parametrize('share', [0.8, 0.5])
def test_the_value_conditions_hold_through_the_front_door(share):
    from demuxalot_amd import Demultiplexer
    sim, want_fixed, want_grid, _out = restated.simulated(share, 128, 0)
    calls, genotypes, handler = helpers.user_inputs(sim, helpers.table_betas(sim), default_prior=1.0)
    _logits, probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.35)
    G = sim['prob'].shape[1]
    fixed = restated.counts_of(sim, probs.values[:, G:].astype(np.float64).sum(axis=1), probs.values.argmax(axis=1))
    result = Demultiplexer.predict_posteriors_with_doublet_shares(calls, genotypes, handler, doublet_prior=0.35)
    grid = restated.counts_of(sim, result.summary()['doublet_probability'].values, result.best_option)
    # (the front door's table is probs_from_betas of the betas above, the simulation's own probabilities only up to the prior: the
    # bits are the designed problems' and the fixtures' above, the conditions hold on either table)
    print(f'restated: fixed {want_fixed}, grid {want_grid}')
    restated.value_conditions(share, fixed, grid)
