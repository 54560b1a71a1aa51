"""Learning from doublets of unequal shares on the GPU (include/demux_hip_debug.h: dmx_em_doublet_shares, dmx_estep_pair_shares_resident,
dmx_mstep_doublet_shares; csrc/estep_pair_shares.hip: the DENSE form; csrc/mstep_doublet_shares.hip;
Demultiplexer.learn_genotypes_with_doublet_shares, staged_genotype_learning_with_doublet_shares).

Bits only: the device is compared with tests/doublet_shares_learning_restatement.py - pinned in tests/test_doublet_shares_learning_cpu.py
to the even loop at the grid {0.5}, to the pooled loop when no pair is credited and to the contract written out call by call - and, at
the grid {0.5}, with dmx_em_doublets on the same context (D1), without a credited pair with dmx_em_pools under exact additions (D2)."""
import functools

import numpy as np
import pytest

from tests import doublet_learning_problems as problems
from tests import doublet_shares_learning_restatement as learning
from tests import fixture_io as fio
from tests import pair_shares_restatement as shares_restated
from tests import pooled_helpers as helpers
from tests import pools_learning_restatement as pooled
from tests.pooled_helpers import install, install_designed, pools_of

pytestmark = pytest.mark.gpu

F1, F2 = helpers.F1, helpers.F2  # f1: G = 20, B = 1000
HALF, ZERO = np.array([0.5], np.float32), np.array([0.0], np.float32)
GRIDS = {  # unsorted, with duplicates and both ends
    1: np.array([0.8], np.float32),
    2: np.array([1.0, 0.0], np.float32),
    3: np.array([0.7, 0.0, 1.0], np.float32),
    5: np.array([0.5, 0.9, 0.1, 0.9, 0.3], np.float32),
    9: shares_restated.DEFAULT_SHARES[::-1].copy(),
    64: np.concatenate([[1.0, 0.0, 0.25, 0.25], np.random.default_rng(64).uniform(0, 1, 60)]).astype(np.float32),
}
SHARED = ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass')


def weights_of(n):
    return np.linspace(-2.0, 0.5, n).astype(np.float32)[np.random.default_rng(n).permutation(n)]


learner = functools.lru_cache(maxsize=None)(helpers.new_learner)  # a fixture installed for learning, the contexts this module's own
assert_iteration = functools.partial(helpers.assert_iteration, same=learning.assert_same)  # (the E-step's outputs with its shares)


def staged(ctx, n, clip, pools, pool_of, with_doublets, penalty, shares, log_weights, threshold, power=2.):
    """The step-wise path over the shares: the resident E-step over the grid, dmx_mstep_doublet_shares on its rows and means behind it."""
    return helpers.staged(
        ctx, n, clip, lambda: ctx.estep_pair_shares(pools, pool_of, with_doublets, penalty, shares, log_weights, resident=True),
        lambda out: ctx.mstep_doublet_shares(pools, pool_of, with_doublets, penalty, out['probs'], out['share_mean'], threshold, power))


# ---- D1: the grid {0.5} is dmx_em_doublets, every output and every iteration's addition --------------------------------------------
@pytest.mark.parametrize('dp', [0.35, 0.0])
@pytest.mark.parametrize('name', [F1, F2, 'f3_small_1.npz'])
def test_d1_the_even_grid_is_em_doublets(name, dp):
    ctx = learner(name)
    pools, pool_of = pools_of(name, ctx.B, ctx.G)
    penalty = learning.pair_penalties(pools, dp)
    problem = pooled.fixture_learning_problem(name)
    history = learning.learn(problem, pools, pool_of, 3, 0.01, dp, HALF, ZERO)
    for n in (1, 2, 3):  # the fused call's addition is the one its last E-step used: every iteration's, one call each
        want = ctx.em_doublets(n, 0.01, pools, pool_of, dp != 0, penalty)
        want_dense, want_betas = ctx.get_probs(), ctx.get_learnt_betas()
        for log_weights in (ZERO, None):
            got = ctx.em_doublet_shares(n, 0.01, pools, pool_of, dp != 0, penalty, HALF, log_weights)
            for key in want:
                assert got[key].tobytes() == want[key].tobytes(), f'{name} dp {dp}, {n} iterations: {key} against dmx_em_doublets'
            fio.assert_bitwise(ctx.get_probs(), want_dense, f'{name} dp {dp}, {n} iterations: get_probs() against dmx_em_doublets')
            fio.assert_bitwise(ctx.get_learnt_betas(), want_betas, f'{name} dp {dp}, {n} iterations: learnt betas against dmx_em_doublets')
        assert_iteration(ctx, got, history[n - 1], f'{name} dp {dp}, {n} iterations: the restatement', got['addition'])
        pair = ~history[n - 1]['single']
        assert (got['share_mean'][pair] == np.float32(0.5)).all() and np.isnan(got['share_mean'][~pair]).all()


# ---- D2: no credited pair is dmx_em_pools with exact additions --------------------------------------------------------------------
@pytest.mark.parametrize('dp, threshold, grid', [(0.35, 2.0, 1), (0.0, 1e-3, 1), (0.0, 1e-3, 9)])
@pytest.mark.parametrize('name', [F1, F2, 'f3_small_3.npz'])
def test_d2_no_credited_pair_is_the_pooled_loop(name, dp, threshold, grid):
    ctx = learner(name)
    pools, pool_of = pools_of(name, ctx.B, ctx.G)
    penalty = learning.pair_penalties(pools, dp)
    shares = HALF if dp else GRIDS[grid]
    problem = pooled.fixture_learning_problem(name)
    history = pooled.learn(problem, pools, pool_of, 3, 0.01, dp)
    what = f'{name} dp {dp} threshold {threshold}'
    ctx.set_exact_additions(True)
    try:
        want = ctx.em_pools(3, 0.01, pools, pool_of, dp != 0, penalty)
        want_dense, want_betas = ctx.get_probs(), ctx.get_learnt_betas()
        got = ctx.em_doublet_shares(3, 0.01, pools, pool_of, dp != 0, penalty, shares, None, threshold)
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), f'{what}: {key} against dmx_em_pools'
        fio.assert_bitwise(ctx.get_probs(), want_dense, f'{what}: get_probs() against dmx_em_pools')
        fio.assert_bitwise(ctx.get_learnt_betas(), want_betas, f'{what}: learnt betas against dmx_em_pools')
        fio.assert_bitwise(got['addition'], history[-1]['addition'], f'{what}: addition against the pooled restatement')
        if dp == 0:
            assert (got['share_index'] == -1).all() and np.isnan(got['share_mean']).all()
            assert (got['best_share_index'] == -1).all() and np.isnan(got['best_share_mean']).all()
    finally:
        ctx.apply_environment()


def test_another_power_without_credited_pairs_is_the_pooled_loop_to_float32_accuracy():
    """dmx_mstep raises to another power than 2 with powf, this M-step with the float64 pow rounded once: each weight
    within 1 ulp and half an ulp of the true power, sums of non-negative terms, two final roundings - 2.5 * 2^-23 relative."""
    ctx = learner('f3_small_3.npz')
    pools, pool_of = pools_of('f3_small_3.npz', ctx.B, ctx.G)
    penalty = learning.pair_penalties(pools, 0.35)
    ctx.set_exact_additions(True)
    try:
        want = ctx.em_pools(2, 0.01, pools, pool_of, True, penalty, contribution_power=1.5)
        got = ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, HALF, None, 2.0, contribution_power=1.5)
    finally:
        ctx.apply_environment()
    assert want['addition'].any()
    np.testing.assert_allclose(got['addition'], want['addition'], rtol=2.5 * 2.0 ** -23, atol=0)


# ---- D4, grids of every length: the fused call, the step-wise path and the restatement on every iteration --------------------------
@pytest.mark.parametrize('n_shares', sorted(GRIDS))
def test_d4_fused_equals_stepwise_on_every_grid(n_shares):
    name = F1 if n_shares in (3, 9) else F2
    ctx = learner(name)
    pools, pool_of = pools_of(name, ctx.B, ctx.G)
    penalty = learning.pair_penalties(pools, 0.35)
    shares, log_weights = GRIDS[n_shares], weights_of(n_shares)
    problem = pooled.fixture_learning_problem(name)
    history = learning.learn(problem, pools, pool_of, 3, 0.01, 0.35, shares, log_weights)
    assert learning.live_pairs(history[1], pools, pool_of, True, 1e-3).any()
    got = ctx.em_doublet_shares(3, 0.01, pools, pool_of, True, penalty, shares, log_weights)
    assert_iteration(ctx, got, history[-1], f'{name}, {n_shares} shares: fused', got['addition'])
    fio.assert_bitwise(ctx.get_learnt_betas(), learning.learnt_betas(problem, history), 'learnt betas against the restatement')
    for it, (step, addition) in enumerate(staged(ctx, 3, 0.01, pools, pool_of, True, penalty, shares, log_weights, 1e-3)):
        assert_iteration(ctx, step, history[it], f'{name}, {n_shares} shares: step-wise iteration {it}', addition)
    for key in SHARED + shares_restated.OWN:
        assert step[key].tobytes() == got[key].tobytes(), f'{n_shares} shares: step-wise {key} against the fused call'
    second = ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, shares, log_weights)['addition']
    fio.assert_bitwise(second, history[1]['addition'], "the fused call's second addition is the stateless M-step's behind the resident E-step")


# ---- the designed problem: all five dense forms, donors in different 64-column words ------------------------------------------------
SIZES = (2, 10, 11, 15, 16, 22, 23, 31, 32, 36, 44)  # options 3, 55 | 66, 120 | 136, 253, 276, 496, 528, 666, 990: 1, 2, 4, 8, 16 slots


@functools.lru_cache(maxsize=None)
def designed():
    """pair_shares_restatement.designed_problem - 48 barcodes of 0 .. 40 calls, a table 1024 columns wide with entries of exactly 0 and
    1 - with pools of SIZES donors drawn over all columns (every pool of more than two donors has donors in several 64-column words),
    barcode b in pool (b + b // 12) % 12, the twelfth in none; the pair penalty of the pool of 23 is -inf."""
    v, cb, e, prob, B, lengths, v2snp = shares_restated.designed_problem()
    rng = np.random.default_rng(17)
    pools = [sorted(int(d) for d in rng.choice(prob.shape[1], size=g, replace=False)) for g in SIZES]
    pool_of = ((np.arange(B) + np.arange(B) // 12) % 12).astype(np.int32)
    pool_of[pool_of == len(pools)] = -1
    penalty = np.linspace(-2, 1.5, len(pools)).astype(np.float32)
    penalty[SIZES.index(23)] = -np.inf
    assert all(len({d >> 6 for d in donors}) > 1 for donors in pools[1:]) and (pool_of == -1).any() and lengths[0] == 0
    for p in range(len(pools)):
        assert len(set(lengths[pool_of == p])) > 1, 'rows of several lengths in every pool'
    betas = (prob + np.float32(0.05)).astype(np.float32)
    problem = dict(v=v, cb=cb, e=e, v2snp=v2snp, betas=betas, raw_betas=betas, B=B)
    return problem, prob, pools, pool_of, penalty


def test_designed_problem_runs_every_dense_form():
    from demuxalot_amd.device import DeviceContext
    problem, _prob, pools, pool_of, penalty = designed()
    shares, log_weights = GRIDS[3], weights_of(3)
    history = learning.learn(problem, pools, pool_of, 2, 0.01, 0.35, shares, log_weights, threshold=1e-6, penalty=penalty)
    live = learning.live_pairs(history[0], pools, pool_of, True, 1e-6)
    print(f'live pairs per barcode: {sorted(set(live.tolist()))}')
    assert live.max() > 64 and (live == 0).any()
    assert not live[pool_of == SIZES.index(23)].any(), 'a pair under the penalty -inf has posterior 0'
    with DeviceContext(0) as ctx:
        install_designed(ctx, problem)
        got = ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, shares, log_weights, 1e-6)
        assert_iteration(ctx, got, history[-1], 'the designed problem, fused', got['addition'])
        assert got['addition'].any()
        for it, (step, addition) in enumerate(staged(ctx, 2, 0.01, pools, pool_of, True, penalty, shares, log_weights, 1e-6)):
            assert_iteration(ctx, step, history[it], f'the designed problem, step-wise iteration {it}', addition)


LIST_LENGTHS = (0, 1, 4, 5, 64, 65, 3, 63, 66, 128, 129, 10 ** 6)  # (capped by the row's pair options: several hundred in the wide pools)


@pytest.mark.parametrize('power', [2., 1.5])
def test_designed_lists_cross_the_ahead_entries_and_the_64_entry_trip(power):
    """The stateless M-step takes the caller's rows: posteriors and shares set by hand give lists of exactly 0, 1, 4, 5, 64, 65 and
    several hundred entries (rows of 253, 666 and 990 options), shares of exactly 0 and 1 among them, on a table with entries of
    exactly 0 and 1 (dmx_set_probs)."""
    from demuxalot_amd.device import DeviceContext
    problem, prob, pools, pool_of, penalty = designed()
    v, cb, e, B = problem['v'], problem['cb'], problem['e'], problem['B']
    shares, threshold = GRIDS[5], 1e-3
    rows, dense = learning.estep(v, cb, e, prob, B, pools, pool_of, penalty, True, shares, None)
    rng = np.random.default_rng(5)
    post = rng.uniform(0, 4e-4, size=len(rows['probs'])).astype(np.float32)
    mean = rng.choice(np.array([0.0, 1.0, 0.5, 0.8, 0.123], np.float32), size=len(post))
    mean[rows['single']] = np.nan
    lengths, full, queue = np.zeros(B, np.int64), set(), list(LIST_LENGTHS)
    called = np.bincount(cb, minlength=B) > 0
    for b in range(B):
        if pool_of[b] < 0:
            continue
        g, first, last = len(pools[pool_of[b]]), rows['row_ptr'][b], rows['row_ptr'][b + 1]
        whole = g >= 22 and called[b] and pool_of[b] not in full  # the first barcode with calls of every wide pool: its whole row
        full.add(pool_of[b]) if whole else None
        wide = called[b] and not whole and last - first - g >= 129 and queue  # the lengths in turn, where a row holds each of them
        wanted = queue.pop(0) if wide else LIST_LENGTHS[(b // 2) % len(LIST_LENGTHS)]
        lengths[b] = last - first - g if whole else min(wanted, last - first - g)
        at = first + g + rng.choice(last - first - g, size=lengths[b], replace=False)
        post[at] = rng.uniform(1e-3, 0.4, size=lengths[b]).astype(np.float32)
        post[at[:1]] = np.float32(1e-3)  # (exactly the threshold: live)
    crafted = dict(rows, probs=post, share_mean=mean)
    assert np.array_equal(learning.live_pairs(crafted, pools, pool_of, True, threshold), lengths)
    print(f'list lengths of the barcodes with calls: {sorted(set(lengths[called].tolist()))}')
    assert {0, 1, 4, 5, 64, 65} <= set(lengths[called].tolist()) and lengths[called].max() > 300
    want = learning.share_addition(v, cb, e, dense, crafted, pools, pool_of, True, prob, power=power, threshold=threshold)
    plain = learning.share_addition(v, cb, e, dense, crafted, pools, pool_of, True, prob, power=power, threshold=2.0)
    assert (want != plain).sum() > 100
    with DeviceContext(0) as ctx:
        ctx.set_problem(B, len(prob), prob.shape[1], v, cb, e, problem['v2snp'])
        ctx.set_probs(prob)
        got = ctx.estep_pair_shares(pools, pool_of, True, penalty, shares, None, resident=True)
        assert_iteration(ctx, got, dict(rows, dense=dense), 'the resident E-step on the table with zeros and ones')
        addition = ctx.mstep_doublet_shares(pools, pool_of, True, penalty, post, mean, threshold, power)
        fio.assert_bitwise(addition, want, f'power {power}: the additions of the crafted lists')
        fio.assert_bitwise(ctx.mstep_doublet_shares(pools, pool_of, True, penalty, post, mean, 2.0, power), plain, f'power {power}: no live pair')


@pytest.mark.parametrize('n_shares', [1, 2, 5, 9, 64])
def test_designed_grids_of_every_length(n_shares):
    from demuxalot_amd.device import DeviceContext
    problem, prob, pools, pool_of, penalty = designed()
    v, cb, e, B = problem['v'], problem['cb'], problem['e'], problem['B']
    keep = [SIZES.index(g) for g in (2, 11, 16, 22)]  # 1, 2 and 4 slots: the register and the LDS state
    pools = [pools[p] for p in keep]
    pool_of = np.array([keep.index(p) if p in keep else -1 for p in pool_of], np.int32)
    penalty = penalty[keep]
    shares, log_weights = GRIDS[n_shares], weights_of(n_shares)
    rows, dense = learning.estep(v, cb, e, prob, B, pools, pool_of, penalty, True, shares, log_weights)
    want = learning.share_addition(v, cb, e, dense, rows, pools, pool_of, True, prob, threshold=1e-6)
    with DeviceContext(0) as ctx:
        ctx.set_problem(B, len(prob), prob.shape[1], v, cb, e, problem['v2snp'])
        ctx.set_probs(prob)
        got = ctx.estep_pair_shares(pools, pool_of, True, penalty, shares, log_weights, resident=True)
        assert_iteration(ctx, got, dict(rows, dense=dense), f'{n_shares} shares: the resident E-step')
        plain = ctx.estep_pair_shares(pools, pool_of, True, penalty, shares, log_weights)
        for key in SHARED + shares_restated.OWN:
            assert plain[key].tobytes() == got[key].tobytes(), f'{n_shares} shares: the dense form against the plain one: {key}'
        addition = ctx.mstep_doublet_shares(pools, pool_of, True, penalty, got['probs'], got['share_mean'], 1e-6)
        fio.assert_bitwise(addition, want, f'{n_shares} shares: the additions')


# ---- D3 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('end', [1.0, 0.0])
def test_d3_a_grid_of_one_end_credits_one_donor(end):
    ctx = learner(F2)
    pools, pool_of = pools_of(F2, ctx.B, ctx.G)
    penalty = learning.pair_penalties(pools, 0.35)
    problem = pooled.fixture_learning_problem(F2)
    shares = np.array([end], np.float32)
    history = learning.learn(problem, pools, pool_of, 2, 0.01, 0.35, shares)  # (pinned to the one-donor credit on the CPU)
    got = ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, shares)
    assert_iteration(ctx, got, history[-1], f'shares {{{end}}}', got['addition'])
    assert (got['share_mean'][~history[-1]['single']] == np.float32(end)).all()


# ---- float32 rounding ties: the redo runs, and at {0.5} it redoes what dmx_mstep_doublets redoes ------------------------------------
TIE_THRESHOLD = 0.5


def test_rounding_ties_are_redone_in_call_order():
    from demuxalot_amd.device import DeviceContext
    p = problems.tie_problem()
    B, (V, G) = p['B'], p['prob'].shape
    penalty = learning.pair_penalties(p['pools'], 0.35)
    rows, dense = learning.estep(p['v'], p['cb'], p['e'], p['prob'], B, p['pools'], p['pool_of'], penalty, True, HALF, None)
    args = (p['v'], p['cb'], p['e'], dense, rows, p['pools'], p['pool_of'], True, p['prob'])
    in_order = learning.share_addition(*args, threshold=TIE_THRESHOLD)
    of_partials = learning.share_addition_of_items(*args, item_calls=1024, threshold=TIE_THRESHOLD)
    differ = np.argwhere(in_order != of_partials)
    assert len(differ) >= 1, 'the problem decides between the two summation orders'
    with DeviceContext(0) as ctx:
        ctx.set_problem(B, V, G, p['v'], p['cb'], p['e'], p['v2snp'])
        ctx.set_probs(p['prob'])
        got = ctx.estep_pair_shares(p['pools'], p['pool_of'], True, penalty, HALF, None, resident=True)
        assert_iteration(ctx, got, dict(rows, dense=dense), 'the E-step of the tie problem')
        addition = ctx.mstep_doublet_shares(p['pools'], p['pool_of'], True, penalty, got['probs'], got['share_mean'], TIE_THRESHOLD)
        redone = ctx.redo_count()
        fio.assert_bitwise(addition, in_order, 'the additions, variants of three work items among them')
        assert redone >= len(differ), 'the sums at a rounding boundary were redone in call order'
        even = ctx.mstep_doublets(p['pools'], p['pool_of'], True, penalty, got['probs'], TIE_THRESHOLD)
        fio.assert_bitwise(addition, even, 'at {0.5}: dmx_mstep_doublets')
        assert ctx.redo_count() == redone, 'at {0.5} both forms queue the same sums'
        # an uneven share on the same rows: the doublets' credit moves from 0.5 to 0.8 / 0.2, the redo still gives the in-order sums
        mean = np.where(rows['single'], np.nan, np.float32(0.8)).astype(np.float32)
        uneven = dict(rows, share_mean=mean)
        want = learning.share_addition(p['v'], p['cb'], p['e'], dense, uneven, p['pools'], p['pool_of'], True, p['prob'], threshold=TIE_THRESHOLD)
        assert (want != in_order).any()
        fio.assert_bitwise(ctx.mstep_doublet_shares(p['pools'], p['pool_of'], True, penalty, got['probs'], mean, TIE_THRESHOLD), want, 'share 0.8')


# ---- refusals, by their code --------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from demuxalot_amd._lib import DemuxHipError
    from demuxalot_amd.device import DeviceContext
    name = 'f3_small_1.npz'
    problem = pooled.fixture_learning_problem(name)
    B, (V, G) = problem['B'], problem['betas'].shape
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    penalty = learning.pair_penalties(pools, 0.35)
    grid = GRIDS[5]

    def changed(array, at, value):
        out = array.copy()
        out[at] = value
        return out

    with DeviceContext(0) as ctx:
        install(ctx, name)
        good = ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, grid)
        rows, mean = good['probs'], good['share_mean']
        pair = int(np.flatnonzero(~np.isnan(mean))[0])
        assert np.isnan(mean[0]) and pair == G
        dense, betas = ctx.get_probs(), ctx.get_learnt_betas()

        def launches():
            timings = ctx.timings()
            return tuple(timings[phase]['launches'] for phase in ('pstep', 'estep', 'mstep', 'mcombine'))

        before = launches()
        em = lambda **kw: ctx.em_doublet_shares(**{**dict(n_iterations=2, p_genotype_clip=0.01, pools=pools, pool_of_barcode=pool_of,  # noqa: E731
                                                          with_doublets=True, pair_penalty=penalty, shares=grid), **kw})
        estep = lambda **kw: ctx.estep_pair_shares(**{**dict(pools=pools, pool_of_barcode=pool_of, with_doublets=True, pair_penalty=penalty,  # noqa: E731
                                                             shares=grid, resident=True), **kw})
        mstep = lambda post_rows=rows, share_rows=mean, pools=pools, **kw: ctx.mstep_doublet_shares(pools, pool_of, True, penalty, post_rows, share_rows, **kw)  # noqa: E731
        cases = [
            (lambda: em(n_iterations=0), r'dmx_em_doublet_shares.*n_iterations.*status -1'),
            (lambda: em(contribution_power=0.0), r'dmx_em_doublet_shares.*power.*status -1'),
            (lambda: em(contribution_power=float('nan')), r'power.*status -1'),
            (lambda: em(min_pair_posterior=0.0), r'min_pair_posterior.*status -1'),
            (lambda: em(min_pair_posterior=float('inf')), r'min_pair_posterior.*status -1'),
            (lambda: em(shares=np.zeros(0, np.float32)), r'dmx_em_doublet_shares.*at least one value.*status -1'),
            (lambda: em(shares=changed(grid, 2, 1.5)), r'dmx_em_doublet_shares.*share is not finite or outside.*index 2.*status -1'),
            (lambda: em(shares=changed(grid, 4, np.nan)), r'share is not finite or outside.*index 4.*status -1'),
            (lambda: em(log_weights=changed(weights_of(5), 1, np.inf)), r'log weight is not finite.*index 1.*status -1'),
            (lambda: em(shares=np.full(65, 0.5, np.float32)), r'dmx_em_doublet_shares.*more than 64 values.*status -5'),
            (lambda: em(shares=changed(grid, 0, -1.0), n_iterations=0), r'share is not finite'),  # (the grid ahead of the count)
            (lambda: em(pools=[[0, 0]]), r'status -1'),
            (lambda: em(pool_of_barcode=changed(pool_of, 2, 5)), r'status -1'),
            (lambda: estep(shares=np.zeros(0, np.float32)), r'dmx_estep_pair_shares_resident.*at least one value.*status -1'),
            (lambda: estep(shares=changed(grid, 1, -0.5)), r'dmx_estep_pair_shares_resident.*index 1.*status -1'),
            (lambda: estep(shares=np.full(65, 0.5, np.float32)), r'dmx_estep_pair_shares_resident.*status -5'),
            (lambda: estep(pools=[[0, 0]]), r'dmx_estep_pair_shares_resident.*status -1'),
            (lambda: mstep(contribution_power=-2.0), r'dmx_mstep_doublet_shares.*power.*status -1'),
            (lambda: mstep(min_pair_posterior=0.0), r'dmx_mstep_doublet_shares.*min_pair_posterior.*status -1'),
            (lambda: mstep(rows[:-1], mean[:-1]), r'dmx_mstep_doublet_shares.*length.*status -1'),
            (lambda: mstep(changed(rows, 3, np.nan)), r'dmx_mstep_doublet_shares.*posterior of the rows.*index 3.*status -1'),
            (lambda: mstep(share_rows=None), r'dmx_mstep_doublet_shares.*null share rows.*status -1'),
            (lambda: mstep(share_rows=changed(mean, pair, np.nan)), rf"dmx_mstep_doublet_shares.*pair's share of the rows.*index {pair}.*status -1"),
            (lambda: mstep(share_rows=changed(mean, len(mean) - 1, 1.5)), rf"pair's share of the rows.*index {len(mean) - 1}.*status -1"),
            (lambda: mstep(share_rows=changed(mean, pair + 1, -0.25)), r"pair's share of the rows.*status -1"),
            (lambda: mstep(pools=[[0, 0]]), r'dmx_mstep_doublet_shares.*status -1'),
        ]
        for call, message in cases:
            with pytest.raises(DemuxHipError, match=message):
                call()
            assert launches() == before, (message, 'a refused call launches nothing')
        fio.assert_bitwise(ctx.get_probs(), dense, 'the resident posteriors after the refusals')
        fio.assert_bitwise(ctx.get_learnt_betas(), betas, 'the addition after the refusals')
        again = em()
        for key in good:
            assert again[key].tobytes() == good[key].tobytes(), f'a valid call after the refused ones: {key}'
        # a singlet's entry of the share rows is not read
        want = mstep()
        fio.assert_bitwise(mstep(share_rows=changed(mean, 0, 7.0)), want, 'a singlet entry of the share rows')
    with DeviceContext(0) as ctx:  # call order: nothing, a problem, a table, posteriors
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_doublet_shares.*problem.*status -1'):
            ctx.B, ctx.V, ctx.G = B, V, G
            ctx.mstep_doublet_shares(pools, pool_of, True, penalty, rows, mean)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_doublet_shares.*genotype probabilities.*status -1'):
            ctx.mstep_doublet_shares(pools, pool_of, True, penalty, rows, mean)
        with pytest.raises(DemuxHipError, match=r'dmx_em_doublet_shares.*call order.*status -1'):
            ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, grid)
        with pytest.raises(DemuxHipError, match=r'dmx_estep_pair_shares_resident.*call order.*status -1'):
            ctx.estep_pair_shares(pools, pool_of, True, penalty, grid, resident=True)
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_doublet_shares.*E-step.*status -1'):
            ctx.mstep_doublet_shares(pools, pool_of, True, penalty, rows, mean)
        assert all(ctx.timings()[phase]['launches'] == 0 for phase in ('estep', 'mstep', 'mcombine'))
    with DeviceContext(0) as ctx:
        ctx.comm_init_emulated(0, 1)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        ctx.estep(np.zeros(G, np.float32), False)
        for call in (lambda: ctx.em_doublet_shares(2, 0.01, pools, pool_of, True, penalty, grid),
                     lambda: ctx.estep_pair_shares(pools, pool_of, True, penalty, grid, resident=True),
                     lambda: ctx.mstep_doublet_shares(pools, pool_of, True, penalty, rows, mean)):
            with pytest.raises(DemuxHipError, match=r'communicator.*status -5'):
                call()
    from demuxalot_amd import Demultiplexer
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='min_pair_posterior'):
            Demultiplexer.learn_genotypes_with_doublet_shares({}, None, None, min_pair_posterior=bad)
    with pytest.raises(ValueError, match='shares'):
        Demultiplexer.learn_genotypes_with_doublet_shares({}, None, None, shares=[0.5, 1.5])


# ---- the front door, and "does it help?" on the device ---------------------------------------------------------------------------
def simulation_inputs(share, seed=0):
    """tests/doublet_shares_learning_restatement.simulated() and what a user holds of it: genotypes with the problem's betas and default
    prior 0 - the prior betas of the learning loop are then those betas themselves."""
    problem, sim, yardstick, history = learning.simulated(share, seed)
    return (problem, sim, yardstick, history) + helpers.user_inputs(sim, problem['betas'], default_prior=0.0)


def test_even_doublets_through_the_front_door_lose_no_more_than_the_half_gain():
    """The share-0.5 simulation at seed 0 through learn_genotypes_with_doublet_shares: the restatement's bits, and what the device
    learnt no further from the truth than 1 + the half-gain of the even loop's error (the grid has nothing to find there)."""
    from demuxalot_amd import Demultiplexer
    problem, sim, yardstick, history, calls, genotypes, handler = simulation_inputs(0.5)
    B, G = sim['B'], sim['prob'].shape[1]
    K = G * (G + 1) // 2
    learnt, result = Demultiplexer.learn_genotypes_with_doublet_shares(calls, genotypes, handler)  # the default grid, the uniform prior
    fio.assert_bitwise(result.posteriors[1].values, history[-1]['probs'].reshape(B, K), 'share 0.5: the last posteriors')
    fio.assert_bitwise(learnt.variant_betas, learning.learnt_betas(problem, history), 'share 0.5: learnt betas')
    assert result.best_option.tobytes() == history[-1]['best_option'].tobytes()
    assert result.best_share_mean.tobytes() == history[-1]['best_share_mean'].tobytes()
    table = learning.demux_oracle.probs_from_betas(sim['v2snp'], learnt.variant_betas, 0.01)
    learning.value_condition(0.5, learning.table_error(yardstick[-1]['prob_table'], sim), learning.table_error(table, sim),
                             yardstick[-1]['best_option'], result.best_option, sim)


def test_learn_genotypes_with_doublet_shares_end_to_end():
    from demuxalot_amd import Demultiplexer, DoubletSharePosteriors, PooledPosteriors
    problem, sim, yardstick, history, calls, genotypes, handler = simulation_inputs(0.8)
    B, G = sim['B'], sim['prob'].shape[1]
    K = G * (G + 1) // 2
    barcodes, donors = handler.ordered_barcodes, list(genotypes.genotype_names)
    learnt, result = Demultiplexer.learn_genotypes_with_doublet_shares(calls, genotypes, handler)  # the default grid, the uniform prior
    assert isinstance(result, DoubletSharePosteriors)
    _logits_df, probs_df = result.posteriors
    assert list(probs_df.index) == barcodes and list(probs_df.columns)[:G] == donors and probs_df.shape == (B, K) and probs_df.values.dtype == np.float32
    fio.assert_bitwise(probs_df.values, history[-1]['probs'].reshape(B, K), 'the last posteriors')
    fio.assert_bitwise(learnt.variant_betas, learning.learnt_betas(problem, history), 'learnt betas')
    assert result.best_share_mean.tobytes() == history[-1]['best_share_mean'].tobytes()
    assert learnt.genotype_names == genotypes.genotype_names and learnt is not genotypes
    # does it help?  what the device learnt, against the even loop's error as its restatement states it
    table = learning.demux_oracle.probs_from_betas(sim['v2snp'], learnt.variant_betas, 0.01)
    learning.value_condition(0.8, learning.table_error(yardstick[-1]['prob_table'], sim), learning.table_error(table, sim),
                             yardstick[-1]['best_option'], result.best_option, sim)
    # the generator: every iteration, the same last one
    for it, (step, debug) in enumerate(Demultiplexer.staged_genotype_learning_with_doublet_shares(calls, genotypes, handler)):
        fio.assert_bitwise(step.posteriors[1].values, history[it]['probs'].reshape(B, K), f'generator, iteration {it}: posteriors')
        fio.assert_bitwise(debug['genotype_addition'], history[it]['addition'], f'generator, iteration {it}: addition')
        fio.assert_bitwise(debug['genotype_prior'], problem['betas'], 'generator: prior betas')
    assert it == 4 and step.posteriors[1].values.tobytes() == probs_df.values.tobytes()
    # the even grid is learn_genotypes_from_doublets
    want_learnt, want = Demultiplexer.learn_genotypes_from_doublets(calls, genotypes, handler, n_iterations=3)
    same_learnt, same = Demultiplexer.learn_genotypes_with_doublet_shares(calls, genotypes, handler, n_iterations=3, shares=[0.5], share_log_weights=[0.0])
    fio.assert_bitwise(same.posteriors[1].values, want.values, 'shares [0.5]: the posteriors of learn_genotypes_from_doublets')
    fio.assert_bitwise(same_learnt.variant_betas, want_learnt.variant_betas, 'shares [0.5]: the betas of learn_genotypes_from_doublets')
    # with pools: the restatement's bits
    pool2donors = {'low': donors[:5][::-1], 'high': donors[3:]}
    barcode2pool = {bc: (None if b % 7 == 0 else 'low' if b % 2 else 'high') for b, bc in enumerate(barcodes)}
    pools = [list(range(5)), list(range(3, G))]
    pool_of = np.array([-1 if b % 7 == 0 else 0 if b % 2 else 1 for b in range(B)], dtype=np.int32)
    grid = [0.2, 0.8, 0.5]
    weights = shares_restated.uniform_log_weights(3)
    pooled_history = learning.learn(problem, pools, pool_of, 3, 0.01, 0.35, np.array(grid, np.float32), weights, threshold=1e-2)
    got_learnt, got = Demultiplexer.learn_genotypes_with_doublet_shares(calls, genotypes, handler, n_iterations=3, shares=grid, min_pair_posterior=1e-2,
                                                                        barcode2pool=barcode2pool, pool2donors=pool2donors)
    assert isinstance(got.posteriors, PooledPosteriors)
    for key in SHARED:
        assert getattr(got.posteriors, key).tobytes() == pooled_history[-1][key].tobytes(), f'with pools against the restatement: {key}'
    assert got.option_share_index.tobytes() == pooled_history[-1]['share_index'].tobytes()
    fio.assert_bitwise(got_learnt.variant_betas, learning.learnt_betas(problem, pooled_history), 'with pools: learnt betas')
    for it, (step, debug) in enumerate(Demultiplexer.staged_genotype_learning_with_doublet_shares(
            calls, genotypes, handler, n_iterations=3, shares=grid, min_pair_posterior=1e-2, barcode2pool=barcode2pool, pool2donors=pool2donors)):
        assert step.posteriors.probs.tobytes() == pooled_history[it]['probs'].tobytes(), f'generator with pools, iteration {it}'
        fio.assert_bitwise(debug['genotype_addition'], pooled_history[it]['addition'], f'generator with pools, iteration {it}: addition')
