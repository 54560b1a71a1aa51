"""Learning from doublet posteriors on the GPU (include/demux_hip_debug.h: dmx_em_doublets, dmx_mstep_doublets; csrc/mstep_doublets.hip;
Demultiplexer.learn_genotypes_from_doublets, staged_genotype_learning_from_doublets).

The additions are compared bit for bit with tests/doublet_learning_restatement.py - the pooled loop with the crediting M-step, pinned in
tests/test_doublet_learning_cpu.py to the pooled loop itself when no pair is credited and to the contract written out call by call -
and, when no pair is credited, with dmx_em_pools under exact additions on the same context."""
import functools

import numpy as np
import pytest

from tests import doublet_learning_problems as problems
from tests import doublet_learning_restatement as learning
from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests import pools_learning_restatement as pooled
from tests import pools_restatement as restated
from tests.pooled_helpers import assert_iteration, exact_mode, install, install_designed, pair_penalty, pool_of_f1  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

F1, SMALL, POOLS_F1 = helpers.F1, helpers.F3_SMALL, helpers.POOLS_F1  # f1: G = 20, B = 1000
learner = functools.lru_cache(maxsize=None)(helpers.new_learner)  # a fixture installed for learning, the contexts this module's own


def staged(ctx, n, clip, pools, pool_of, with_doublets, penalty, threshold, power=2.):
    """The step-wise path with credited pairs: the resident pooled E-step, dmx_mstep_doublets on its rows behind it."""
    return helpers.staged(ctx, n, clip, lambda: ctx.estep_pools(pools, pool_of, with_doublets, penalty, resident=True),
                          lambda out: ctx.mstep_doublets(pools, pool_of, with_doublets, penalty, out['probs'], threshold, power))


# ---- 1. no pair is credited: dmx_em_pools with exact additions, and the restatement --------------------------------
@pytest.mark.parametrize('dp, threshold', [(0.35, 2.0), (0.0, 1e-3)])
@pytest.mark.parametrize('name', SMALL + ['f2_synthetic_g4.npz', F1])
def test_no_credited_pair_is_the_pooled_loop(name, dp, threshold):
    ctx = learner(name)
    problem = pooled.fixture_learning_problem(name)
    B, G = ctx.B, ctx.G
    pools, pool_of = (POOLS_F1, pool_of_f1()) if name == F1 else ([list(range(G))], np.zeros(B, np.int32))
    penalty = pair_penalty(pools, dp)
    n = 3
    history = pooled.learn(problem, pools, pool_of, n, 0.01, dp)
    what = f'{name} dp {dp} threshold {threshold}'
    ctx.set_exact_additions(True)
    try:
        want = ctx.em_pools(n, 0.01, pools, pool_of, dp != 0, penalty)
        want_dense, want_betas = ctx.get_probs(), ctx.get_learnt_betas()
        got = ctx.em_doublets(n, 0.01, pools, pool_of, dp != 0, penalty, threshold)
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), f'{what}: {key} against dmx_em_pools'
        fio.assert_bitwise(ctx.get_probs(), want_dense, f'{what}: get_probs() against dmx_em_pools')
        fio.assert_bitwise(ctx.get_learnt_betas(), want_betas, f'{what}: learnt betas against dmx_em_pools')
        restated.assert_same(got, history[-1], f'{what}: the restatement')
        fio.assert_bitwise(got['addition'], history[-1]['addition'], f'{what}: addition')
        fio.assert_bitwise(ctx.get_learnt_betas(), pooled.learnt_betas(problem, history), f'{what}: learnt betas')
        for it, (step, addition) in enumerate(staged(ctx, n, 0.01, pools, pool_of, dp != 0, penalty, threshold)):
            assert_iteration(ctx, step, history[it], f'{what}: step-wise iteration {it}', addition)
        for key in ('logits', 'probs', 'best_option', 'best_prob', 'doublet_mass'):
            assert step[key].tobytes() == want[key].tobytes(), f'{what}: step-wise {key} against dmx_em_pools'
        fio.assert_bitwise(ctx.get_learnt_betas(), want_betas, f'{what}: step-wise learnt betas against dmx_em_pools')
    finally:
        ctx.apply_environment()


def test_another_power_without_credited_pairs_is_the_pooled_loop_to_float32_accuracy():
    """dmx_mstep raises to another power than 2 with powf, this M-step with the float64 pow rounded once: each weight
    within 1 ulp and half an ulp of the true power, sums of non-negative terms, two final roundings - 2.5 * 2^-23 relative."""
    name = 'f3_small_3.npz'
    ctx = learner(name)
    B, G = ctx.B, ctx.G
    pools, pool_of, penalty = [list(range(G))], np.zeros(B, np.int32), pair_penalty([list(range(G))], 0.35)
    ctx.set_exact_additions(True)
    try:
        want = ctx.em_pools(2, 0.01, pools, pool_of, True, penalty, contribution_power=1.5)
        got = ctx.em_doublets(2, 0.01, pools, pool_of, True, penalty, 2.0, contribution_power=1.5)
    finally:
        ctx.apply_environment()
    assert want['addition'].any()
    np.testing.assert_allclose(got['addition'], want['addition'], rtol=2.5 * 2.0 ** -23, atol=0)


# ---- 2. kernel-shape edges ---------------------------------------------------------------------------------------
SHAPES = [(2, 2., 1e-6), (63, 2., 1e-6), (64, 2., 1e-6), (65, 2., 1e-6), (130, 2., 1e-6), (65, 1.5, 1e-3), (130, 1.5, 1e-3), (130, 2., 1e-3)]


@pytest.mark.parametrize('G, power, threshold', SHAPES)
def test_kernel_shape_edges(G, power, threshold):
    from demuxalot_amd.device import DeviceContext
    problem = problems.shape_problem(G)
    pools, pool_of, B = problem['pools'], problem['pool_of'], problem['B']
    lengths = np.bincount(problem['cb'], minlength=B)
    assert lengths[0] == 0 and pool_of[1] == -1 and {1, 8, 9, 16, 65, 513} <= set(lengths.tolist())
    assert (np.bincount(problem['v'], minlength=len(problem['betas'])) == 0).any(), 'a variant without calls'
    if G == 130:
        assert {63, 64, 127, 128} <= set(pools[0]), 'a pool whose donors straddle the columns 63 | 64 and 127 | 128'
    n, dp = 3, 0.35
    penalty = pair_penalty(pools, dp)
    history = learning.learn(problem, pools, pool_of, n, 0.01, dp, threshold=threshold, power=power)
    live = np.array([learning.live_pairs(rec, pools, pool_of, True, threshold) for rec in history[:-1]])
    print(f'G = {G}: live pairs per barcode up to {live.max()}, {int(live.sum())} in all; rows up to {np.diff(history[0]["row_ptr"]).max()} options')
    if G >= 13:
        assert lengths[2] == 1 and pool_of[2] == 2 and len(pools[2]) == 12
        if threshold == 1e-6:
            assert (live[:, 2] == 66).all(), 'the one-call barcode of the 12-donor pool: every pair is live, two trips of 64 entries'
            assert live.max() > 64 and len(pools[0]) * (len(pools[0]) - 1) // 2 > 64
    plain = pooled.learn(problem, pools, pool_of, 2, 0.01, dp, power=power)
    assert not np.array_equal(plain[1]['addition'], history[1]['addition']), 'a plain M-step would pass otherwise'
    with DeviceContext(0) as ctx:
        install_designed(ctx, problem)
        got = ctx.em_doublets(n, 0.01, pools, pool_of, True, penalty, threshold, contribution_power=power)
        assert_iteration(ctx, got, history[-1], f'G = {G}', got['addition'])
        if G > 2:
            nobody = got['addition'][:, 1]
            assert not nobody.any() and not np.signbit(nobody).any(), 'a donor in no pool: exactly +0'
        assert got['addition'][:, 0].any()
        for it, (step, addition) in enumerate(staged(ctx, n, 0.01, pools, pool_of, True, penalty, threshold, power)):
            assert_iteration(ctx, step, history[it], f'G = {G}: staged iteration {it}', addition)


# ---- 3. + 4. pair posteriors of exactly 1 beside an empty bitmap row; variants of several work items ---------------
TIE_THRESHOLD = 0.5


@functools.lru_cache(maxsize=None)
def restated_tie():
    p = problems.tie_problem()
    B, (V, G) = p['B'], p['prob'].shape
    rows = restated.Restatement(p['v'], p['cb'], p['e'], p['prob'], B, 0.35)(p['pools'], p['pool_of'])
    dense = pooled.dense_singlets(rows, p['pools'], p['pool_of'], B, G)
    args = (p['v'], p['cb'], p['e'], dense, rows, p['pools'], p['pool_of'], True, p['prob'])
    in_order = learning.doublet_addition(*args, threshold=TIE_THRESHOLD)
    of_partials = learning.doublet_addition_of_items(*args, item_calls=1024, threshold=TIE_THRESHOLD)
    return p, rows, dense, in_order, of_partials


@functools.lru_cache(maxsize=None)
def tie_on_device():
    """(the context after the E-step and the crediting M-step of the designed problem, the E-step's dict, the addition)"""
    from demuxalot_amd.device import DeviceContext
    p = problems.tie_problem()
    B, (V, G) = p['B'], p['prob'].shape
    ctx = DeviceContext(0)
    ctx.set_problem(B, V, G, p['v'], p['cb'], p['e'], p['v2snp'])
    ctx.set_probs(p['prob'])
    penalty = pair_penalty(p['pools'], 0.35)
    got = ctx.estep_pools(p['pools'], p['pool_of'], True, penalty, resident=True)
    addition = ctx.mstep_doublets(p['pools'], p['pool_of'], True, penalty, got['probs'], TIE_THRESHOLD)
    return ctx, got, addition


def test_a_barcode_without_live_singlets_is_credited_through_its_pair():
    p, rows, dense, in_order, _of_partials = restated_tie()
    doublets = p['doublets']
    assert (dense[doublets] <= learning.live_floor(2.)).all(), "the doublets' bitmap rows are empty"
    assert (rows['probs'].reshape(p['B'], 3)[doublets, 2] == 1).all(), 'their pair posterior is exactly 1'
    only = np.setdiff1d(p['v'][np.isin(p['cb'], doublets)], p['v'][~np.isin(p['cb'], doublets)])
    assert len(only) == 0, 'every variant the doublets call is called by others too'
    without = learning.doublet_addition(p['v'], p['cb'], p['e'], dense, rows, p['pools'], p['pool_of'], True, p['prob'], threshold=2.0)
    assert (in_order > without).sum() > 100, 'the credited calls move many sums'
    ctx, got, addition = tie_on_device()
    restated.assert_same(got, rows, 'the E-step of the designed problem')
    fio.assert_bitwise(ctx.get_probs(), dense, 'its dense posteriors')
    fio.assert_bitwise(addition, in_order, 'the additions, calls of barcodes with an empty bitmap row among them')


def test_variants_of_several_work_items_are_summed_in_call_order():
    p, _rows, _dense, in_order, of_partials = restated_tie()
    V = len(p['prob'])
    calls_of = np.bincount(p['v'], minlength=V)
    assert len(p['v']) < 6000 * 1024 and (calls_of[p['hot']] > 2 * 1024).all(), 'three work items of 1024 calls per hot variant'
    hot_doublet = np.isin(p['v'], p['hot']) & np.isin(p['cb'], p['doublets'])
    assert hot_doublet.sum() > 20000, 'credited calls in the variants of several work items'
    differ = np.argwhere(in_order != of_partials)
    print(f'sums whose float32 depends on the order of the additions: {differ.tolist()}')
    assert len(differ) >= 1 and set(differ[:, 0]) <= set(p['hot'].tolist()), 'the problem decides between the two summation orders'
    ctx, _got, addition = tie_on_device()
    fio.assert_bitwise(addition, in_order, 'the additions, variants of three work items among them')
    assert ctx.redo_count() >= len(differ), 'the sums at a rounding boundary were redone in call order'


def test_both_weighted_forms_agree_where_their_weights_do():
    """With no live pair the crediting M-step, and at fraction 0 the M-step under ambient fractions (the table has no zero entry: r is
    exactly 1), are the plain float64 M-step of the dense posteriors: one combining rule (csrc/mstep_weighted.hip), so the same sums
    queued and the same bits from both."""
    p, rows, dense, _in_order, _of_partials = restated_tie()
    assert (p['prob'] != 0).all(), 'a zero table entry would make r of the ambient form 0'
    without = learning.doublet_addition(p['v'], p['cb'], p['e'], dense, rows, p['pools'], p['pool_of'], True, p['prob'], threshold=2.0)
    ctx, got, _addition = tie_on_device()
    penalty = pair_penalty(p['pools'], 0.35)
    uncredited = ctx.mstep_doublets(p['pools'], p['pool_of'], True, penalty, got['probs'], min_pair_posterior=2.0)
    redone = ctx.redo_count()
    fio.assert_bitwise(uncredited, without, 'the crediting M-step without a live pair')
    at_zero = ctx.mstep_ambient(np.zeros(p['B'], np.float32))
    fio.assert_bitwise(at_zero, without, 'the M-step under ambient fractions at fraction 0')
    print(f'sums redone in call order: {redone} and {ctx.redo_count()}')
    assert ctx.redo_count() == redone, 'both forms queue the same sums'
    ctx.mstep_doublets(p['pools'], p['pool_of'], True, penalty, got['probs'], TIE_THRESHOLD, fetch=False)  # (the shared context as tie_on_device left it)


# ---- 5. the fused loop is the step-wise one; the context survives ------------------------------------------------
def test_fused_equals_stepwise_and_the_context_survives():
    from demuxalot_amd.device import DeviceContext
    pool_of = pool_of_f1()
    penalty = pair_penalty(POOLS_F1, 0.35)
    problem = pooled.fixture_learning_problem(F1)
    V, G = problem['betas'].shape
    history = learning.learn(problem, POOLS_F1, pool_of, 3, 0.01, 0.35)
    assert learning.live_pairs(history[1], POOLS_F1, pool_of, True, 1e-3).any()
    with DeviceContext(0) as fused, DeviceContext(0) as stepwise:
        for ctx in (fused, stepwise):
            install(ctx, F1)
            ctx.set_exact_additions(True)  # (for dmx_mstep and dmx_em_pools below; the crediting M-step has one arithmetic)
        got = fused.em_doublets(3, 0.01, POOLS_F1, pool_of, True, penalty)
        assert_iteration(fused, got, history[-1], 'fused', got['addition'])
        *_, (want, addition) = staged(stepwise, 3, 0.01, POOLS_F1, pool_of, True, penalty, 1e-3)
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), key
        fio.assert_bitwise(got['addition'], addition, 'addition')
        fio.assert_bitwise(fused.get_probs(), stepwise.get_probs(), 'get_probs()')
        fio.assert_bitwise(fused.get_learnt_betas(), stepwise.get_learnt_betas(), 'learnt betas')
        fio.assert_bitwise(fused.get_learnt_betas(), learning.learnt_betas(problem, history), 'learnt betas against the restatement')
        # dmx_mstep on the posteriors the E-step left is the plain M-step of that dense matrix: a full pass, nothing kept from the crediting one
        dense = stepwise.get_probs()
        for ctx in (fused, stepwise):
            fio.assert_bitwise(ctx.mstep(), restated.demux_oracle.beta_addition(problem['v'], problem['cb'], problem['e'], dense, V, G), 'dmx_mstep')
        again = fused.em_pools(2, 0.01, POOLS_F1, pool_of, True, penalty)
        plain = pooled.learn(problem, POOLS_F1, pool_of, 2, 0.01, 0.35)
        restated.assert_same(again, plain[-1], 'em_pools afterwards')


# ---- 6. refusals -------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from demuxalot_amd._lib import DemuxHipError
    from demuxalot_amd.device import DeviceContext
    name = 'f3_small_1.npz'
    problem = pooled.fixture_learning_problem(name)
    B, (V, G) = problem['B'], problem['betas'].shape
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    penalty = pair_penalty(pools, 0.35)

    def changed(array, at, value):
        out = array.copy()
        out[at] = value
        return out

    with DeviceContext(0) as ctx:
        install(ctx, name)
        good = ctx.em_doublets(2, 0.01, pools, pool_of, True, penalty)
        rows = good['probs']
        dense, betas = ctx.get_probs(), ctx.get_learnt_betas()

        def launches():
            timings = ctx.timings()
            return tuple(timings[phase]['launches'] for phase in ('pstep', 'estep', 'mstep', 'mcombine'))

        before = launches()
        em = lambda **kw: ctx.em_doublets(**{**dict(n_iterations=2, p_genotype_clip=0.01, pools=pools, pool_of_barcode=pool_of, with_doublets=True,  # noqa: E731
                                                    pair_penalty=penalty), **kw})
        mstep = lambda post_rows=rows, pools=pools, **kw: ctx.mstep_doublets(pools, pool_of, True, penalty, post_rows, **kw)  # noqa: E731
        cases = [
            (lambda: em(n_iterations=0), r'dmx_em_doublets.*n_iterations.*status -1'),
            (lambda: em(contribution_power=0.0), r'power.*status -1'),
            (lambda: em(contribution_power=float('nan')), r'power.*status -1'),
            (lambda: em(contribution_power=float('inf')), r'power.*status -1'),
            (lambda: em(min_pair_posterior=0.0), r'min_pair_posterior.*status -1'),
            (lambda: em(min_pair_posterior=-1e-3), r'min_pair_posterior.*status -1'),
            (lambda: em(min_pair_posterior=float('nan')), r'min_pair_posterior.*status -1'),
            (lambda: em(min_pair_posterior=float('inf')), r'min_pair_posterior.*status -1'),
            (lambda: em(pools=[[0, 0]]), r'status -1'),
            (lambda: em(pool_of_barcode=changed(pool_of, 2, 5)), r'status -1'),
            (lambda: mstep(contribution_power=-2.0), r'dmx_mstep_doublets.*power.*status -1'),
            (lambda: mstep(min_pair_posterior=0.0), r'dmx_mstep_doublets.*min_pair_posterior.*status -1'),
            (lambda: mstep(rows[:-1]), r'dmx_mstep_doublets.*length.*status -1'),
            (lambda: mstep(np.concatenate([rows, rows[:1]])), r'dmx_mstep_doublets.*length.*status -1'),
            (lambda: mstep(changed(rows, 3, np.nan)), r'dmx_mstep_doublets.*posterior of the rows.*index 3.*status -1'),
            (lambda: mstep(changed(rows, len(rows) - 1, 1.5)), r'dmx_mstep_doublets.*posterior of the rows.*status -1'),
            (lambda: mstep(changed(rows, 0, -0.25)), r'dmx_mstep_doublets.*posterior of the rows.*status -1'),
            (lambda: mstep(pools=[[0, 0]]), r'dmx_mstep_doublets.*status -1'),
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
    with DeviceContext(0) as ctx:  # call order: nothing, a problem, a table, posteriors
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_doublets.*problem.*status -1'):
            ctx.B, ctx.V, ctx.G = B, V, G
            ctx.mstep_doublets(pools, pool_of, True, penalty, rows)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_doublets.*genotype probabilities.*status -1'):
            ctx.mstep_doublets(pools, pool_of, True, penalty, rows)
        with pytest.raises(DemuxHipError, match=r'dmx_em_doublets.*status -1'):
            ctx.em_doublets(2, 0.01, pools, pool_of, True, penalty)
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_doublets.*E-step.*status -1'):
            ctx.mstep_doublets(pools, pool_of, True, penalty, rows)
        assert all(ctx.timings()[phase]['launches'] == 0 for phase in ('estep', 'mstep', 'mcombine'))
    with DeviceContext(0) as ctx:
        ctx.comm_init_emulated(0, 1)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        ctx.estep(np.zeros(G, np.float32), False)
        for call in (lambda: ctx.em_doublets(2, 0.01, pools, pool_of, True, penalty),
                     lambda: ctx.mstep_doublets(pools, pool_of, True, penalty, rows)):
            with pytest.raises(DemuxHipError, match=r'communicator.*status -5'):
                call()
    from demuxalot_amd import Demultiplexer
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='min_pair_posterior'):
            Demultiplexer.learn_genotypes_from_doublets({}, None, None, min_pair_posterior=bad)


# ---- 7. end to end (exact_mode: the pooled loop in the exact arithmetic, what the loop without credited pairs is compared with) ---
def test_learn_genotypes_from_doublets_end_to_end(exact_mode):
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    problem, sim, plain, history = learning.simulated(0)
    # (genotypes with the problem's betas and default prior 0: the prior betas of the learning loop are then those betas themselves)
    calls, genotypes, handler = helpers.user_inputs(sim, problem['betas'], default_prior=0.0)
    B, G = sim['B'], sim['prob'].shape[1]
    K = G * (G + 1) // 2
    barcodes, donors = handler.ordered_barcodes, list(genotypes.genotype_names)
    learnt, probs_df = Demultiplexer.learn_genotypes_from_doublets(calls, genotypes, handler)
    assert list(probs_df.index) == barcodes and list(probs_df.columns)[:G] == donors and probs_df.shape == (B, K) and probs_df.values.dtype == np.float32
    fio.assert_bitwise(probs_df.values, history[-1]['probs'].reshape(B, K), 'the last posteriors')
    fio.assert_bitwise(learnt.variant_betas, learning.learnt_betas(problem, history), 'learnt betas')
    assert learnt.genotype_names == genotypes.genotype_names and learnt is not genotypes
    # does it help?  what the device learnt, against the plain loop's error as the restatement states it
    table = restated.demux_oracle.probs_from_betas(sim['v2snp'], learnt.variant_betas, 0.01)
    learning.value_condition(learning.table_error(plain[-1]['prob_table'], sim), learning.table_error(table, sim), probs_df.values.argmax(axis=1), sim)
    # the generator: every iteration, the same last one, and it may be closed early
    generator = Demultiplexer.staged_genotype_learning_from_doublets(calls, genotypes, handler)
    for it, (step, debug) in enumerate(generator):
        fio.assert_bitwise(step.values, history[it]['probs'].reshape(B, K), f'generator, iteration {it}: posteriors')
        fio.assert_bitwise(debug['genotype_addition'], history[it]['addition'], f'generator, iteration {it}: addition')
        fio.assert_bitwise(debug['genotype_prior'], problem['betas'], 'generator: prior betas')
    assert it == 4 and step.values.tobytes() == probs_df.values.tobytes()
    early = Demultiplexer.staged_genotype_learning_from_doublets(calls, genotypes, handler)
    first, _debug = next(early)
    early.close()
    fio.assert_bitwise(first.values, history[0]['probs'].reshape(B, K), 'generator closed after its first iteration')
    # with pools: the restatement's bits; no credited pair: learn_genotypes_in_pools
    pool2donors = {'low': donors[:5][::-1], 'high': donors[3:]}
    barcode2pool = {bc: (None if b % 7 == 0 else 'low' if b % 2 else 'high') for b, bc in enumerate(barcodes)}
    pools = [list(range(5)), list(range(3, G))]
    pool_of = np.array([-1 if b % 7 == 0 else 0 if b % 2 else 1 for b in range(B)], dtype=np.int32)
    pooled_history = learning.learn(problem, pools, pool_of, 3, 0.01, 0.35, threshold=1e-2)
    got_learnt, got = Demultiplexer.learn_genotypes_from_doublets(calls, genotypes, handler, n_iterations=3, min_pair_posterior=1e-2,
                                                                  barcode2pool=barcode2pool, pool2donors=pool2donors)
    assert isinstance(got, PooledPosteriors)
    for key in ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass'):
        assert getattr(got, key).tobytes() == pooled_history[-1][key].tobytes(), f'with pools against the restatement: {key}'
    fio.assert_bitwise(got_learnt.variant_betas, learning.learnt_betas(problem, pooled_history), 'with pools: learnt betas')
    for it, (step, debug) in enumerate(Demultiplexer.staged_genotype_learning_from_doublets(calls, genotypes, handler, n_iterations=3, min_pair_posterior=1e-2,
                                                                                           barcode2pool=barcode2pool, pool2donors=pool2donors)):
        assert step.probs.tobytes() == pooled_history[it]['probs'].tobytes(), f'generator with pools, iteration {it}'
        fio.assert_bitwise(debug['genotype_addition'], pooled_history[it]['addition'], f'generator with pools, iteration {it}: addition')
    assert step.probs.tobytes() == got.probs.tobytes()
    want_learnt, want = Demultiplexer.learn_genotypes_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, n_iterations=3, doublet_prior=0.35)
    same_learnt, same = Demultiplexer.learn_genotypes_from_doublets(calls, genotypes, handler, n_iterations=3, min_pair_posterior=2.0,
                                                                    barcode2pool=barcode2pool, pool2donors=pool2donors)
    assert same.pools == want.pools
    for key in ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass'):
        assert getattr(same, key).tobytes() == getattr(want, key).tobytes(), f'no credited pair against learn_genotypes_in_pools: {key}'
    fio.assert_bitwise(same_learnt.variant_betas, want_learnt.variant_betas, 'no credited pair against learn_genotypes_in_pools: learnt betas')
