"""Learning under per-barcode ambient fractions on the GPU (include/demux_hip_debug.h: dmx_estep_ambient_resident, dmx_mstep_ambient,
dmx_em_ambient; csrc/mstep_ambient.hip, the DENSE form of csrc/estep_ambient.hip; Demultiplexer.learn_genotypes_with_ambient,
staged_genotype_learning_with_ambient).

Everything is compared bit for bit with tests/ambient_learning_restatement.py - the pooled loop with the E-step under the fractions and
the weighted M-step, proven in tests/test_ambient_learning_cpu.py to be the pooled loop itself at fraction 0 - and, at fraction 0, with
dmx_em_pools under exact additions on the same context."""
import functools

import numpy as np
import pytest

from tests import ambient_learning_problems as problems
from tests import ambient_learning_restatement as learning
from tests import ambient_restatement
from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests import pools_learning_restatement as pooled
from tests import pools_restatement as restated
from tests.pooled_helpers import assert_iteration, exact_mode, install, install_designed, pair_penalty, pool_of_f1  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1, SMALL, POOLS_F1 = helpers.F1, helpers.F3_SMALL, helpers.POOLS_F1  # f1: G = 20, B = 1000
FRACTIONS = np.array([0.0, 0.1, 0.37, 0.63, 1.0, 0.0, 0.25], dtype=np.float32)  # 0, grid values and exactly 1
learner = functools.lru_cache(maxsize=None)(helpers.new_learner)  # a fixture installed for learning, the contexts this module's own


def fractions(B, shift=0):
    return FRACTIONS[(np.arange(B) + shift) % len(FRACTIONS)].copy()


def staged(ctx, n, clip, pools, pool_of, with_doublets, penalty, alpha, soup, power=2.):
    """The step-wise path under the fractions: the resident ambient E-step, dmx_mstep_ambient behind it."""
    return helpers.staged(ctx, n, clip, lambda: ctx.estep_ambient(pools, pool_of, with_doublets, penalty, alpha, clip, ambient=soup, resident=True),
                          lambda _out: ctx.mstep_ambient(alpha, power, clip, ambient=soup))


# ---- 1. every fraction 0: dmx_em_pools with exact additions, and the restatement ---------------------------------
@pytest.mark.parametrize('dp', [0.0, 0.35])
@pytest.mark.parametrize('name', SMALL + ['f2_synthetic_g4.npz', F1])
def test_zero_fractions_are_the_pooled_loop(name, dp):
    ctx = learner(name)
    problem = pooled.fixture_learning_problem(name)
    B, G = ctx.B, ctx.G
    pools, pool_of = (POOLS_F1, pool_of_f1()) if name == F1 else ([list(range(G))], np.zeros(B, np.int32))
    penalty = pair_penalty(pools, dp)
    n = 3
    history = pooled.learn(problem, pools, pool_of, n, 0.01, dp)
    ctx.set_exact_additions(True)
    try:
        want = ctx.em_pools(n, 0.01, pools, pool_of, dp != 0, penalty)
        want_dense, want_betas = ctx.get_probs(), ctx.get_learnt_betas()
        got = ctx.em_ambient(n, 0.01, pools, pool_of, dp != 0, penalty, np.zeros(B, np.float32))
    finally:
        ctx.apply_environment()
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), f'{name} dp {dp}: {key} against dmx_em_pools'
    fio.assert_bitwise(ctx.get_probs(), want_dense, f'{name} dp {dp}: get_probs() against dmx_em_pools')
    fio.assert_bitwise(ctx.get_learnt_betas(), want_betas, f'{name} dp {dp}: learnt betas against dmx_em_pools')
    restated.assert_same(got, history[-1], f'{name} dp {dp}: the restatement')
    fio.assert_bitwise(got['addition'], history[-1]['addition'], f'{name} dp {dp}: addition')
    fio.assert_bitwise(ctx.get_learnt_betas(), pooled.learnt_betas(problem, history), f'{name} dp {dp}: learnt betas')


# ---- 2. mixed fractions ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_mixed(name, with_pools, dp, n, power, supplied):
    problem = pooled.fixture_learning_problem(name)
    B, (V, G) = problem['B'], problem['betas'].shape
    if with_pools and name == F1:
        pools, pool_of = POOLS_F1, pool_of_f1()
    elif with_pools:
        pools, pool_of = [list(range(G - 1)), list(range(1, G)), [0, G - 1]], ((np.arange(B) % 4) - 1).astype(np.int32)
    else:
        pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    if supplied:
        soup = np.random.default_rng(7).uniform(0, 1, size=V).astype(np.float32)
        soup[::17], soup[5::17] = 0.0, 1.0
    else:
        soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    alpha = fractions(B)
    history = learning.learn(problem, pools, pool_of, alpha, soup, n, 0.01, dp, power=power)
    for rec in history:
        for value in rec.values():
            value.flags.writeable = False
    return problem, pools, pool_of, alpha, soup, history


# (a power other than 2 is f32(pow(f64(base), f64(power))) on both sides: a float32 `**` is no reference of bits - DESIGN.md 4.9)
MIXED = [
    (F1, True, 0.35, 2, 2., False),
    (F1, False, 0.0, 4, 2., True),
    (F1, True, 0.0, 2, 1.5, True),
    ('f3_small_0.npz', False, 0.0, 2, 2., False),
    ('f3_small_1.npz', False, 0.35, 4, 1.5, False),
    ('f3_small_2.npz', True, 0.35, 4, 2., True),
    ('f3_small_3.npz', True, 0.0, 2, 1.5, True),
    ('f3_small_3.npz', False, 0.35, 2, 2., False),
]


@pytest.mark.parametrize('name, with_pools, dp, n, power, supplied', MIXED)
def test_mixed_fractions(name, with_pools, dp, n, power, supplied):
    problem, pools, pool_of, alpha, soup, history = restated_mixed(name, with_pools, dp, n, power, supplied)
    what = f'{name} pools {with_pools} dp {dp} n {n} power {power} supplied {supplied}'
    assert np.isfinite(history[-1]['addition']).all() and (alpha == 1).any() and (alpha == 0).any()
    plain = pooled.learn(problem, pools, pool_of, 2, 0.01, dp, power=power)
    assert not np.array_equal(plain[1]['addition'], history[1]['addition']), 'a plain M-step behind the ambient E-step would pass otherwise'
    ctx = learner(name)
    penalty = pair_penalty(pools, dp)
    got = ctx.em_ambient(n, 0.01, pools, pool_of, dp != 0, penalty, alpha, ambient=soup if supplied else None, contribution_power=power)
    assert_iteration(ctx, got, history[-1], what, got['addition'])
    fio.assert_bitwise(ctx.get_learnt_betas(), learning.learnt_betas(problem, history), f'{what}: learnt betas')


# ---- 3. kernel-shape edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', [1, 63, 64, 65, 130])
def test_kernel_shape_edges(G):
    from demuxalot_amd.device import DeviceContext
    problem = problems.shape_problem(G)
    pools, pool_of, alpha, B = problem['pools'], problem['pool_of'], problem['alpha'], problem['B']
    lengths = np.bincount(problem['cb'], minlength=B)
    assert lengths[0] == 0 and pool_of[1] == -1 and {1, 8, 9, 16, 65, 513} <= set(lengths.tolist())
    assert (np.bincount(problem['v'], minlength=len(problem['betas'])) == 0).any(), 'a variant without calls'
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    history = learning.learn(problem, pools, pool_of, alpha, soup, 3, 0.01, 0.0)
    with DeviceContext(0) as ctx:
        install_designed(ctx, problem)
        got = ctx.em_ambient(3, 0.01, pools, pool_of, False, [0.0, 0.0], alpha)
        assert_iteration(ctx, got, history[-1], f'G = {G}', got['addition'])
        if G > 1:
            nobody = got['addition'][:, G - 1]
            assert not nobody.any() and not np.signbit(nobody).any(), 'a donor in no pool: exactly +0'
        assert got['addition'][:, 0].any()
        for it, (step, addition) in enumerate(staged(ctx, 3, 0.01, pools, pool_of, False, [0.0, 0.0], alpha, None)):
            assert_iteration(ctx, step, history[it], f'G = {G}: staged iteration {it}', addition)


# ---- 4. variants of several work items ---------------------------------------------------------------------------
def test_variants_of_several_work_items_are_summed_in_call_order():
    from demuxalot_amd.device import DeviceContext
    p = problems.tie_problem()
    B, (V, G) = p['B'], p['prob'].shape
    calls_of = np.bincount(p['v'], minlength=V)
    assert len(p['v']) < 6000 * 1024 and (calls_of[p['hot']] > 2 * 1024).all(), 'three work items of 1024 calls per hot variant'
    rows = learning.scoring.restate(p['v'], p['cb'], p['e'], p['prob'], B, p['pools'], p['pool_of'], np.zeros(1, np.float32), False, p['alpha'], p['soup'])
    dense = pooled.dense_singlets(rows, p['pools'], p['pool_of'], B, G)
    args = (p['v'], p['cb'], p['e'], dense, p['prob'], p['alpha'], p['soup'])
    in_order = learning.ambient_addition(*args)
    of_partials = learning.ambient_addition_of_items(*args, item_calls=1024)
    differ = np.argwhere(in_order != of_partials)
    print(f'sums whose float32 depends on the order of the additions: {differ.tolist()}')
    assert len(differ) >= 1 and set(differ[:, 0]) <= set(p['hot'].tolist()), 'the problem decides between the two summation orders'
    with DeviceContext(0) as ctx:
        ctx.set_problem(B, V, G, p['v'], p['cb'], p['e'], p['v2snp'])
        ctx.set_probs(p['prob'])
        got = ctx.estep_ambient(p['pools'], p['pool_of'], False, [0.0], p['alpha'], ambient=p['soup'], resident=True)
        restated.assert_same(got, rows, 'the E-step of the designed problem')
        fio.assert_bitwise(ctx.get_probs(), dense, 'its dense posteriors')
        addition = ctx.mstep_ambient(p['alpha'], ambient=p['soup'])
        fio.assert_bitwise(addition, in_order, 'the additions, variants of three work items among them')
        assert ctx.redo_count() >= len(differ), 'the sums at a rounding boundary were redone in call order'


# ---- 5. the fused loop is the step-wise one; the context survives ------------------------------------------------
def test_fused_equals_stepwise_and_the_context_survives():
    from demuxalot_amd.device import DeviceContext
    fx = fio.load(F1)
    pool_of = pool_of_f1()
    penalty = pair_penalty(POOLS_F1, 0.35)
    alpha = fractions(1000, shift=3)
    with DeviceContext(0) as fused, DeviceContext(0) as stepwise:
        for ctx in (fused, stepwise):
            install(ctx, F1)
        got = fused.em_ambient(3, 0.01, POOLS_F1, pool_of, True, penalty, alpha)
        *_, (want, addition) = staged(stepwise, 3, 0.01, POOLS_F1, pool_of, True, penalty, alpha, None)
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), key
        fio.assert_bitwise(got['addition'], addition, 'addition')
        fio.assert_bitwise(fused.get_probs(), stepwise.get_probs(), 'get_probs()')
        fio.assert_bitwise(fused.get_learnt_betas(), stepwise.get_learnt_betas(), 'learnt betas')
        # dmx_mstep on the posteriors the resident ambient E-step left is the plain M-step of that dense matrix
        dense = stepwise.get_probs()
        problem = pooled.fixture_learning_problem(F1)
        V, G = problem['betas'].shape
        fio.assert_bitwise(stepwise.mstep(), restated.demux_oracle.beta_addition(problem['v'], problem['cb'], problem['e'], dense, V, G), 'dmx_mstep')
        # afterwards: dmx_em, dmx_estep + dmx_mstep and dmx_em_pools as if nothing had happened
        n = int(fx['em0_n_iterations'])
        assert float(fx['em0_dp']) == 0
        zeros = np.zeros(G, np.float32)
        _logits, probs, plain_addition = fused.em(n, float(fx['em0_clip']), zeros, False)
        fio.assert_bitwise(probs, fx[f'em0_it{n - 1}_probs'], 'em: probs')
        fio.assert_bitwise(plain_addition, fx[f'em0_it{n - 1}_addition'], 'em: addition')
        fio.assert_bitwise(fused.get_learnt_betas(), fx['em0_learnt_betas'], 'em: learnt betas')
        fused.set_addition(None)
        fused.probs_from_betas(float(fx['em0_clip']), fetch=False)
        _logits, probs = fused.estep(zeros, False)
        fio.assert_bitwise(probs, fx['em0_it0_probs'], 'estep: probs')
        fio.assert_bitwise(fused.mstep(), fx['em0_it1_addition'], 'mstep: addition')
        history = pooled.learn(problem, POOLS_F1, pool_of, 2, 0.01, 0.35)
        again = fused.em_pools(2, 0.01, POOLS_F1, pool_of, True, penalty)
        restated.assert_same(again, history[-1], 'em_pools afterwards')
        fio.assert_bitwise(again['addition'], history[-1]['addition'], 'em_pools afterwards: addition')


# ---- 6. refusals -------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from demuxalot_amd._lib import DemuxHipError
    from demuxalot_amd.device import DeviceContext
    name = 'f3_small_1.npz'
    problem = pooled.fixture_learning_problem(name)
    B, (V, G) = problem['B'], problem['betas'].shape
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    alpha = fractions(B)
    soup = np.full(V, 0.5, np.float32)

    def changed(array, at, value):
        out = array.copy()
        out[at] = value
        return out

    with DeviceContext(0) as ctx:
        install(ctx, name)
        good = ctx.em_ambient(2, 0.01, pools, pool_of, False, [0.0], alpha, ambient=soup)
        dense, betas = ctx.get_probs(), ctx.get_learnt_betas()

        def launches():
            timings = ctx.timings()
            return tuple(timings[phase]['launches'] for phase in ('pstep', 'estep', 'mstep', 'mcombine'))

        before = launches()
        em = lambda **kw: ctx.em_ambient(**{**dict(n_iterations=2, p_genotype_clip=0.01, pools=pools, pool_of_barcode=pool_of, with_doublets=False,  # noqa: E731
                                                   pair_penalty=[0.0], alpha=alpha, ambient=soup), **kw})
        cases = [
            (lambda: em(n_iterations=0), r'n_iterations.*status -1'),
            (lambda: em(contribution_power=0.0), r'power.*status -1'),
            (lambda: em(contribution_power=-2.0), r'power.*status -1'),
            (lambda: em(contribution_power=float('nan')), r'power.*status -1'),
            (lambda: em(contribution_power=float('inf')), r'power.*status -1'),
            (lambda: em(alpha=changed(alpha, 3, 1.5)), r'alpha of a barcode.*status -1'),
            (lambda: em(alpha=changed(alpha, B - 1, np.nan)), r'alpha of a barcode.*status -1'),
            (lambda: em(ambient=changed(soup, 2, -0.25)), r'ambient value.*status -1'),
            (lambda: em(ambient=changed(soup, V - 1, np.inf)), r'ambient value.*status -1'),
            (lambda: em(pools=[[0, 0]]), r'status -1'),
            (lambda: ctx.mstep_ambient(alpha, contribution_power=0.0, ambient=soup), r'dmx_mstep_ambient.*power.*status -1'),
            (lambda: ctx.mstep_ambient(changed(alpha, 0, 2.0), ambient=soup), r'dmx_mstep_ambient.*alpha of a barcode.*status -1'),
            (lambda: ctx.mstep_ambient(alpha, ambient=changed(soup, 0, np.nan)), r'dmx_mstep_ambient.*ambient value.*status -1'),
            (lambda: ctx.estep_ambient(pools, pool_of, False, [0.0], changed(alpha, 1, -0.5), ambient=soup, resident=True),
             r'dmx_estep_ambient_resident.*alpha of a barcode.*status -1'),
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
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_ambient.*problem.*status -1'):
            ctx.B, ctx.V, ctx.G = B, V, G
            ctx.mstep_ambient(alpha, ambient=soup)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_ambient.*genotype probabilities.*status -1'):
            ctx.mstep_ambient(alpha, ambient=soup)
        with pytest.raises(DemuxHipError, match=r'dmx_em_ambient.*status -1'):
            ctx.em_ambient(2, 0.01, pools, pool_of, False, [0.0], alpha)
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_ambient.*E-step.*status -1'):
            ctx.mstep_ambient(alpha, ambient=soup)
        assert all(ctx.timings()[phase]['launches'] == 0 for phase in ('estep', 'mstep', 'mcombine'))
    with DeviceContext(0) as ctx:
        ctx.comm_init_emulated(0, 1)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        ctx.estep(np.zeros(G, np.float32), False)
        for call in (lambda: ctx.em_ambient(2, 0.01, pools, pool_of, False, [0.0], alpha),
                     lambda: ctx.mstep_ambient(alpha, ambient=soup),
                     lambda: ctx.estep_ambient(pools, pool_of, False, [0.0], alpha, resident=True)):
            with pytest.raises(DemuxHipError, match=r'communicator.*status -5'):
                call()


# ---- 7. end to end (exact_mode: the pooled loop in the exact arithmetic, what the loop at fraction 0 is compared with) ------------
def test_learn_genotypes_with_ambient_end_to_end(exact_mode):
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    problem, sim = learning.simulated_problem(0)
    # (genotypes with the problem's betas and default prior 0: the prior betas of the learning loop are then those betas themselves)
    calls, genotypes, handler = helpers.user_inputs(sim, problem['betas'], default_prior=0.0)
    B, G = sim['B'], sim['prob'].shape[1]
    barcodes, donors = handler.ordered_barcodes, list(genotypes.genotype_names)
    alpha = sim['truth'].astype(np.float32)
    fractions_of = {bc: float(a) for bc, a in zip(barcodes, alpha)}
    history = learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), alpha, sim['soup'], 5, 0.01, 0.)
    learnt, probs_df = Demultiplexer.learn_genotypes_with_ambient(calls, genotypes, handler, fractions_of, ambient=sim['soup'])
    assert list(probs_df.index) == barcodes and list(probs_df.columns) == donors and probs_df.values.dtype == np.float32
    fio.assert_bitwise(probs_df.values, history[-1]['probs'].reshape(B, G), 'the last posteriors')
    fio.assert_bitwise(learnt.variant_betas, learning.learnt_betas(problem, history), 'learnt betas')
    assert learnt.genotype_names == genotypes.genotype_names and learnt is not genotypes
    # the value condition, on what the device learnt: the table of the learnt betas against the plain loop's
    plain_learnt, plain_probs = Demultiplexer.learn_genotypes(calls, genotypes, handler)
    table = lambda betas: restated.demux_oracle.probs_from_betas(sim['v2snp'], betas, 0.01)  # noqa: E731
    error = lambda betas: float(np.abs(table(betas).astype(np.float64) - sim['prob']).mean())  # noqa: E731
    assert np.array_equal(plain_probs.values.argmax(axis=1), sim['donor1'])
    learning.value_condition(error(plain_learnt.variant_betas), error(learnt.variant_betas), probs_df.values.argmax(axis=1), sim)
    # the generator: every iteration, the same last one, and it may be closed early
    generator = Demultiplexer.staged_genotype_learning_with_ambient(calls, genotypes, handler, fractions_of, ambient=sim['soup'])
    for it, (step, debug) in enumerate(generator):
        fio.assert_bitwise(step.values, history[it]['probs'].reshape(B, G), f'generator, iteration {it}: posteriors')
        fio.assert_bitwise(debug['genotype_addition'], history[it]['addition'], f'generator, iteration {it}: addition')
        fio.assert_bitwise(debug['genotype_prior'], problem['betas'], 'generator: prior betas')
        fio.assert_bitwise(debug['ambient'], sim['soup'], 'generator: the soup profile')
    assert it == 4 and step.values.tobytes() == probs_df.values.tobytes()
    early = Demultiplexer.staged_genotype_learning_with_ambient(calls, genotypes, handler, fractions_of)
    first, debug = next(early)
    early.close()
    soup = ambient_restatement.derived_ambient(sim['v'], sim['v2snp'], 0.01)
    fio.assert_bitwise(debug['ambient'], soup, 'generator closed after its first iteration: the derived profile')
    derived = learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), alpha, soup, 1, 0.01, 0.)
    fio.assert_bitwise(first.values, derived[0]['probs'].reshape(B, G), 'generator closed after its first iteration')
    # every fraction 0: learn_genotypes_in_pools, with pools and doublets
    pool2donors = {'low': donors[:5][::-1], 'high': donors[3:]}
    barcode2pool = {bc: (None if b % 7 == 0 else 'low' if b % 2 else 'high') for b, bc in enumerate(barcodes)}
    want_learnt, want = Demultiplexer.learn_genotypes_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, n_iterations=3, doublet_prior=0.35)
    got_learnt, got = Demultiplexer.learn_genotypes_with_ambient(calls, genotypes, handler, {}, n_iterations=3, doublet_prior=0.35,
                                                                 barcode2pool=barcode2pool, pool2donors=pool2donors)
    assert isinstance(got, PooledPosteriors) and got.pools == want.pools
    for key in ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass'):
        assert getattr(got, key).tobytes() == getattr(want, key).tobytes(), f'fractions 0 against learn_genotypes_in_pools: {key}'
    fio.assert_bitwise(got_learnt.variant_betas, want_learnt.variant_betas, 'fractions 0 against learn_genotypes_in_pools: learnt betas')
