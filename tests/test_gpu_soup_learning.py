"""Learning the soup's allele profile on the GPU (include/demux_hip_debug.h: dmx_mstep_soup, dmx_em_ambient_soup; csrc/mstep_soup.hip;
Demultiplexer.learn_ambient_profile, learn_genotypes_and_ambient, staged_genotype_learning_and_ambient).

Everything is compared bit for bit with tests/soup_learning_restatement.py - the ambient learning loop with the profile replaced after
every iteration, proven in tests/test_soup_learning_cpu.py to be that loop itself under a fixed profile and the pooled loop at fraction
0 - and, at fraction 0, with dmx_em_pools under exact additions on the same context."""
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
from tests import soup_learning_problems
from tests import soup_learning_restatement as soup_learning
from tests.pooled_helpers import assert_iteration, exact_mode, install, install_designed, pair_penalty, pool_of_f1  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

F1, SMALL, POOLS_F1 = helpers.F1, helpers.F3_SMALL, helpers.POOLS_F1  # f1: G = 20, B = 1000
FRACTIONS = np.array([0.0, 0.1, 0.37, 0.63, 1.0, 0.0, 0.25], dtype=np.float32)  # 0, grid values and exactly 1
learner = functools.lru_cache(maxsize=None)(helpers.new_learner)  # a fixture installed for learning, the contexts this module's own


def fractions(B, shift=0):
    return FRACTIONS[(np.arange(B) + shift) % len(FRACTIONS)].copy()


def staged(ctx, n, clip, pools, pool_of, with_doublets, penalty, alpha, soup, power=2., pseudo_count=1.):
    """The step-wise path: the P-step, the resident ambient E-step with the current profile, then dmx_mstep_soup and dmx_mstep_ambient,
    both with the profile that E-step read.  Yields (E-step results with 'counts' and 'next_ambient' of the soup step behind it - run
    before the yield, as the restatement records them -, the addition the E-step's table was made with)."""
    state = dict(ambient=soup)

    def estep():
        out = ctx.estep_ambient(pools, pool_of, with_doublets, penalty, alpha, clip, ambient=state['ambient'], resident=True)
        before = ctx.get_probs()
        state['ambient'], counts = ctx.mstep_soup(alpha, pseudo_count, clip, ambient=out['ambient'])
        fio.assert_bitwise(ctx.get_probs(), before, 'dmx_mstep_soup leaves the posteriors')
        return dict(out, counts=counts, next_ambient=state['ambient'])

    return helpers.staged(ctx, n, clip, estep, lambda out: ctx.mstep_ambient(alpha, power, clip, ambient=out['ambient']))


def assert_soup_step(got, want, what):
    """The soup step behind an E-step: the totals and the profile formed from them."""
    fio.assert_bitwise(got['counts'], want['counts'], f'{what}: counts')
    fio.assert_bitwise(got['next_ambient'], want['next_ambient'], f'{what}: the new profile')


def assert_fused(ctx, got, history, what):
    """dmx_em_ambient_soup's results against the restatement's last iteration; counts_out: the totals the last profile was formed from."""
    assert_iteration(ctx, got, history[-1], what, got['addition'])
    counts = history[-2]['counts'] if len(history) > 1 else np.zeros_like(history[-1]['counts'])
    fio.assert_bitwise(got['counts'], counts, f'{what}: counts_out')


# ---- B1. kernel-shape edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', [1, 63, 64, 65, 130])
def test_kernel_shape_edges(G):
    from demuxalot_amd.device import DeviceContext
    problem = problems.shape_problem(G)
    pools, pool_of, alpha, B = problem['pools'], problem['pool_of'], problem['alpha'], problem['B']
    lengths = np.bincount(problem['cb'], minlength=B)
    assert lengths[0] == 0 and pool_of[1] == -1 and {1, 8, 9, 16, 65, 513} <= set(lengths.tolist())
    uncalled = np.bincount(problem['v'], minlength=len(problem['betas'])) == 0
    assert uncalled.any(), 'a variant without calls'
    assert (alpha == 0).any() and (alpha == 1).any()
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    history = soup_learning.learn(problem, pools, pool_of, alpha, soup, 3, 0.01, 0.0)
    assert history[0]['counts'].any() and not np.array_equal(history[0]['next_ambient'], soup)
    with DeviceContext(0) as ctx:
        install_designed(ctx, problem)
        # dmx_mstep_soup behind a resident ambient E-step, then the whole step-wise loop
        for it, (step, addition) in enumerate(staged(ctx, 3, 0.01, pools, pool_of, False, [0.0, 0.0], alpha, None)):
            assert_iteration(ctx, step, history[it], f'G = {G}: staged iteration {it}', addition)
            assert_soup_step(step, history[it], f'G = {G}: staged iteration {it}')
            nothing = step['counts'][uncalled]
            assert not nothing.any() and not np.signbit(nothing).any(), 'a variant without calls: total == +0'
        got = ctx.em_ambient_soup(3, 0.01, pools, pool_of, False, [0.0, 0.0], alpha)
        assert_fused(ctx, got, history, f'G = {G}')
        assert not got['counts'][uncalled].any() and not np.signbit(got['counts'][uncalled]).any()
        if G > 1:
            nobody = got['addition'][:, G - 1]
            assert not nobody.any() and not np.signbit(nobody).any(), 'a donor in no pool: exactly +0'


# ---- B2. variants of several work items --------------------------------------------------------------------------
def test_variants_of_several_work_items_are_summed_in_call_order():
    from demuxalot_amd.device import DeviceContext
    # ambient_learning_problems.tie_problem() does not decide between the two orders for this step: its hot sums are on no tie at power 1
    q = problems.tie_problem()
    rows = learning.scoring.restate(q['v'], q['cb'], q['e'], q['prob'], q['B'], q['pools'], q['pool_of'], np.zeros(1, np.float32), False, q['alpha'], q['soup'])
    q_args = (q['v'], q['cb'], q['e'], pooled.dense_singlets(rows, q['pools'], q['pool_of'], q['B'], 2), q['prob'], q['alpha'], q['soup'])
    undecided = np.array_equal(soup_learning.soup_counts(*q_args)[0], soup_learning.soup_counts_of_items(*q_args, item_calls=1024)[0])
    p = soup_learning_problems.tie_problem() if undecided else q
    B, (V, G) = p['B'], p['prob'].shape
    calls_of = np.bincount(p['v'], minlength=V)
    assert len(p['v']) < 6000 * 1024 and (calls_of[p['hot']] > 2 * 1024).all(), 'three work items of 1024 calls per hot variant'
    rows = learning.scoring.restate(p['v'], p['cb'], p['e'], p['prob'], B, p['pools'], p['pool_of'], np.zeros(1, np.float32), False, p['alpha'], p['soup'])
    dense = pooled.dense_singlets(rows, p['pools'], p['pool_of'], B, G)
    args = (p['v'], p['cb'], p['e'], dense, p['prob'], p['alpha'], p['soup'])
    in_order, total = soup_learning.soup_counts(*args)
    of_partials, total_of_partials = soup_learning.soup_counts_of_items(*args, item_calls=1024)
    differ = np.argwhere(in_order != of_partials)
    print(f'counts whose float32 depends on the order of the additions: {differ.tolist()}')
    assert len(differ) >= 1 and set(differ[:, 0]) <= set(p['hot'].tolist()), 'the problem decides between the two summation orders'
    assert not np.array_equal(total, total_of_partials), 'and the totals show it'
    with DeviceContext(0) as ctx:
        ctx.set_problem(B, V, G, p['v'], p['cb'], p['e'], p['v2snp'])
        ctx.set_probs(p['prob'])
        got = ctx.estep_ambient(p['pools'], p['pool_of'], False, [0.0], p['alpha'], ambient=p['soup'], resident=True)
        restated.assert_same(got, rows, 'the E-step of the designed problem')
        fio.assert_bitwise(ctx.get_probs(), dense, 'its dense posteriors')
        profile, counts = ctx.mstep_soup(p['alpha'], ambient=p['soup'])
        fio.assert_bitwise(counts, total, 'the totals, variants of three work items among them')
        fio.assert_bitwise(profile, soup_learning.profile_from_totals(total, p['v2snp'], 1., 0.01), 'the profile')
        assert ctx.redo_count() >= len(differ), 'the sums at a rounding boundary were redone in call order'


# ---- B3. the call leaves the context alone -----------------------------------------------------------------------
def test_the_soup_step_leaves_the_context_alone():
    from demuxalot_amd.device import DeviceContext
    pool_of = pool_of_f1()
    penalty = pair_penalty(POOLS_F1, 0.35)
    alpha = fractions(1000, shift=2)
    with DeviceContext(0) as ctx, DeviceContext(0) as other:
        for c in (ctx, other):
            install(c, F1)
            c.em_ambient(2, 0.01, POOLS_F1, pool_of, True, penalty, alpha)  # an addition, a table, posteriors
            c.probs_from_betas(0.01, fetch=False)
            c.estep_ambient(POOLS_F1, pool_of, True, penalty, alpha, resident=True)
        probs, addition, betas = ctx.get_probs(), ctx.get_addition(), ctx.get_learnt_betas()
        assert addition.any()
        profile, counts = ctx.mstep_soup(alpha)
        assert counts.any() and np.isfinite(profile).all()
        fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() around dmx_mstep_soup')
        fio.assert_bitwise(ctx.get_addition(), addition, 'the addition around dmx_mstep_soup')
        fio.assert_bitwise(ctx.get_learnt_betas(), betas, 'the learnt betas around dmx_mstep_soup')
        for power in (2., 1.5):
            fio.assert_bitwise(ctx.mstep_ambient(alpha, power), other.mstep_ambient(alpha, power), f'dmx_mstep_ambient behind it, power {power}')
        fio.assert_bitwise(ctx.mstep(), other.mstep(), 'dmx_mstep behind it')
        again, counts_again = ctx.mstep_soup(alpha)
        fio.assert_bitwise(again, profile, 'the step again: the profile')
        fio.assert_bitwise(counts_again, counts, 'the step again: the counts')


# ---- B4. the fused loop is the step-wise one ---------------------------------------------------------------------
def test_fused_equals_stepwise():
    from demuxalot_amd.device import DeviceContext
    pool_of = pool_of_f1()
    penalty = pair_penalty(POOLS_F1, 0.35)
    alpha = fractions(1000, shift=3)
    problem = pooled.fixture_learning_problem(F1)
    soup = ambient_restatement.derived_ambient(problem['v'], problem['v2snp'], 0.01)
    history = soup_learning.learn(problem, POOLS_F1, pool_of, alpha, soup, 4, 0.01, 0.35)
    with DeviceContext(0) as fused, DeviceContext(0) as stepwise:
        for ctx in (fused, stepwise):
            install(ctx, F1)
        previous_counts = np.zeros(len(soup), np.float32)  # (one iteration: no soup step ran)
        for it, (step, addition) in enumerate(staged(stepwise, 4, 0.01, POOLS_F1, pool_of, True, penalty, alpha, None)):
            # every iteration's profile, addition and rows: the step-wise sequence against the restatement, the fused loop of it + 1
            # iterations against the step-wise sequence
            assert_iteration(stepwise, step, history[it], f'staged iteration {it}', addition)
            assert_soup_step(step, history[it], f'staged iteration {it}')
            got = fused.em_ambient_soup(it + 1, 0.01, POOLS_F1, pool_of, True, penalty, alpha)
            for key in ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass', 'ambient'):
                assert got[key].tobytes() == step[key].tobytes(), (it, key)
            fio.assert_bitwise(got['addition'], addition, f'fused, {it + 1} iterations: addition')
            fio.assert_bitwise(got['counts'], previous_counts, f'fused, {it + 1} iterations: counts_out')
            fio.assert_bitwise(fused.get_probs(), stepwise.get_probs(), f'fused, {it + 1} iterations: get_probs()')
            previous_counts = step['counts']
        assert not np.array_equal(history[1]['ambient'], history[0]['ambient']) and not np.array_equal(history[3]['ambient'], history[2]['ambient'])
        fio.assert_bitwise(fused.get_probs(), stepwise.get_probs(), 'get_probs()')
        fio.assert_bitwise(fused.get_learnt_betas(), stepwise.get_learnt_betas(), 'learnt betas')
        fio.assert_bitwise(fused.get_learnt_betas(), soup_learning.learnt_betas(problem, history), 'learnt betas against the restatement')


# ---- B5. every fraction 0: dmx_em_pools with exact additions -----------------------------------------------------
@pytest.mark.parametrize('name', SMALL + [F1])
def test_zero_fractions_are_the_pooled_loop(name):
    ctx = learner(name)
    B, G = ctx.B, ctx.G
    dp = 0.35 if name in (F1, 'f3_small_1.npz') else 0.0
    pools, pool_of = helpers.pools_of(name, B, G)
    penalty = pair_penalty(pools, dp)
    n = 3
    ctx.set_exact_additions(True)
    try:
        want = ctx.em_pools(n, 0.01, pools, pool_of, dp != 0, penalty)
        want_dense, want_betas = ctx.get_probs(), ctx.get_learnt_betas()
        got = ctx.em_ambient_soup(n, 0.01, pools, pool_of, dp != 0, penalty, np.zeros(B, np.float32))
    finally:
        ctx.apply_environment()
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), f'{name}: {key} against dmx_em_pools'
    fio.assert_bitwise(ctx.get_probs(), want_dense, f'{name}: get_probs() against dmx_em_pools')
    fio.assert_bitwise(ctx.get_learnt_betas(), want_betas, f'{name}: learnt betas against dmx_em_pools')
    assert not got['counts'].any() and not np.signbit(got['counts']).any(), 'every count is +0'
    v2snp = pooled.fixture_learning_problem(name)['v2snp']
    fio.assert_bitwise(got['ambient'], soup_learning.profile_from_totals(got['counts'], v2snp, 1., 0.01), 'the pseudo-counts\' uniform share')


# ---- B6. refusals -------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from demuxalot_amd._lib import DemuxHipError
    from demuxalot_amd.device import DeviceContext
    name = 'f3_small_1.npz'
    problem = pooled.fixture_learning_problem(name)
    B, (V, G) = problem['B'], problem['betas'].shape
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    alpha = fractions(B)
    soup = np.full(V, 0.5, np.float32)
    changed = helpers.at
    with DeviceContext(0) as ctx:
        install(ctx, name)
        good = ctx.em_ambient_soup(2, 0.01, pools, pool_of, False, [0.0], alpha, ambient=soup)
        good_step = ctx.mstep_soup(alpha, ambient=soup)
        dense, betas, addition = ctx.get_probs(), ctx.get_learnt_betas(), ctx.get_addition()

        def launches():
            timings = ctx.timings()
            return tuple(timings[phase]['launches'] for phase in ('pstep', 'estep', 'mstep', 'mcombine'))

        before = launches()
        em = lambda **kw: ctx.em_ambient_soup(**{**dict(n_iterations=2, p_genotype_clip=0.01, pools=pools, pool_of_barcode=pool_of,  # noqa: E731
                                                        with_doublets=False, pair_penalty=[0.0], alpha=alpha, ambient=soup), **kw})
        step = lambda a=alpha, **kw: ctx.mstep_soup(a, **{**dict(ambient=soup), **kw})  # noqa: E731
        cases = [
            (lambda: em(n_iterations=0), r'dmx_em_ambient_soup.*n_iterations.*status -1'),
            (lambda: em(n_iterations=0, pseudo_count=0.0), r'n_iterations.*status -1'),
            (lambda: em(contribution_power=0.0), r'power.*status -1'),
            (lambda: em(contribution_power=float('nan'), pseudo_count=0.0), r'power.*status -1'),
            (lambda: em(pseudo_count=0.0), r'dmx_em_ambient_soup.*pseudo-count.*status -1'),
            (lambda: em(pseudo_count=-1.0), r'pseudo-count.*status -1'),
            (lambda: em(pseudo_count=float('nan')), r'pseudo-count.*status -1'),
            (lambda: em(pseudo_count=float('inf')), r'pseudo-count.*status -1'),
            (lambda: em(pseudo_count=0.0, alpha=changed(alpha, 3, 1.5)), r'pseudo-count.*status -1'),
            (lambda: em(alpha=changed(alpha, 3, 1.5)), r'alpha of a barcode.*status -1'),
            (lambda: em(alpha=changed(alpha, B - 1, np.nan)), r'alpha of a barcode.*status -1'),
            (lambda: em(ambient=changed(soup, 2, -0.25)), r'ambient value.*status -1'),
            (lambda: em(ambient=changed(soup, V - 1, np.inf)), r'ambient value.*status -1'),
            (lambda: em(pools=[[0, 0]]), r'status -1'),
            (lambda: step(pseudo_count=0.0), r'dmx_mstep_soup.*pseudo-count.*status -1'),
            (lambda: step(pseudo_count=float('nan')), r'dmx_mstep_soup.*pseudo-count.*status -1'),
            (lambda: step(pseudo_count=float('inf')), r'dmx_mstep_soup.*pseudo-count.*status -1'),
            (lambda: step(changed(alpha, 0, 2.0), pseudo_count=-1.0), r'dmx_mstep_soup.*pseudo-count.*status -1'),
            (lambda: step(changed(alpha, 0, 2.0)), r'dmx_mstep_soup.*alpha of a barcode.*status -1'),
            (lambda: step(ambient=changed(soup, 0, np.nan)), r'dmx_mstep_soup.*ambient value.*status -1'),
        ]
        for call, message in cases:
            with pytest.raises(DemuxHipError, match=message):
                call()
            assert launches() == before, (message, 'a refused call launches nothing')
            fio.assert_bitwise(ctx.get_probs(), dense, f'{message}: the resident posteriors after the refusal')
            fio.assert_bitwise(ctx.get_learnt_betas(), betas, f'{message}: the learnt betas after the refusal')
            fio.assert_bitwise(ctx.get_addition(), addition, f'{message}: the addition after the refusal')
        for got, want in zip(step(), good_step):
            fio.assert_bitwise(got, want, 'a valid step after the refused ones')
        again = em()
        for key in good:
            assert again[key].tobytes() == good[key].tobytes(), f'a valid call after the refused ones: {key}'
    with DeviceContext(0) as ctx:  # call order: nothing, a problem, a table, posteriors
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_soup.*problem.*status -1'):
            ctx.B, ctx.V, ctx.G = B, V, G
            ctx.mstep_soup(alpha, ambient=soup)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_soup.*genotype probabilities.*status -1'):
            ctx.mstep_soup(alpha, ambient=soup, pseudo_count=0.0)
        with pytest.raises(DemuxHipError, match=r'dmx_em_ambient_soup.*status -1'):
            ctx.em_ambient_soup(2, 0.01, pools, pool_of, False, [0.0], alpha)
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        with pytest.raises(DemuxHipError, match=r'dmx_mstep_soup.*E-step.*status -1'):
            ctx.mstep_soup(alpha, ambient=soup)
        assert all(ctx.timings()[phase]['launches'] == 0 for phase in ('estep', 'mstep', 'mcombine'))
    with DeviceContext(0) as ctx:
        ctx.comm_init_emulated(0, 1)
        ctx.set_problem(B, V, G, problem['v'], problem['cb'], problem['e'], problem['v2snp'])
        ctx.set_betas(problem['betas'])
        ctx.probs_from_betas(0.01, fetch=False)
        ctx.estep(np.zeros(G, np.float32), False)
        for call in (lambda: ctx.em_ambient_soup(2, 0.01, pools, pool_of, False, [0.0], alpha),
                     lambda: ctx.mstep_soup(alpha, ambient=soup),
                     lambda: ctx.mstep_soup(alpha, ambient=soup, pseudo_count=0.0)):
            with pytest.raises(DemuxHipError, match=r'communicator.*status -5'):
                call()


# ---- B7. end to end (exact_mode: the default context's passes in the exact arithmetic) -----------------------------------------
def test_learn_the_profile_end_to_end(exact_mode):
    from demuxalot_amd import Demultiplexer
    sim = soup_learning.simulate(0)
    B, G = sim['B'], sim['prob'].shape[1]
    derived = ambient_restatement.derived_ambient(sim['v'], sim['v2snp'], 0.01)
    derived_error = soup_learning.profile_error(derived, sim)
    alpha = sim['truth'].astype(np.float32)
    # the genotypes fixed: betas that are the simulation's table times 1000, so the P-step's table is the true one to float32 accuracy
    calls, genotypes, handler = helpers.user_inputs(sim, helpers.table_betas(sim), default_prior=0.0)
    table = restated.demux_oracle.probs_from_betas(sim['v2snp'], helpers.table_betas(sim), 0.01)
    assert np.abs(table - sim['prob']).max() < 1e-6
    calls_only = dict(v=sim['v'], cb=sim['cb'], e=sim['e'], v2snp=sim['v2snp'], B=B)
    history = soup_learning.learn_profile(calls_only, table, [list(range(G))], np.zeros(B, np.int32), alpha, derived, 3, 0.01, 0.)
    barcodes = handler.ordered_barcodes
    fractions_of = {bc: float(a) for bc, a in zip(barcodes, alpha)}
    profile = Demultiplexer.learn_ambient_profile(calls, genotypes, handler, fractions_of)
    assert profile.dtype == np.float32 and profile.shape == (len(sim['v2snp']),)
    fio.assert_bitwise(profile, history[-1]['next_ambient'], 'learn_ambient_profile: the restatement\'s bits')
    soup_learning.recovery_condition(derived_error, soup_learning.profile_error(profile, sim), 'learn_ambient_profile: ')
    # the genotypes learnt along: prior betas that know half of the truth, as the ambient learning's simulated problem has them
    betas = ((np.float32(0.5) * sim['prob'] + np.float32(0.25)) * np.float32(2)).astype(np.float32)
    problem = dict(v=sim['v'], cb=sim['cb'], e=sim['e'], v2snp=sim['v2snp'], betas=betas, raw_betas=betas, B=B)
    calls, genotypes, handler = helpers.user_inputs(sim, betas, default_prior=0.0)
    n = 4  # three updates of the profile
    both = soup_learning.learn(problem, [list(range(G))], np.zeros(B, np.int32), alpha, derived, n, 0.01, 0.)
    learnt, probs_df, learnt_profile = Demultiplexer.learn_genotypes_and_ambient(calls, genotypes, handler, fractions_of, n_iterations=n)
    assert list(probs_df.index) == barcodes and list(probs_df.columns) == list(genotypes.genotype_names) and probs_df.values.dtype == np.float32
    fio.assert_bitwise(probs_df.values, both[-1]['probs'].reshape(B, G), 'learn_genotypes_and_ambient: the last posteriors')
    fio.assert_bitwise(learnt.variant_betas, soup_learning.learnt_betas(problem, both), 'learn_genotypes_and_ambient: learnt betas')
    fio.assert_bitwise(learnt_profile, both[-1]['ambient'], 'learn_genotypes_and_ambient: the profile of the last E-step')
    soup_learning.recovery_condition(derived_error, soup_learning.profile_error(learnt_profile, sim), 'learn_genotypes_and_ambient: ')
    assert np.array_equal(probs_df.values.argmax(axis=1), sim['donor1']), 'an arg-max is not the true donor'
    # the generator: every iteration, the profile its E-step read; it may be closed early
    generator = Demultiplexer.staged_genotype_learning_and_ambient(calls, genotypes, handler, fractions_of, n_iterations=n)
    for it, (step, debug) in enumerate(generator):
        fio.assert_bitwise(step.values, both[it]['probs'].reshape(B, G), f'generator, iteration {it}: posteriors')
        fio.assert_bitwise(debug['genotype_addition'], both[it]['addition'], f'generator, iteration {it}: addition')
        fio.assert_bitwise(debug['ambient'], both[it]['ambient'], f'generator, iteration {it}: the profile')
        if it == 1:
            generator.close()
            break
