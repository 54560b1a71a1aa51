"""Learning within pools on the GPU (include/demux_hip_debug.h: dmx_estep_pools_resident, dmx_em_pools; csrc/estep_pools.hip, the DENSE form;
Demultiplexer.learn_genotypes_in_pools, staged_genotype_learning_in_pools).

In the exact mode the suite pins, everything is compared bit for bit with tests/pools_learning_restatement.py - the reference's loop with the
pooled E-step, proven against the reference's own captured EM runs in tests/test_pools_learning_cpu.py - and, for one all-donor pool, with
those captured runs themselves.  The default additions (fixed point, incremental) carry the bounds the M-step already has."""
import functools

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests import pools_learning_restatement as learning
from tests import pools_restatement as restated
from tests.pooled_helpers import assert_iteration, install, pair_penalty, pool_of_f1

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1 = helpers.F1  # G = 20, B = 1000
WIDE = helpers.WIDE  # G = 70, B = 24: two nz words per row, no `first` codes
learner = functools.lru_cache(maxsize=None)(helpers.new_learner)  # a fixture installed for learning, the contexts this module's own


def all_donor_penalty(G, dp):
    return [restated.demux_oracle.doublet_penalties(G, dp)[-1] if dp != 0 else 0.0]


def staged(ctx, n, clip, pools, pool_of, with_doublets, penalty):
    """The step-wise path of the pooled loop: the resident pooled E-step, dmx_mstep behind it."""
    return helpers.staged(ctx, n, clip, lambda: ctx.estep_pools(pools, pool_of, with_doublets, penalty, resident=True), lambda _out: ctx.mstep())


# ---- 1. one all-donor pool is the reference's learn_genotypes ---------------------------------------------------
@pytest.mark.parametrize('name', ['f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz', 'f2_synthetic_g4.npz', F1])
def test_all_donor_pool_is_the_reference(name):
    fx = fio.load(name)
    ctx = learner(name)
    B, G = ctx.B, ctx.G
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    seen = set()
    for i in range(int(fx['n_em'])):
        if f'em{i}_prior_logits' in fx:
            continue
        n, dp, clip = int(fx[f'em{i}_n_iterations']), float(fx[f'em{i}_dp']), float(fx[f'em{i}_clip'])
        K = fx[f'em{i}_it0_probs'].shape[1]
        penalty = all_donor_penalty(G, dp)

        def check(got, it, what):
            assert np.array_equal(got['row_ptr'], np.arange(B + 1) * K)
            fio.assert_bitwise(got['logits'].reshape(B, K), fx[f'em{i}_it{it}_logits'], f'{what}: logits')
            fio.assert_bitwise(got['probs'].reshape(B, K), fx[f'em{i}_it{it}_probs'], f'{what}: probs')
            assert np.array_equal(got['best_option'], fx[f'em{i}_it{it}_probs'].argmax(axis=1))
            fio.assert_bitwise(ctx.get_probs(), np.ascontiguousarray(fx[f'em{i}_it{it}_probs'][:, :G]), f'{what}: get_probs()')

        got = ctx.em_pools(n, clip, pools, pool_of, dp != 0, penalty)
        check(got, n - 1, f'{name} run {i}, em_pools({n})')
        fio.assert_bitwise(got['addition'], fx[f'em{i}_it{n - 1}_addition'], f'{name} run {i}: addition')
        fio.assert_bitwise(ctx.get_learnt_betas(), fx[f'em{i}_learnt_betas'], f'{name} run {i}: learnt betas')
        for it, (step, addition) in enumerate(staged(ctx, n, clip, pools, pool_of, dp != 0, penalty)):
            check(step, it, f'{name} run {i}, staged iteration {it}')
            fio.assert_bitwise(addition, fx[f'em{i}_it{it}_addition'], f'{name} run {i}, staged iteration {it}: addition')
        fio.assert_bitwise(ctx.get_learnt_betas(), fx[f'em{i}_learnt_betas'], f'{name} run {i}: learnt betas after the staged path')
        seen.add(dp != 0)
    assert seen == {False, True}, 'with and without doublets'


# ---- 2. overlapping pools, barcodes and nobody's donors ---------------------------------------------------------
POOLS = helpers.POOLS_F1
ITERATIONS = 4


@functools.lru_cache(maxsize=None)
def restated_f1(dp):
    """The restatement's history of the overlapping pools on f1, computed once per doublet prior and shared."""
    problem = learning.fixture_learning_problem(F1)
    history = learning.learn(problem, POOLS, pool_of_f1(problem['B']), ITERATIONS, 0.01, dp)
    for rec in history:
        for value in rec.values():
            value.flags.writeable = False
    return problem, history


@pytest.mark.parametrize('dp', [0.35, 0.0])
def test_overlapping_pools(dp):
    problem, history = restated_f1(dp)
    pool_of = pool_of_f1()
    assert (pool_of < 0).sum() == 143
    # what makes the problem a test: finite rows, far from the full table's answer, still moving
    assert all(np.isfinite(rec['logits']).all() and np.isfinite(rec['probs']).all() for rec in history)
    if dp == 0:
        assert np.abs(history[-1]['addition'] - fio.load(F1)[f'em0_it{ITERATIONS - 1}_addition']).max() > 100
    assert np.abs(history[-1]['dense'] - history[-2]['dense']).max() >= 0.4
    ctx = learner(F1)
    penalty = pair_penalty(POOLS, dp)
    got = ctx.em_pools(ITERATIONS, 0.01, POOLS, pool_of, dp != 0, penalty)
    assert_iteration(ctx, got, history[-1], f'dp {dp}: em_pools({ITERATIONS})', got['addition'])
    fio.assert_bitwise(ctx.get_learnt_betas(), learning.learnt_betas(problem, history), f'dp {dp}: learnt betas')
    for it, (step, addition) in enumerate(staged(ctx, ITERATIONS, 0.01, POOLS, pool_of, dp != 0, penalty)):
        assert_iteration(ctx, step, history[it], f'dp {dp}: staged iteration {it}', addition)


# ---- 3. more than 64 donors: two bitmap words per row, no codes --------------------------------------------------
@pytest.mark.parametrize('dp, pools', [
    (0.0, [list(range(64)), list(range(3, 68)), list(range(70))]),  # one slot exactly, two, two
    (0.35, [list(range(13, 57)), list(range(30)), [69]]),  # K = 990: sixteen slots; K = 465: eight; one
])
def test_more_than_64_donors(dp, pools):
    problem = learning.fixture_learning_problem(WIDE)
    B, G = problem['B'], problem['betas'].shape[1]
    assert G == 70
    pool_of = (np.arange(B) % 3).astype(np.int32)
    history = learning.learn(problem, pools, pool_of, 3, 0.01, dp)
    ctx = learner(WIDE)
    got = ctx.em_pools(3, 0.01, pools, pool_of, dp != 0, pair_penalty(pools, dp))
    assert_iteration(ctx, got, history[-1], f'G = 70, dp {dp}', got['addition'])
    fio.assert_bitwise(ctx.get_learnt_betas(), learning.learnt_betas(problem, history), f'G = 70, dp {dp}: learnt betas')
    if dp != 0:
        outside = sorted(set(range(G)) - set(sum(pools, [])))
        assert len(outside) == 12 and history[-1]['addition'].any(axis=0).sum() == 58
        nobody = got['addition'][:, outside]
        assert not nobody.any() and not np.signbit(nobody).any(), 'a donor in no pool: exactly +0'
    for it, (step, addition) in enumerate(staged(ctx, 3, 0.01, pools, pool_of, dp != 0, pair_penalty(pools, dp))):
        assert_iteration(ctx, step, history[it], f'G = 70, dp {dp}: staged iteration {it}', addition)


# ---- 4. the fused loop is the step-wise one ---------------------------------------------------------------------
@pytest.mark.parametrize('exact', [True, False])
def test_fused_equals_stepwise(exact):
    from demuxalot_amd.device import DeviceContext
    pool_of = pool_of_f1()
    penalty = pair_penalty(POOLS, 0.35)
    with DeviceContext(0) as fused, DeviceContext(0) as stepwise:
        for ctx in (fused, stepwise):
            install(ctx, F1)
            ctx.set_exact_additions(exact)
        got = fused.em_pools(3, 0.01, POOLS, pool_of, True, penalty)
        *_, (want, addition) = staged(stepwise, 3, 0.01, POOLS, pool_of, True, penalty)
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), f'exact additions {exact}: {key}'
        fio.assert_bitwise(got['addition'], addition, f'exact additions {exact}: addition')
        fio.assert_bitwise(fused.get_probs(), stepwise.get_probs(), f'exact additions {exact}: get_probs()')
        fio.assert_bitwise(fused.get_learnt_betas(), stepwise.get_learnt_betas(), f'exact additions {exact}: learnt betas')


# ---- 5. the default additions -------------------------------------------------------------------------------------
# The largest deviation of em_pools(4)'s posteriors from the restatement with the default additions, measured on the MI355X on this
# problem: 0.0 at both doublet priors - the additions differ by at most 7.1e-15 (dp 0.35) and 3.7e-16 (dp 0), in entries
# that round to the same genotype table.  The bound is 4 x the measured figure and never above 1e-5, the default mode's contract, so the
# test asks for equal posteriors here.  The fixed-point sums are integers: the figure does not depend on the order of the additions.
MEASURED_DEVIATION = {0.35: 0.0, 0.0: 0.0}


def compact_argmax_gap(rec, B):
    """Per barcode the gap between its two largest posteriors (inf for a row of fewer than two options)."""
    gap = np.full(B, np.inf)
    for b in range(B):
        row = np.sort(rec['probs'][rec['row_ptr'][b]:rec['row_ptr'][b + 1]])
        if len(row) >= 2:
            gap[b] = float(row[-1]) - float(row[-2])
    return gap


@pytest.mark.parametrize('dp', [0.35, 0.0])
def test_default_additions(dp):
    problem, history = restated_f1(dp)
    B = problem['B']
    pool_of = pool_of_f1()
    penalty = pair_penalty(POOLS, dp)
    ctx = learner(F1)
    ctx.set_exact_additions(False)
    try:
        # the posteriors of the first E-step go into the first M-step bit-identical: its addition differs by the fixed-point sum only
        first = ctx.em_pools(1, 0.01, POOLS, pool_of, dp != 0, penalty)
        restated.assert_same(first, history[0], f'dp {dp}: the first E-step')
        two = ctx.em_pools(2, 0.01, POOLS, pool_of, dp != 0, penalty)
        calls = np.bincount(problem['v'], minlength=len(problem['betas'])).max()
        assert np.allclose(two['addition'], history[1]['addition'], rtol=3e-7, atol=1e-12 * calls), f'dp {dp}: the first addition'
        got = ctx.em_pools(ITERATIONS, 0.01, POOLS, pool_of, dp != 0, penalty)
        want = history[-1]
        assert np.array_equal(got['row_ptr'], want['row_ptr'])
        sharp = compact_argmax_gap(want, B) > 1e-3
        assert (~sharp).sum() <= 0.01 * B, 'at most 1 % of the barcodes are too close to call'
        assert np.array_equal(got['best_option'][sharp], want['best_option'][sharp]), f'dp {dp}: arg-max'
        deviation = float(np.abs(got['probs'].astype(np.float64) - want['probs']).max())
        print(f'default additions, dp {dp}: largest posterior deviation of em_pools({ITERATIONS}) = {deviation!r}; '
              f'addition: {float(np.abs(got["addition"].astype(np.float64) - want["addition"]).max())!r}')
        assert deviation <= min(4 * MEASURED_DEVIATION[dp], 1e-5), f'dp {dp}: posteriors deviate by {deviation}'
    finally:
        ctx.apply_environment()


# ---- 6. the context survives ------------------------------------------------------------------------------------
def raw_em_pools(ctx, n, row_ptr, pools, pool_of, with_doublets, penalty, entry='dmx_em_pools'):
    """The entry with the row pointer as given: (status, message)."""
    from demuxalot_amd import _lib
    sizes = np.array([len(d) for d in pools], np.int64)
    pool_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    donors = np.concatenate([np.asarray(d, np.int32) for d in pools])
    penalty, pool_of, row_ptr = np.asarray(penalty, np.float32), np.asarray(pool_of, np.int32), np.asarray(row_ptr, np.int64)
    size = max(int(row_ptr[-1]), 1)
    logits, probs = np.zeros(size, np.float32), np.zeros(size, np.float32)
    best, best_p, mass = np.zeros(ctx.B, np.int32), np.zeros(ctx.B, np.float32), np.zeros(ctx.B, np.float64)
    pool_args = (int(with_doublets), len(pools), _lib.ptr(pool_start), _lib.ptr(donors), _lib.ptr(penalty), _lib.ptr(pool_of), _lib.ptr(row_ptr))
    results = (_lib.ptr(logits), _lib.ptr(probs), _lib.ptr(best), _lib.ptr(best_p), _lib.ptr(mass))
    if entry == 'dmx_em_pools':
        status = ctx._lib.dmx_em_pools(ctx._h, n, 0.01, 0.99, *pool_args, 2.0, *results, None)
    else:
        status = ctx._lib.dmx_estep_pools_resident(ctx._h, *pool_args, *results)
    return status, _lib.load().dmx_last_error().decode()


def test_the_context_survives():
    from demuxalot_amd._lib import DemuxHipError
    fx = fio.load(F1)
    problem, history = restated_f1(0.0)
    pool_of = pool_of_f1()
    ctx = learner(F1)
    G = ctx.G
    penalty = pair_penalty(POOLS, 0.0)
    n = int(fx['em0_n_iterations'])
    assert float(fx['em0_dp']) == 0

    def plain_em():
        _logits, probs, addition = ctx.em(n, float(fx['em0_clip']), np.zeros(G, np.float32), False)
        fio.assert_bitwise(probs, fx[f'em0_it{n - 1}_probs'], 'em: probs')
        fio.assert_bitwise(addition, fx[f'em0_it{n - 1}_addition'], 'em: addition')
        fio.assert_bitwise(ctx.get_learnt_betas(), fx['em0_learnt_betas'], 'em: learnt betas')
        return probs

    def pooled_em(what):
        got = ctx.em_pools(ITERATIONS, 0.01, POOLS, pool_of, False, penalty)
        assert_iteration(ctx, got, history[-1], what, got['addition'])

    pooled_em('first')
    probs = plain_em()
    # dmx_estep_pools itself still leaves the resident results alone
    restated_rows = ctx.estep_pools(POOLS, pool_of, False, penalty)
    fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() after dmx_estep_pools')
    assert np.array_equal(restated_rows['row_ptr'], history[-1]['row_ptr'])
    pooled_em('after em')
    dense = ctx.get_probs()
    # refusals launch nothing and leave a usable context with its results
    launches = ctx.timings()['estep']['launches']
    with pytest.raises(DemuxHipError, match=r'n_iterations.*status -1'):
        ctx.em_pools(0, 0.01, POOLS, pool_of, False, penalty)
    bad_rows = history[-1]['row_ptr'].copy()
    bad_rows[-1] += 1
    for entry in ('dmx_em_pools', 'dmx_estep_pools_resident'):
        status, text = raw_em_pools(ctx, 2, bad_rows, POOLS, pool_of, False, penalty, entry)
        assert status == DMX_ERR_INVALID and 'row_ptr' in text and entry in text, (entry, status, text)
    assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    fio.assert_bitwise(ctx.get_probs(), dense, 'the resident posteriors after the refusals')
    pooled_em('after the refusals')
    plain_em()
    wide = learner(WIDE)
    launches = wide.timings()['estep']['launches']
    for call in (lambda: wide.em_pools(2, 0.01, [list(range(45))], np.zeros(wide.B, np.int32), True, [0.0]),
                 lambda: wide.estep_pools([list(range(45))], np.zeros(wide.B, np.int32), True, [0.0], resident=True)):
        with pytest.raises(DemuxHipError, match=r'1035 options.*status -5'):
            call()
    assert wide.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    singles = [list(range(64)), list(range(3, 68)), list(range(70))]
    thirds = (np.arange(wide.B) % 3).astype(np.int32)
    want = learning.learn(learning.fixture_learning_problem(WIDE), singles, thirds, 2, 0.01, 0.0)[-1]
    got = wide.em_pools(2, 0.01, singles, thirds, False, [0.0, 0.0, 0.0])
    assert_iteration(wide, got, want, 'G = 70 after the refusals', got['addition'])


# ---- 7. end to end ----------------------------------------------------------------------------------------------
def pooled_raw(pooled):
    return dict(row_ptr=pooled.row_ptr, logits=pooled.logits, probs=pooled.probs, best_option=pooled.best_option, best_prob=pooled.best_prob,
                doublet_mass=pooled.doublet_mass)


def test_learn_genotypes_in_pools_end_to_end():
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    # one all-donor pool: learn_genotypes itself
    name = 'f3_small_2.npz'
    fx = fio.load(name)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    for i in range(int(fx['n_em'])):
        if f'em{i}_prior_logits' in fx:
            continue
        n, dp, clip = int(fx[f'em{i}_n_iterations']), float(fx[f'em{i}_dp']), float(fx[f'em{i}_clip'])
        learnt, pooled = Demultiplexer.learn_genotypes_in_pools(calls, genotypes, handler, {bc: 'all' for bc in barcodes}, {'all': donors[::-1]},
                                                                n_iterations=n, p_genotype_clip=clip, doublet_prior=dp)
        assert isinstance(pooled, PooledPosteriors) and pooled.pools == ['all']
        fio.assert_bitwise(learnt.variant_betas, fx[f'em{i}_learnt_betas'], f'{name} run {i}: learnt betas')
        _logits_df, probs_df = pooled.to_dataframes('all')
        assert list(probs_df.index) == barcodes and list(probs_df.columns) == restated.demux_oracle.option_names(donors, dp)
        fio.assert_bitwise(probs_df.values, fx[f'em{i}_it{n - 1}_probs'], f'{name} run {i}: the last posteriors')
    # the overlapping pools of test 2, from the containers
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    problem, history = restated_f1(0.35)
    pool_of = pool_of_f1()
    pool2donors = {f'pool{p}': [donors[g] for g in reversed(columns)] for p, columns in enumerate(POOLS)}  # (any order)
    barcode2pool = {bc: (None if pool_of[b] < 0 else f'pool{pool_of[b]}') for b, bc in enumerate(barcodes)}
    learnt, pooled = Demultiplexer.learn_genotypes_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, n_iterations=ITERATIONS,
                                                            doublet_prior=0.35)
    restated.assert_same(pooled_raw(pooled), history[-1], 'end to end')
    fio.assert_bitwise(learnt.variant_betas, learning.learnt_betas(problem, history), 'end to end: learnt betas')
    assert pooled.columns_of('pool2') == restated.demux_oracle.option_names([donors[0], donors[19]], 0.35)
    assert learnt.genotype_names == genotypes.genotype_names and learnt is not genotypes
    # the generator: every iteration, the same last one, and it may be closed early
    generator = Demultiplexer.staged_genotype_learning_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, n_iterations=ITERATIONS,
                                                                doublet_prior=0.35)
    for it, (step, debug) in enumerate(generator):
        restated.assert_same(pooled_raw(step), history[it], f'generator, iteration {it}')
        fio.assert_bitwise(debug['genotype_addition'], history[it]['addition'], f'generator, iteration {it}: addition')
        fio.assert_bitwise(debug['genotype_prior'], problem['betas'], 'generator: prior betas')
    assert it == ITERATIONS - 1
    for key, value in pooled_raw(step).items():
        assert value.tobytes() == getattr(pooled, key).tobytes(), f'generator, last iteration: {key}'
    early = Demultiplexer.staged_genotype_learning_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, n_iterations=ITERATIONS,
                                                            doublet_prior=0.35)
    first, _debug = next(early)
    early.close()
    restated.assert_same(pooled_raw(first), history[0], 'generator closed after its first iteration')
