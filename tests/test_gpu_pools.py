"""The pooled E-step on the GPU (include/demux_hip_debug.h: dmx_estep_pools; csrc/estep_pools.hip; Demultiplexer.predict_posteriors_in_pools).

The kernel has no tolerance arithmetic: everything is compared bit for bit.  The checker is tests/pools_restatement.py - the oracle on
prob[:, d_p] per donor list, proven against the reference's own outputs in tests/test_pools_cpu.py - and, for one all-donor pool, the
reference's captured predict_posteriors itself.  The shapes are the smallest at which the kernel can go wrong: every number of option
slots per lane (1, 2, 4, 8, 16), both sides of the 64-lane boundary and of numpy's 128-element pairwise block, more pools than
barcodes per wavefront, overlapping pools, barcodes without calls and barcodes in no pool."""
import functools

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests import pools_restatement as restated

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
resident = functools.lru_cache(maxsize=None)(helpers.new_resident)  # (ctx, v, cb, e, prob, B, v2snp), the contexts this module's own


@functools.lru_cache(maxsize=None)
def restatement(name, doublet_prior, clip=0.01, extra_barcodes=0):
    _ctx, v, cb, e, prob, B, _v2snp = resident(name, clip, extra_barcodes)
    return restated.Restatement(v, cb, e, prob, B, doublet_prior)


def run(ctx, r, pools, pool_of):
    return ctx.estep_pools(pools, pool_of, r.doublet_prior != 0, r.pair_penalty(pools))


def prefix_pools(sizes):
    return [list(range(g)) for g in sizes]


# ---- 1. one all-donor pool is the reference's predict_posteriors ----------------------------------------------
@pytest.mark.parametrize('name', ['f3_small_0.npz', 'f3_small_1.npz', 'f3_small_2.npz', 'f3_small_3.npz', 'f2_synthetic_g4.npz',
                                  'f1_synthetic_default.npz'])
def test_all_donor_pool_is_the_reference(name):
    fx = fio.load(name)
    G = len(fx['genotype_names'])
    seen = set()
    for i in range(int(fx['n_predict'])):
        dp, clip = float(fx[f'predict{i}_dp']), float(fx[f'predict{i}_clip'])
        ctx, _v, _cb, _e, _prob, B, _v2snp = resident(name, clip)
        pen = restated.demux_oracle.doublet_penalties(G, dp)[-1] if dp != 0 else 0.0
        got = ctx.estep_pools([list(range(G))], np.zeros(B, np.int32), dp != 0, [pen])
        K = fx[f'predict{i}_logits'].shape[1]
        assert np.array_equal(got['row_ptr'], np.arange(B + 1) * K)
        fio.assert_bitwise(got['logits'].reshape(B, K), fx[f'predict{i}_logits'], f'{name} predict {i}: logits')
        fio.assert_bitwise(got['probs'].reshape(B, K), fx[f'predict{i}_probs'], f'{name} predict {i}: probs')
        assert np.array_equal(got['best_option'], fx[f'predict{i}_probs'].argmax(axis=1))
        seen.add(dp != 0)
    assert seen == {False, True}, 'with and without doublets'


# ---- 2. slot and pairwise-sum boundaries ------------------------------------------------------------------------
F1 = helpers.F1
SIZES = (1, 2, 7, 8, 10, 11, 15, 16, 20)  # K = 1, 3, 28, 36, 55 | 66, 120 | 136, 210: slots 1, 2, 4; the 64 and the 128 boundary


def test_slot_and_pairwise_boundaries_round_robin():
    ctx, *_rest, B, _v2snp = resident(F1)
    r = restatement(F1, 0.35)
    pools = prefix_pools(SIZES)
    pool_of = (np.arange(B) % len(pools)).astype(np.int32)
    restated.assert_same(run(ctx, r, pools, pool_of), r(pools, pool_of), 'round robin')
    # without doublets the same pools have 1 .. 20 options
    r0 = restatement(F1, 0.0)
    got = run(ctx, r0, pools, pool_of)
    restated.assert_same(got, r0(pools, pool_of), 'round robin, singlets only')
    assert not got['doublet_mass'].any()


def test_every_barcode_in_a_pool_of_its_own():
    ctx, *_rest, B, _v2snp = resident(F1)
    r = restatement(F1, 0.35)
    pools = [list(range(SIZES[b % len(SIZES)])) for b in range(B)]
    pool_of = np.arange(B, dtype=np.int32)[::-1].copy()  # (and not in pool order)
    restated.assert_same(run(ctx, r, pools, pool_of), r(pools, pool_of), 'B pools')


def test_overlapping_pools():
    ctx, *_rest, B, _v2snp = resident(F1)
    r = restatement(F1, 0.35)
    pools = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11], [0, 19], [3, 7, 11, 15, 19], list(range(5, 20)), [19]]
    pool_of = ((np.arange(B) * 7) % len(pools)).astype(np.int32)
    restated.assert_same(run(ctx, r, pools, pool_of), r(pools, pool_of), 'overlapping pools')


# ---- 3. wide rows ---------------------------------------------------------------------------------------------------
WIDE = helpers.WIDE  # G = 70, B = 24


def test_wide_singlet_pools():
    ctx, *_rest, B, _v2snp = resident(WIDE)
    r = restatement(WIDE, 0.0)
    pools = [list(range(64)), list(range(3, 68)), list(range(70))]  # one slot exactly, two, two
    pool_of = (np.arange(B) % 3).astype(np.int32)
    restated.assert_same(run(ctx, r, pools, pool_of), r(pools, pool_of), 'singlet pools of 64, 65, 70')


def test_widest_doublet_pool_and_the_refusal_behind_it():
    ctx, *_rest, B, _v2snp = resident(WIDE)
    r = restatement(WIDE, 0.35)
    pools = [list(range(13, 57)), list(range(30))]  # K = 990: sixteen slots; K = 465: eight
    pool_of = (np.arange(B) % 2).astype(np.int32)
    want = r(pools, pool_of)
    assert want['row_ptr'][1] == 990
    restated.assert_same(run(ctx, r, pools, pool_of), want, 'doublet pools of 44 and 30')
    before = ctx.timings()['estep']['launches']
    from demuxalot_amd._lib import DemuxHipError
    with pytest.raises(DemuxHipError, match=r'1035 options.*status -5'):
        run(ctx, r, [list(range(45))], np.zeros(B, np.int32))
    assert ctx.timings()['estep']['launches'] == before, 'a refused call launches nothing'
    restated.assert_same(run(ctx, r, pools, pool_of), want, 'after the refusal')


# ---- 4. rows that need care ------------------------------------------------------------------------------------------
def test_barcodes_without_calls_and_barcodes_in_no_pool():
    name, extra = 'f3_small_2.npz', 3
    ctx, *_rest, B, _v2snp = resident(name, 0.01, extra)
    r = restatement(name, 0.35, 0.01, extra)
    pools = [[0, 1, 2, 3, 4], [1, 3], [2]]
    pool_of = (np.arange(B) % 4 - 1).astype(np.int32)
    pool_of[B - extra:] = [0, 1, -1]
    got, want = run(ctx, r, pools, pool_of), r(pools, pool_of)
    restated.assert_same(got, want, 'with empty barcodes')
    b = B - extra  # no calls, pool 0: the row is the penalties, the posterior their softmax
    pen = restated.demux_oracle.doublet_penalties(5, 0.35)
    fio.assert_bitwise(got['logits'][got['row_ptr'][b]:got['row_ptr'][b + 1]], pen, 'logits of a barcode without calls')
    fio.assert_bitwise(got['probs'][got['row_ptr'][b]:got['row_ptr'][b + 1]], restated.demux_oracle.softmax_rows(pen[None, :])[0], 'its posterior')
    none = pool_of < 0
    assert none.sum() >= 2 and (np.diff(got['row_ptr'])[none] == 0).all(), 'nothing inside row_ptr for a barcode in no pool'
    assert (got['best_option'][none] == -1).all() and np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all()
    # nobody in a pool: an empty result
    empty = run(ctx, r, pools, np.full(B, -1, np.int32))
    assert empty['logits'].shape == (0,) and empty['probs'].shape == (0,) and not empty['row_ptr'].any()
    assert (empty['best_option'] == -1).all() and np.isnan(empty['best_prob']).all() and np.isnan(empty['doublet_mass']).all()
    restated.assert_same(run(ctx, r, pools, pool_of), want, 'after the empty call')


# ---- 5. read-outs: exact ties ------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_option():
    """Two identical table columns: the two singlets tie exactly, and so do the pairs either forms with a third donor."""
    from demuxalot_amd.device import DeviceContext
    fx = fio.load('f3_small_2.npz')
    v, cb, e, prob, B = restated.fixture_problem('f3_small_2.npz')
    prob = prob.copy()
    prob[:, 3] = prob[:, 1]
    with DeviceContext(0) as ctx:
        ctx.set_problem(B, len(fx['pack_v2snp']), prob.shape[1], v, cb, e, fx['pack_v2snp'])
        ctx.set_probs(prob)
        for dp in (0.35, 0.0):
            r = restated.Restatement(v, cb, e, prob, B, dp)
            pools = [[1, 3], [0, 1, 3]]
            pool_of = (np.arange(B) % 2).astype(np.int32)
            got, want = run(ctx, r, pools, pool_of), r(pools, pool_of)
            restated.assert_same(got, want, f'tied columns, doublet prior {dp}')
            for b in np.flatnonzero(pool_of == 0):
                row = got['probs'][got['row_ptr'][b]:got['row_ptr'][b + 1]]
                assert row[0] == row[1], 'the two singlets tie'
                if row[0] >= row[-1]:
                    assert got['best_option'][b] == 0, 'ties go to the lower index'
            assert (got['best_option'][pool_of == 0] != 1).all()


# ---- 6. isolation ----------------------------------------------------------------------------------------------------
def test_leaves_the_resident_results_alone_and_ignores_the_estep_mode():
    ctx, *_rest, B, _v2snp = resident(F1)
    r = restatement(F1, 0.35)
    pools = prefix_pools((3, 11, 16))
    pool_of = (np.arange(B) % 4 - 1).astype(np.int32)
    ctx.set_estep_mode('exact')
    try:
        penalties = restated.demux_oracle.doublet_penalties(ctx.G, 0.35)
        _logits, probs = ctx.estep(penalties, True)
        first = run(ctx, r, pools, pool_of)
        fio.assert_bitwise(ctx.get_probs(), probs, 'dmx_get_probs after dmx_estep_pools')
        second = run(ctx, r, pools, pool_of)
        for key in first:
            assert first[key].tobytes() == second[key].tobytes(), f'{key}: two runs differ'
        ctx.set_estep_mode('guarded')
        guarded = run(ctx, r, pools, pool_of)
        for key in first:
            assert first[key].tobytes() == guarded[key].tobytes(), f'{key}: guarded mode differs'
        restated.assert_same(first, r(pools, pool_of), 'three pools and barcodes in none')
        # the read-outs alone: nothing of size row_ptr[B] is downloaded
        lean = ctx.estep_pools(pools, pool_of, True, r.pair_penalty(pools), fetch_logits=False, fetch_probs=False)
        assert lean['logits'] is None and lean['probs'] is None
        for key in ('best_option', 'best_prob', 'doublet_mass'):
            assert lean[key].tobytes() == first[key].tobytes(), key
    finally:
        ctx.apply_environment()


# ---- 7. invalid inputs -------------------------------------------------------------------------------------------------
def raw_call(ctx, with_doublets, pool_start, donors, penalty, pool_of, row_ptr, n_pools=None, B=None):
    """dmx_estep_pools with the arrays as given: (status, message)."""
    from demuxalot_amd import _lib
    pool_start, donors = np.asarray(pool_start, np.int64), np.asarray(donors, np.int32)
    penalty, pool_of, row_ptr = np.asarray(penalty, np.float32), np.asarray(pool_of, np.int32), np.asarray(row_ptr, np.int64)
    n = int(row_ptr[-1]) if len(row_ptr) and row_ptr[-1] > 0 else 0
    logits, probs = np.zeros(n, np.float32), np.zeros(n, np.float32)
    B = ctx.B if B is None else B
    best, best_p, mass = np.zeros(B, np.int32), np.zeros(B, np.float32), np.zeros(B, np.float64)
    status = ctx._lib.dmx_estep_pools(ctx._h, with_doublets, len(pool_start) - 1 if n_pools is None else n_pools, _lib.ptr(pool_start),
                                      _lib.ptr(donors), _lib.ptr(penalty), _lib.ptr(pool_of), _lib.ptr(row_ptr), _lib.ptr(logits),
                                      _lib.ptr(probs), _lib.ptr(best), _lib.ptr(best_p), _lib.ptr(mass))
    return status, _lib.load().dmx_last_error().decode()


def test_invalid_inputs_are_refused_and_leave_the_context_usable():
    name = 'f3_small_2.npz'  # G = 5
    ctx, *_rest, B, _v2snp = resident(name)
    r = restatement(name, 0.35)
    pools = [[0, 1], [1, 2, 4]]
    pool_of = (np.arange(B) % 2).astype(np.int32)
    want = r(pools, pool_of)
    good = dict(with_doublets=1, pool_start=[0, 2, 5], donors=[0, 1, 1, 2, 4], penalty=r.pair_penalty(pools), pool_of=pool_of,
                row_ptr=want['row_ptr'])
    assert raw_call(ctx, **good)[0] == 0
    short_rows = want['row_ptr'].copy()
    short_rows[-1] -= 1
    cases = helpers.pool_refusal_cases(good, pool_of) + [
        (dict(pool_start=[0, 3, 2], donors=[0, 1, 2, 4, 4]), DMX_ERR_INVALID, 'decreases'),
        (dict(donors=[0, 0, 1, 2, 4]), DMX_ERR_INVALID, 'ascending'),
        (dict(donors=[-1, 1, 1, 2, 4]), DMX_ERR_INVALID, 'outside'),
        (dict(pool_of=helpers.at(pool_of, 1, -2)), DMX_ERR_INVALID, 'pool_of_barcode'),
        (dict(row_ptr=short_rows), DMX_ERR_INVALID, 'row_ptr'),
        (dict(with_doublets=0), DMX_ERR_INVALID, 'row_ptr'),  # (the rows were laid out for the pairs)
    ]
    launches = ctx.timings()['estep']['launches']
    for change, status, message in cases:
        got_status, text = raw_call(ctx, **{**good, **change})
        assert got_status == status, (change, got_status, text)
        assert message in text, (change, text)
        assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    restated.assert_same(run(ctx, r, pools, pool_of), want, 'a valid call after the refused ones')


def test_needs_a_problem_and_a_table():
    from demuxalot_amd.device import DeviceContext
    fx = fio.load('f3_small_0.npz')
    v, cb, e, prob, B = restated.fixture_problem('f3_small_0.npz')
    with DeviceContext(0) as ctx:
        args = dict(with_doublets=1, pool_start=[0, 2], donors=[0, 1], penalty=[0.0], pool_of=np.zeros(B, np.int32), row_ptr=np.arange(B + 1) * 3, B=B)
        status, text = raw_call(ctx, **args)
        assert status == DMX_ERR_INVALID and 'before dmx_estep_pools' in text
        ctx.set_problem(B, len(fx['pack_v2snp']), 2, v, cb, e, fx['pack_v2snp'])
        status, text = raw_call(ctx, **args)
        assert status == DMX_ERR_INVALID and 'before dmx_estep_pools' in text
        ctx.set_probs(prob)
        assert raw_call(ctx, **args)[0] == 0


# ---- 8. end to end ---------------------------------------------------------------------------------------------------
def test_predict_posteriors_in_pools_end_to_end():
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    name = 'f6_shipped_example.npz'
    fx = fio.load(name)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    B = len(barcodes)
    pool2donors = {'A': [donors[1], donors[0]], 'B': [donors[3], donors[1], donors[2]]}  # (any order)
    barcode2pool = {bc: (None if i % 5 == 4 else 'AB'[i % 2]) for i, bc in enumerate(barcodes)}
    pooled = Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, doublet_prior=0.35)
    assert isinstance(pooled, PooledPosteriors) and pooled.pools == ['A', 'B']
    v, cb, e, prob, n = restated.fixture_problem(name)
    assert n == B
    r = restated.Restatement(v, cb, e, prob, B, 0.35)
    pools = [[0, 1], [1, 2, 3]]
    pool_of = np.array([-1 if i % 5 == 4 else i % 2 for i in range(B)], np.int32)
    want = r(pools, pool_of)
    raw = dict(row_ptr=pooled.row_ptr, logits=pooled.logits, probs=pooled.probs, best_option=pooled.best_option, best_prob=pooled.best_prob,
               doublet_mass=pooled.doublet_mass)
    restated.assert_same(raw, want, 'end to end')
    for p, pool in enumerate('AB'):
        names = restated.demux_oracle.option_names([donors[g] for g in pools[p]], 0.35)
        rows = np.flatnonzero(pool_of == p)
        logits_df, probs_df = pooled.to_dataframes(pool)
        for frame, full in ((logits_df, r.pool_rows(pools[p])[0]), (probs_df, r.pool_rows(pools[p])[1])):
            assert list(frame.columns) == names and list(frame.index) == [barcodes[i] for i in rows] and frame.index.name == 'BARCODE'
            assert frame.values.dtype == np.float32
            fio.assert_bitwise(frame.values, full[rows], f'pool {pool}')
        assert pooled.barcodes_of(pool) == [barcodes[i] for i in rows]
    best = pooled.best()
    assert list(best.index) == barcodes and best['option'][barcodes[4]] is None and best['pool'][barcodes[4]] is None
    b = int(np.flatnonzero(pool_of == 1)[0])
    assert best['option'][barcodes[b]] == restated.demux_oracle.option_names([donors[g] for g in pools[1]], 0.35)[want['best_option'][b]]
    assigned = pooled.assignments(0.9)
    assert len(assigned) == int((want['best_prob'] > np.float32(0.9)).sum())
    fio.assert_bitwise(pooled.doublet_probability().values[pool_of >= 0], want['doublet_mass'][pool_of >= 0], 'doublet_probability()')
    # resident call sets are accepted in place of the host containers, as everywhere else
    from demuxalot_amd import ResidentCalls
    resident = {chromosome: ResidentCalls(c) for chromosome, c in calls.items()}
    try:
        again = Demultiplexer.predict_posteriors_in_pools(resident, genotypes, handler, barcode2pool, pool2donors, doublet_prior=0.35)
    finally:
        for r_calls in resident.values():
            r_calls.close()
    for key in raw:
        assert getattr(again, key).tobytes() == raw[key].tobytes(), f'resident call sets: {key}'
    # the all-donor pool through the same entry point is predict_posteriors itself
    one = Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, {bc: 'all' for bc in barcodes}, {'all': donors[::-1]},
                                                    doublet_prior=float(fx['predict0_dp']))
    logits_df, probs_df = one.to_dataframes('all')
    assert list(probs_df.columns) == [str(c) for c in fx['predict0_columns']]
    fio.assert_bitwise(logits_df.values, fx['predict0_logits'], 'all-donor pool: logits')
    fio.assert_bitwise(probs_df.values, fx['predict0_probs'], 'all-donor pool: probs')
