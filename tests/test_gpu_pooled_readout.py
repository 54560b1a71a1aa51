"""Pooled results kept resident, and the read-outs over them, on the GPU (include/demux_hip_debug.h "Pooled results kept resident";
csrc/pooled_readout.hip; DevicePooledPosteriors).

Nothing here has a tolerance: the order of additions is the contract, so every comparison is on bits (a NaN equals a NaN).  The
checker is tests/pooled_readout_restatement.py, proven against the dense donor-level restatement in tests/test_pooled_readout_cpu.py.
  1. uploaded designs: every read-out at every row length at which the kernels change path;
  2. the slabs of the option sums;
  3. the four pooled passes with the keep switch on and off, on the small problem of tests/test_gpu_pools.py;
  4. the front door: on_device=True against the host route."""
import functools

import numpy as np
import pytest

from tests import fixture_io as fio
from tests import pooled_readout_restatement as restated
from tests import pools_restatement

pytestmark = pytest.mark.gpu

NAN32 = np.float32(np.nan)


def same_bits(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == 'f':
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f'{what}: NaNs elsewhere'
        got, want = np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(want.dtype)
    assert got.tobytes() == want.tobytes(), f'{what}: {int((got != want).sum())} entries differ'


def softmax_rows(rng, row_ptr):
    probs = np.zeros(int(row_ptr[-1]), dtype=np.float32)
    for b in range(len(row_ptr) - 1):
        n = int(row_ptr[b + 1] - row_ptr[b])
        if n:
            x = (rng.normal(size=n) * 3).astype(np.float32)
            e = np.exp(x - x.max())
            probs[row_ptr[b]:row_ptr[b + 1]] = e / e.sum()
    return probs


# ---- 1. uploaded designs ----------------------------------------------------------------------------------------------------
DOUBLET_POOLS = (1, 2, 10, 11, 15, 16, 22, 23, 44)  # K = 1, 3, 55, 66, 120, 136, 253, 276, 990
SINGLET_POOLS = (1, 63, 64, 65, 256, 257, 1024)


@functools.lru_cache(maxsize=None)
def design(with_doublets):
    """(pool sizes - the last pool has no barcodes -, pool_of, row_ptr, logits, probs): every pool has 1, 4 or 5 barcodes,
    interleaved; barcodes in no pool first, in the middle and last."""
    rng = np.random.default_rng(7 + with_doublets)
    sizes = list(DOUBLET_POOLS if with_doublets else SINGLET_POOLS) + [3]
    members = [p for p in range(len(sizes) - 1) for _ in range((1, 4, 5)[p % 3])]
    members = [members[i] for i in rng.permutation(len(members))]
    half = len(members) // 2
    pool_of = np.array([-1] + members[:half] + [-1, -1] + members[half:] + [-1], dtype=np.int32)
    row_ptr = restated.row_pointer(sizes, pool_of, with_doublets)
    probs = softmax_rows(rng, row_ptr)
    logits = rng.normal(size=len(probs)).astype(np.float32)

    def rows_of_width(at_least):
        return [b for b in range(len(pool_of)) if row_ptr[b + 1] - row_ptr[b] >= at_least]

    def row(b):
        return probs[row_ptr[b]:row_ptr[b + 1]]
    wide = rows_of_width(66)
    g = [sizes[pool_of[b]] for b in wide]
    row(wide[0])[[63, 64]] = np.float32(2.0)  # a tie across the first lane boundary: 63 wins
    row(wide[1])[:] = 0  # exact zeros, and a tie of the last two entries
    row(wide[1])[[-2, -1]] = np.float32(0.5)
    row(wide[2])[:] = NAN32  # nothing to find
    row(wide[3])[::3] = NAN32  # NaNs among numbers (the singlet 0 among them)
    row(wide[4])[:] = np.float32(1.0 / len(row(wide[4])))  # everything ties
    if with_doublets:
        row(wide[5])[:g[5]] = 0  # a tie inside the pair block above every singlet
        row(wide[5])[[g[5] + 5, g[5] + 40]] = np.float32(3.0)
    narrow = [b for b in range(len(pool_of)) if row_ptr[b + 1] - row_ptr[b] == 1]
    row(narrow[0])[:] = NAN32  # a row of one NaN
    return sizes, pool_of, row_ptr, logits, probs


@pytest.fixture(scope='module')
def ctx():
    from demuxalot_amd.device import DeviceContext
    with DeviceContext(0) as context:
        yield context


def upload(ctx, with_doublets, logits=True):
    sizes, pool_of, row_ptr, all_logits, probs = design(with_doublets)
    got = ctx.pooled_upload(max(sizes), [list(range(g)) for g in sizes], pool_of, with_doublets, probs, all_logits if logits else None)
    assert np.array_equal(got, row_ptr)
    return sizes, pool_of, row_ptr, all_logits, probs


@pytest.mark.parametrize('with_doublets', [True, False])
def test_uploaded_design_every_readout(ctx, with_doublets):
    sizes, pool_of, row_ptr, logits, probs = upload(ctx, with_doublets)
    B = len(pool_of)
    info = ctx.pooled_info()
    assert info == dict(present=1, B=B, n_pools=len(sizes), n_values=len(probs), with_doublets=int(with_doublets), has_logits=1,
                        has_alpha_index=0, has_alpha_mean=0)
    want = restated.readout(probs, row_ptr, pool_of, sizes, with_doublets)
    got = ctx.pooled_readout(marginals=True)
    for key in want:
        same_bits(got[key], want[key], key)
    # the masses and the maxima do not depend on what else is asked for
    plain, lean = ctx.pooled_readout(), ctx.pooled_readout(masses=False)
    for key in plain:
        if plain[key] is not None:
            same_bits(plain[key], want[key], f'{key} without marginals')
        if lean[key] is not None:
            same_bits(lean[key], want[key], f'{key} without masses')
    assert lean['singlet_mass'] is None and lean['doublet_mass'] is None
    none = pool_of < 0
    assert none[0] and none[-1] and none.sum() == 4
    assert (got['best_option'][none] == -1).all() and np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all()
    if not with_doublets:
        assert not got['doublet_mass'][~none].any() and (got['best_pair'] == -1).all()
    for k in (1, 2, 3, 4):
        want_options, want_probs = restated.top_options(probs, row_ptr, k)
        options, values = ctx.pooled_top_options(k)
        assert np.array_equal(options, want_options), f'top {k}'
        same_bits(values, want_probs, f'top {k} probabilities')
    assert (options[np.diff(row_ptr) == 1, 1:] == -1).all(), 'rows shorter than k'
    sums, counts = ctx.pooled_option_sums(int(restated.row_pointer(sizes, np.arange(len(sizes)), with_doublets)[-1]))
    want_sums, want_counts = restated.option_sums(probs, row_ptr, pool_of, sizes, with_doublets)
    same_bits(sums, want_sums, 'option sums')
    assert np.array_equal(counts, want_counts) and counts[-1] == 0 and not sums[-restated.n_options(3, with_doublets):].any()
    # the matrices
    for what, values in (('logits', logits), ('probs', probs)):
        same_bits(ctx.pooled_get(what, 0, B, len(values)), values, f'get {what}')
        for b0, b1 in ((0, 0), (0, 1), (3, 9), (B - 1, B), (B, B)):
            same_bits(ctx.pooled_get(what, b0, b1, row_ptr[b1] - row_ptr[b0]), values[row_ptr[b0]:row_ptr[b1]], f'get {what} {b0}:{b1}')
        for p, g in enumerate(sizes):
            frame = restated.pool_frame(values, row_ptr, pool_of, p)
            K = restated.n_options(g, with_doublets)
            same_bits(ctx.pooled_get_pool(what, p, len(frame), K), frame.reshape(len(frame), K), f'get_pool {what} {p}')


@pytest.mark.parametrize('with_doublets', [True, False])
def test_uploaded_design_allowed_mass(ctx, with_doublets):
    from demuxalot_amd._lib import DemuxHipError
    sizes, pool_of, row_ptr, _logits, probs = upload(ctx, with_doublets, logits=False)
    B = len(pool_of)
    assert ctx.pooled_info()['has_logits'] == 0
    with pytest.raises(DemuxHipError, match='dmx_pooled_get: .*does not hold'):
        ctx.pooled_get('logits', 0, B, len(probs))
    rng = np.random.default_rng(3)
    start, options = [0], []
    for b in range(B):
        K = int(row_ptr[b + 1] - row_ptr[b])
        if K and b % 4 != 3:  # (every fourth list is empty)
            listed = list(rng.integers(0, K, size=int(rng.integers(1, 7))))
            options.extend(listed + listed[:1])  # a duplicate
            if b % 4 == 0:
                options.extend([K - 1, 0])  # the row's ends
        start.append(len(options))
    start, options = np.asarray(start, np.int64), np.asarray(options, np.int32)
    mass, hit = ctx.pooled_allowed_mass(start, options)
    want_mass, want_hit = restated.allowed_mass(probs, row_ptr, pool_of, start, options)
    same_bits(mass, want_mass, 'allowed mass')
    assert np.array_equal(hit, want_hit) and hit.any() and not hit.all()
    assert np.isnan(mass[pool_of < 0]).all() and not hit[pool_of < 0].any()
    # every refusal, before anything is launched
    pooled_b = int(np.flatnonzero(pool_of >= 0)[0])
    K = int(row_ptr[pooled_b + 1] - row_ptr[pooled_b])

    def refused(bad_start, bad_options, words):
        with pytest.raises(DemuxHipError, match=f'dmx_pooled_allowed_mass: .*{words}.*status -1'):
            ctx.pooled_allowed_mass(bad_start, bad_options)
    shifted = start.copy()
    shifted[0] = 1
    refused(shifted, options, r'allowed_start\[0\]')
    one = np.zeros(B + 1, np.int64)
    one[pooled_b + 1:] = 1
    falling = one.copy()
    falling[-1] = 0
    refused(falling, np.zeros(1, np.int32), 'decreases')
    refused(one, np.array([K], np.int32), 'outside its barcode')
    refused(one, np.array([-1], np.int32), 'outside its barcode')
    nobody = np.zeros(B + 1, np.int64)
    nobody[1:] = 1  # barcode 0 is in no pool
    refused(nobody, np.zeros(1, np.int32), 'in no pool')
    again, _ = ctx.pooled_allowed_mass(start, options)
    same_bits(again, want_mass, 'after the refusals')


def test_an_empty_slot_refuses_every_entry():
    from demuxalot_amd._lib import DemuxHipError, check
    from demuxalot_amd.device import DeviceContext
    with DeviceContext(0) as fresh:
        assert fresh.pooled_info()['present'] == 0
        fresh.pooled_release()  # nothing to drop: no error
        calls = (lambda: fresh.pooled_get('probs', 0, 0, 0), lambda: fresh.pooled_get_pool('probs', 0, 0, 0),
                 lambda: check(fresh._lib.dmx_pooled_readout(fresh._h, *([None] * 10))),
                 lambda: check(fresh._lib.dmx_pooled_top_options(fresh._h, 1, None, None)),
                 lambda: check(fresh._lib.dmx_pooled_option_sums(fresh._h, None, None)),
                 lambda: check(fresh._lib.dmx_pooled_allowed_mass(fresh._h, None, None, None, None)))
        for call in calls:
            with pytest.raises(DemuxHipError, match='call order: .*before dmx_pooled_'):
                call()
        # an upload that is refused leaves the slot empty; one that is accepted fills it; release empties it
        with pytest.raises(DemuxHipError, match='dmx_pooled_upload: .*strictly ascending'):
            fresh.pooled_upload(4, [[2, 1]], np.zeros(2, np.int32), True, np.zeros(6, np.float32))
        assert fresh.pooled_info()['present'] == 0
        fresh.pooled_upload(4, [[1, 2]], np.zeros(2, np.int32), True, np.full(6, 0.25, np.float32))
        assert fresh.pooled_info()['present'] == 1
        with pytest.raises(DemuxHipError, match='dmx_pooled_upload: .*row_ptr gives'):  # a failed upload leaves the previous result
            arrays = (np.array([0, 2], np.int64), np.array([1, 2], np.int32), np.zeros(2, np.int32), np.array([0, 3, 5], np.int64), np.zeros(6, np.float32))
            check(fresh._lib.dmx_pooled_upload(fresh._h, 2, 4, 1, 1, arrays[0].ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data,
                                               arrays[3].ctypes.data, None, arrays[4].ctypes.data))
        same_bits(fresh.pooled_get('probs', 0, 2, 6), np.full(6, 0.25, np.float32), 'the previous upload')
        with pytest.raises(DemuxHipError, match='k is outside'):
            fresh.pooled_top_options(5)
        fresh.pooled_release()
        assert fresh.pooled_info()['present'] == 0


# ---- 2. slabs ---------------------------------------------------------------------------------------------------------------
def test_option_sums_over_slabs(ctx):
    """Two interleaved pools of 1300 and 513 barcodes (slabs of 3 and of 2 positions, the last ones short or empty) and stragglers."""
    rng = np.random.default_rng(19)
    pool_of = np.array([0] * 1300 + [1] * 513 + [-1] * 80 + [2] * 7, dtype=np.int32)
    pool_of = pool_of[rng.permutation(len(pool_of))]
    sizes = [2, 2, 2, 2]  # K = 3; the last pool has no barcodes
    row_ptr = restated.row_pointer(sizes, pool_of, True)
    probs = softmax_rows(rng, row_ptr)
    ctx.pooled_upload(2, [[0, 1]] * 4, pool_of, True, probs)
    sums, counts = ctx.pooled_option_sums(12)
    want_sums, want_counts = restated.option_sums(probs, row_ptr, pool_of, sizes, True)
    assert counts.tolist() == [1300, 513, 7, 0] == want_counts.tolist()
    same_bits(sums, want_sums, 'slab sums')
    assert not sums[9:].any()
    want = restated.readout(probs, row_ptr, pool_of, sizes, True)
    got = ctx.pooled_readout(marginals=True)
    for key in want:
        same_bits(got[key], want[key], key)


# ---- 3. kept passes -----------------------------------------------------------------------------------------------------------
SMALL, EXTRA = 'f3_small_2.npz', 3
POOLS = [[0, 1, 2, 3, 4], [1, 3], [2]]


@pytest.fixture(scope='module')
def problem():
    """The small designed problem of tests/test_gpu_pools.py (barcodes without calls, barcodes in no pool), on a context of its own."""
    from demuxalot_amd.device import DeviceContext
    fx = fio.load(SMALL)
    v, cb, e, prob, B = pools_restatement.fixture_problem(SMALL, 0.01)
    B += EXTRA
    with DeviceContext(0) as context:
        context.set_problem(B, len(fx['pack_v2snp']), prob.shape[1], v, cb, e, fx['pack_v2snp'])
        context.set_betas(fx['pack0_betas'])
        context.set_addition(None)
        context.probs_from_betas(0.01)
        pool_of = (np.arange(B) % 4 - 1).astype(np.int32)
        pool_of[B - EXTRA:] = [0, 1, -1]
        yield context, pool_of, B


def passes(ctx, pool_of, B, with_doublets=True):
    penalty = np.array([-0.5, -1.25, 0.0], np.float32)
    alpha = (np.arange(B) % 5 * 0.1).astype(np.float32)
    grid = np.array([0.0, 0.3, 0.05, 0.6], np.float32)
    return {
        'pools': lambda: ctx.estep_pools(POOLS, pool_of, with_doublets, penalty),
        'ambient': lambda: ctx.estep_ambient(POOLS, pool_of, with_doublets, penalty, alpha),
        'grid': lambda: ctx.estep_ambient_grid(POOLS, pool_of, with_doublets, penalty, grid),
        'marginal': lambda: ctx.estep_ambient_grid(POOLS, pool_of, with_doublets, penalty, grid, over_grid='marginal',
                                                   log_weights=np.array([0.0, -0.5, -0.1, -2.0], np.float32)),
    }


@pytest.mark.parametrize('name', ['pools', 'ambient', 'grid', 'marginal'])
def test_kept_pass_is_the_pass(problem, name):
    ctx, pool_of, B = problem
    run = passes(ctx, pool_of, B)[name]
    ctx.pooled_release()
    ctx.set_keep_pooled(False)
    off = run()
    assert ctx.pooled_info()['present'] == 0, 'nothing is kept with the switch off'
    ctx.set_keep_pooled(True)
    try:
        on = run()
    finally:
        ctx.set_keep_pooled(False)
    assert set(on) == set(off)
    for key in on:
        if on[key] is not None:
            same_bits(on[key], off[key], f'{name}: {key} with keep on')
    n = int(on['row_ptr'][-1])
    info = ctx.pooled_info()
    assert info == dict(present=1, B=B, n_pools=3, n_values=n, with_doublets=1, has_logits=1, has_alpha_index=int(name in ('grid', 'marginal')),
                        has_alpha_mean=int(name == 'marginal'))
    held = [('logits', on['logits']), ('probs', on['probs'])]
    if info['has_alpha_index']:
        held.append(('alpha_index', on['alpha_index']))
    if info['has_alpha_mean']:
        held.append(('alpha_mean', on['alpha_mean']))
    for what, values in held:
        same_bits(ctx.pooled_get(what, 0, B, n), values, f'{name}: get {what}')
        for p, columns in enumerate(POOLS):
            frame = restated.pool_frame(values, on['row_ptr'], pool_of, p)
            same_bits(ctx.pooled_get_pool(what, p, len(frame), frame.shape[1]), frame, f'{name}: get_pool {what} {p}')
    r = ctx.pooled_readout(marginals=True)
    for key in ('best_option', 'best_prob', 'doublet_mass'):
        same_bits(r[key], on[key], f'{name}: {key} of the read-out against the pass')
    want = restated.readout(on['probs'], on['row_ptr'], pool_of, [len(c) for c in POOLS], True)
    for key in want:
        same_bits(r[key], want[key], f'{name}: {key}')
    # NULL row outputs: the B-sized read-outs are the same, the slot is the same
    ctx.set_keep_pooled(True)
    try:
        kwargs = dict(fetch_logits=False, fetch_probs=False)
        penalty = np.array([-0.5, -1.25, 0.0], np.float32)
        if name == 'pools':
            lean = ctx.estep_pools(POOLS, pool_of, True, penalty, **kwargs)
            for key in ('best_option', 'best_prob', 'doublet_mass'):
                same_bits(lean[key], on[key], f'lean {key}')
            same_bits(ctx.pooled_get('probs', 0, B, n), on['probs'], 'lean: get probs')
    finally:
        ctx.set_keep_pooled(False)


def test_slot_life_cycle(problem):
    ctx, pool_of, B = problem
    from demuxalot_amd._lib import DemuxHipError
    penalties = pools_restatement.demux_oracle.doublet_penalties(ctx.G, 0.35)
    run = passes(ctx, pool_of, B)
    ctx.pooled_release()
    _logits, probs = ctx.estep(penalties, True)
    dense = ctx.get_donor_readout(marginals=True)
    ctx.set_keep_pooled(True)
    try:
        first = run['grid']()
        n = int(first['row_ptr'][-1])
        # the slot survives the dense path, whose results are those of a run without it
        _logits, again = ctx.estep(penalties, True)
        same_bits(again, probs, 'dmx_estep with a slot')
        for key, values in ctx.get_donor_readout(marginals=True).items():
            same_bits(values, dense[key], f'dmx_get_donor_readout with a slot: {key}')
        assert ctx.pooled_info()['has_alpha_index'] == 1
        same_bits(ctx.pooled_get('probs', 0, B, n), first['probs'], 'the slot after dmx_estep')
        same_bits(ctx.pooled_get('alpha_index', 0, B, n), first['alpha_index'], 'the slot after dmx_estep')
        # a second kept pass replaces the first
        singlets = passes(ctx, pool_of, B, with_doublets=False)['pools']()
        info = ctx.pooled_info()
        assert info['with_doublets'] == 0 and info['n_values'] == int(singlets['row_ptr'][-1]) < n and info['has_alpha_index'] == 0
        same_bits(ctx.pooled_get('probs', 0, B, info['n_values']), singlets['probs'], 'the second result')
        # a failed call leaves the previous one in place
        with pytest.raises(DemuxHipError):
            ctx.estep_pools([[1, 0]], np.zeros(B, np.int32), True, np.zeros(1, np.float32))
        assert ctx.pooled_info() == info
        same_bits(ctx.pooled_get('probs', 0, B, info['n_values']), singlets['probs'], 'after a refused call')
        # the resident and EM entries never touch it
        penalty = np.array([-0.5, -1.25, 0.0], np.float32)
        alpha = np.full(B, 0.1, np.float32)
        ctx.estep_pools(POOLS, pool_of, True, penalty, resident=True)
        ctx.estep_ambient(POOLS, pool_of, True, penalty, alpha, resident=True)
        ctx.em_pools(1, 0.01, POOLS, pool_of, True, penalty)
        ctx.em_ambient(1, 0.01, POOLS, pool_of, True, penalty, alpha)
        assert ctx.pooled_info() == info
        same_bits(ctx.pooled_get('probs', 0, B, info['n_values']), singlets['probs'], 'after the resident and EM entries')
    finally:
        ctx.set_keep_pooled(False)
    # dmx_release_problem drops it
    ctx.release_problem()
    assert ctx.pooled_info()['present'] == 0


# ---- 4. the front door ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shipped():
    fx = fio.load('f6_shipped_example.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    pool2donors = {'A': [donors[1], donors[0]], 'B': [donors[3], donors[1], donors[2]]}
    barcode2pool = {bc: (None if i % 5 == 4 else 'AB'[i % 2]) for i, bc in enumerate(barcodes)}
    return calls, genotypes, handler, donors, pool2donors, barcode2pool


def check_against_host(device, host, with_doublets=True, threshold=0.6):
    """A DevicePooledPosteriors against the PooledPosteriors of the host route on the same inputs."""
    back = device.to_host()
    for field in ('pool_of_barcode', 'row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass'):
        same_bits(getattr(back, field), getattr(host, field), f'to_host().{field}')
    assert back.barcodes == host.barcodes and back.pools == host.pools == device.pools
    pool_of, row_ptr, probs = host.pool_of_barcode, host.row_ptr, host.probs
    names = host.pools
    columns = [host.columns_of(pool) for pool in names]
    sizes = list(device._pool_sizes)
    assert [len(cols) for cols in columns] == [restated.n_options(g, with_doublets) for g in sizes]
    donors = [cols[:g] for cols, g in zip(columns, sizes)]
    r = restated.readout(probs, row_ptr, pool_of, sizes, with_doublets)
    for pool in names:
        for got, want in zip(device.to_dataframes(pool), host.to_dataframes(pool)):
            assert list(got.columns) == list(want.columns) and list(got.index) == list(want.index) and got.index.name == want.index.name
            same_bits(got.values, want.values, f'to_dataframes({pool!r})')
        assert device.columns_of(pool) == host.columns_of(pool) and device.barcodes_of(pool) == host.barcodes_of(pool)
    got_best, want_best = device.best(), host.best()
    assert list(got_best.index) == list(want_best.index) and list(got_best.columns) == list(want_best.columns)
    assert list(got_best['pool'].values) == list(want_best['pool'].values) and list(got_best['option'].values) == list(want_best['option'].values)
    same_bits(got_best['probability'].values, want_best['probability'].values, 'best(): probability')
    got_assigned, want_assigned = device.assignments(threshold), host.assignments(threshold)
    assert list(got_assigned.index) == list(want_assigned.index) and list(got_assigned.values) == list(want_assigned.values) and len(want_assigned)
    same_bits(device.doublet_probability().values, host.doublet_mass, 'doublet_probability()')
    # droplet calls, summaries, marginals, option sums: the restatement on the host route's rows
    want_calls = restated.calls(r, pool_of, names, donors, with_doublets, threshold)
    got_calls = device.droplet_calls(threshold)
    assert list(got_calls.index) == host.barcodes and list(got_calls.columns) == list(want_calls.columns)
    for column in ('pool', 'status', 'donor_1', 'donor_2'):
        assert list(got_calls[column].values) == list(want_calls[column].values), column
    for column in ('probability', 'doublet_probability'):
        same_bits(got_calls[column].values.astype(np.float64), want_calls[column].values.astype(np.float64), column)
    sums, _counts = restated.option_sums(probs, row_ptr, pool_of, sizes, with_doublets)
    want_summary = restated.summary(want_calls, sums, names, donors, with_doublets)
    got_summary = device.donor_summary(threshold)
    assert list(got_summary.index) == list(want_summary.index)
    assert np.array_equal(got_summary['n_singlets'].values, want_summary['n_singlets'].values)
    assert np.array_equal(got_summary['n_doublets'].values, want_summary['n_doublets'].values)
    same_bits(got_summary['expected_cells'].values.astype(np.float64), want_summary['expected_cells'].values.astype(np.float64), 'expected_cells')
    first = 0
    for p, pool in enumerate(names):
        rows = restated.rows_of(pool_of, p)
        marginals = device.donor_marginals(pool)
        assert list(marginals.columns) == donors[p] and list(marginals.index) == host.barcodes_of(pool)
        want = np.stack([r['donor_marginals'][r['marg_ptr'][b]:r['marg_ptr'][b + 1]] for b in rows]) if len(rows) else np.zeros((0, sizes[p]), np.float32)
        same_bits(marginals.values, want, f'donor_marginals({pool!r})')
        K = len(columns[p])
        same_bits(device.option_sums(pool).values, sums[first:first + K], f'option_sums({pool!r})')
        first += K
    top = device.top_options(2)
    want_options, want_probs = restated.top_options(probs, row_ptr, 2)
    same_bits(top['probability_2'].values, want_probs[:, 1], 'top_options: second probability')
    # qualities: two possible options per pooled barcode, the first of its pool and its best one
    possible = {}
    for b, barcode in enumerate(host.barcodes):
        if pool_of[b] >= 0:
            cols = columns[pool_of[b]]
            possible[barcode] = [cols[0], cols[-1]] if b % 3 else [cols[0]]
    position = [{name: k for k, name in enumerate(cols)} for cols in columns]
    start, flat = [0], []
    for b, barcode in enumerate(host.barcodes):
        if pool_of[b] >= 0:
            flat.extend(position[pool_of[b]][o] for o in possible[barcode])
        start.append(len(flat))
    mass, hit = restated.allowed_mass(probs, row_ptr, pool_of, np.asarray(start), np.asarray(flat, np.int32))
    pooled_rows = pool_of >= 0
    got_q = device.qualities(possible)
    assert got_q['logloss'] == np.mean(-np.log(np.maximum(mass[pooled_rows], 1e-4))) and got_q['accuracy'] == np.mean(hit[pooled_rows] != 0)
    with pytest.raises(ValueError, match='not options of its pool'):
        device.qualities({barcode: ['nobody'] for barcode in host.barcodes})


def test_front_door_in_pools():
    from demuxalot_amd import Demultiplexer, DevicePooledPosteriors
    calls, genotypes, handler, _donors, pool2donors, barcode2pool = shipped()
    for dp in (0.35, 0.0):
        host = Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, doublet_prior=dp)
        with Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, doublet_prior=dp, on_device=True) as device:
            assert isinstance(device, DevicePooledPosteriors)
            check_against_host(device, host, with_doublets=dp != 0)


@pytest.mark.parametrize('pooled', [True, False])
def test_front_door_with_ambient(pooled):
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    calls, genotypes, handler, _donors, pool2donors, barcode2pool = shipped()
    barcodes = handler.ordered_barcodes
    fractions = {bc: 0.05 * (i % 4) for i, bc in enumerate(barcodes)}
    kwargs = dict(barcode2pool=barcode2pool, pool2donors=pool2donors) if pooled else {}
    host = Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, fractions, **kwargs)
    with Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, fractions, on_device=True, **kwargs) as device:
        if pooled:
            check_against_host(device, host)
            return
        assert device.pools == ['all']
        logits_df, probs_df = host
        back = device.to_host()
        B, K = probs_df.shape
        same_bits(back.probs.reshape(B, K), probs_df.values, 'unpooled: probs')
        same_bits(back.logits.reshape(B, K), logits_df.values, 'unpooled: logits')
        assert device.columns_of('all') == list(probs_df.columns)
        check_against_host(device, PooledPosteriors(barcodes, ['all'], [list(probs_df.columns)], np.zeros(B, np.int32), np.arange(B + 1) * K,
                                                    logits_df.values.reshape(-1), probs_df.values.reshape(-1), back.best_option, back.best_prob,
                                                    back.doublet_mass, index_name='BARCODE'))
        assert np.array_equal(back.best_option, probs_df.values.argmax(axis=1))


@pytest.mark.parametrize('pooled', [True, False])
@pytest.mark.parametrize('over_grid', ['max', 'marginal'])
def test_front_door_joint_ambient(pooled, over_grid):
    from demuxalot_amd import DeviceJointAmbientPosteriors, Demultiplexer, PooledPosteriors
    calls, genotypes, handler, _donors, pool2donors, barcode2pool = shipped()
    barcodes = handler.ordered_barcodes
    kwargs = dict(alphas=[0.0, 0.2, 0.05, 0.5], over_grid=over_grid)
    if pooled:
        kwargs.update(barcode2pool=barcode2pool, pool2donors=pool2donors)
    if over_grid == 'marginal':
        kwargs.update(alpha_log_weights=[0.0, -1.0, -0.25, -3.0])
    host = Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, **kwargs)
    with pytest.raises(ValueError, match='keep_profile with on_device'):
        Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, alphas=[0.0, 0.2], keep_profile=True, on_device=True)
    with Demultiplexer.predict_posteriors_joint_ambient(calls, genotypes, handler, on_device=True, **kwargs) as device:
        assert isinstance(device, DeviceJointAmbientPosteriors)
        same_bits(device.ambient, host.ambient, 'ambient')
        same_bits(device.best_alpha_index, host.best_alpha_index, 'best_alpha_index')
        if pooled:
            host_posteriors = host.posteriors
        else:
            logits_df, probs_df = host.posteriors
            B, K = probs_df.shape
            host_posteriors = PooledPosteriors(barcodes, ['all'], [list(probs_df.columns)], np.zeros(B, np.int32), np.arange(B + 1) * K,
                                               logits_df.values.reshape(-1), probs_df.values.reshape(-1), host.best_option, host.best_prob,
                                               host.doublet_mass, index_name='BARCODE')
        check_against_host(device.posteriors, host_posteriors)
        got, want = device.summary(), host.summary()
        assert list(got.columns) == list(want.columns) and list(got.index) == list(want.index)
        for column in want.columns:
            if want[column].dtype.kind == 'f':
                same_bits(got[column].values, want[column].values, f'summary: {column}')
            else:
                assert list(got[column].values) == list(want[column].values), column
        for barcode in (barcodes[0], barcodes[3], barcodes[4]):  # (the last one is in no pool when pooled)
            a, b = device.alphas_of(barcode), host.alphas_of(barcode)
            assert list(a.index) == list(b.index)
            same_bits(a.values.astype(np.float64), b.values.astype(np.float64), f'alphas_of({barcode!r})')
        n = int(host.row_ptr[-1])
        same_bits(device.posteriors._ctx.pooled_get('alpha_index', 0, len(barcodes), n), host.alpha_index, 'alpha_index')
        if over_grid == 'marginal':
            same_bits(device.best_alpha_mean, host.best_alpha_mean, 'best_alpha_mean')
            same_bits(device.posteriors._ctx.pooled_get('alpha_mean', 0, len(barcodes), n).astype(np.float64), host.option_alpha_means, 'alpha_mean')
            b = barcodes[0]
            same_bits(device.alpha_means_of(b).values, host.option_alpha_means[host.row_ptr[0]:host.row_ptr[1]], 'alpha_means_of')


def test_private_context_comes_back_clean():
    """close() hands the context back with the switch off and the slot dropped: the next holder sees neither."""
    from demuxalot_amd import Demultiplexer
    from demuxalot_amd.device import acquire_private_context, release_private_context
    calls, genotypes, handler, _donors, pool2donors, barcode2pool = shipped()
    device = Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, on_device=True)
    assert device._ctx.pooled_info()['present'] == 1
    device.close()
    device.close()  # twice is fine
    ctx = acquire_private_context()
    try:
        assert ctx.pooled_info()['present'] == 0
    finally:
        release_private_context(ctx)
