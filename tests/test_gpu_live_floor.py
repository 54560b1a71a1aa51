"""The live floor of the barcode codes (csrc/kernels.h: live_floor_fixed; include/demux_hip_debug.h: dmx_set_live_floor_on_grid).  An E-step
that a fixed-point M-step will follow calls a posterior live from 2^-26 on instead of from 2^-80 on: below 2^-26 those M-step forms add the
integer 0.  Nothing may differ in any bit between the two floors - additions, posteriors, the incremental M-step's decisions -, no M-step may
have to rebuild the codes in steady state, and the float64 forms must never see codes written at the higher floor.

Small problems in the sparse regime with many posteriors in the band (2^-80, 2^-26): sibling donors, 3000 barcodes x 2000 SNPs x 400 calls per
barcode (numpy oracle, iteration 0, 64 genotypes: 52 % of the barcodes have a posterior in the band, 699 posteriors within (2^-30, 2^-22]; calls
of barcodes with more than 4 live posteriors: 11.6 % at 2^-80, 0.3 % at 2^-26); 33 and 17 genotypes (other lane shapes of the epilogue), and 8
genotypes with doublets (36 options: the codes cover the singlet columns only)."""
import functools

import numpy as np
import pytest

from tests.thread_plane import ThreadWorld

pytestmark = pytest.mark.gpu

FLOOR_F64 = np.float32(2.0 ** -80)                                 # live <=> p > 2^-80: what the float64 forms need
FLOOR_GRID = np.nextafter(np.float32(2.0 ** -26), np.float32(0))   # live <=> p >= 2^-26: what adds a non-zero integer somewhere

CASES = {'G64': (64, False), 'G33': (33, False), 'G17': (17, False), 'G8_doublets': (8, True)}


@functools.lru_cache(maxsize=None)
def _problem(name):
    from demuxalot_amd import Demultiplexer, synth
    G, doublets = CASES[name]
    p = synth.generate(3000, 2000, G, calls_per_barcode=400, sibling_pairs=True, seed=5)
    pen = Demultiplexer._doublet_penalties(G, 0.2 if doublets else 0.0)
    return p, G, doublets, pen, p.prior_betas()


def _context(name, grid, tiles='always', incremental=True, exact=False):
    from demuxalot_amd.device import DeviceContext
    p, G, _doublets, _pen, betas = _problem(name)
    ctx = DeviceContext(0)
    ctx.set_estep_mode('exact')  # the reference's posteriors under both floors
    ctx.set_exact_additions(exact)
    ctx.set_mstep_tiles(tiles)
    ctx.set_mstep_incremental(incremental)
    ctx.set_live_floor_on_grid(grid)
    ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
    ctx.set_betas(betas)
    ctx.set_addition(None)
    return ctx


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _assert_not_vacuous(name, post):
    """The case still has what it is there for (a change of the generator must not empty it): posteriors in the band, a sparse regime."""
    p, G, _doublets, _pen, _betas = _problem(name)
    singlets = post[:, :G]
    in_band = ((singlets > FLOOR_F64) & (singlets <= FLOOR_GRID)).any(axis=1).mean()
    calls = np.bincount(p.compressed_cb, minlength=p.n_barcodes)
    dense = calls[(singlets > FLOOR_F64).sum(axis=1) > 4].sum() / calls.sum()
    print(f'{name}: {in_band:.3f} of the barcodes with a posterior in the band, dense share at 2^-80 {dense:.3f}')
    assert in_band >= 0.20, (name, in_band)
    assert dense < 0.20, (name, dense)


def _one_mstep(name, grid, tiles, want_form):
    """(addition, posteriors) of one P-, E- and M-step; the codes checked against the posteriors on the way."""
    p, G, doublets, pen, _betas = _problem(name)
    ctx = _context(name, grid, tiles=tiles)
    try:
        ctx.probs_from_betas(0.01, fetch=False)
        _logits, post = ctx.estep(pen, with_doublets=doublets, fetch_logits=False)
        floor, rebuilds = ctx.live_floor()
        assert floor == (FLOOR_GRID if grid else FLOOR_F64) and rebuilds == 0, (floor, rebuilds)
        assert np.array_equal(ctx.debug_live_counts(), (~(post[:, :G] <= floor)).sum(axis=1)), 'live counts of the codes'
        addition = ctx.mstep()
        assert ctx.mstep_form() == want_form, ctx.mstep_form()  # (not the dense regime's kernel either: _assert_not_vacuous)
        assert ctx.live_floor() == (floor, 0), 'a fixed-point M-step takes the codes at either floor'
        return addition, post
    finally:
        ctx.close()


@pytest.mark.parametrize('tiles,form', [('always', 'tiles'), ('auto', 'items_fixed')])
@pytest.mark.parametrize('name', list(CASES))
def test_one_mstep_is_bit_identical_under_both_floors(name, tiles, form):
    add_off, post_off = _one_mstep(name, False, tiles, form)
    add_on, post_on = _one_mstep(name, True, tiles, form)
    _assert_not_vacuous(name, post_off)
    assert np.array_equal(_bits(post_off), _bits(post_on)), 'posteriors'
    assert np.isfinite(add_on).all() and add_on.max() > 0
    assert np.array_equal(_bits(add_off), _bits(add_on)), f'{name}: the addition of the {form} form differs between the floors'


def _six_iterations(name, grid, tiles):
    p, G, doublets, pen, _betas = _problem(name)
    ctx = _context(name, grid, tiles=tiles, incremental=True)
    try:
        ctx.reset_timings()
        additions, forms = [], []
        for _ in range(6):
            ctx.probs_from_betas(0.01, fetch=False)
            ctx.estep(pen, with_doublets=doublets, fetch_logits=False, fetch_probs=False)
            additions.append(ctx.mstep())
            forms.append(ctx.mstep_form())
        full, delta, _last = ctx.mstep_incremental()
        return additions, ctx.get_probs(), (full, delta), forms, ctx.live_floor()
    finally:
        ctx.close()


@pytest.mark.parametrize('tiles', ['always', 'auto'])
@pytest.mark.parametrize('name', ['G64', 'G8_doublets'])
def test_six_incremental_iterations_are_bit_identical_under_both_floors(name, tiles):
    off = _six_iterations(name, False, tiles)
    on = _six_iterations(name, True, tiles)
    assert set(on[3]) <= ({'tiles'} if tiles == 'always' else {'items_fixed', 'tiles'}) and on[3] == off[3], (on[3], off[3])
    for it, (a, b) in enumerate(zip(off[0], on[0])):
        assert np.array_equal(_bits(a), _bits(b)), f'{name}: addition of iteration {it}'
    assert np.array_equal(_bits(off[1]), _bits(on[1])), 'final posteriors'
    assert off[2] == on[2] and sum(on[2]) == 6, ('full / delta passes', off[2], on[2])
    assert on[4] == (FLOOR_GRID, 0) and off[4] == (FLOOR_F64, 0), 'no rebuild launch in steady state'


def test_a_plain_em_call_needs_no_rebuild_and_keeps_its_bits():
    p, G, doublets, pen, _betas = _problem('G64')
    out = {}
    for grid in (False, True):
        ctx = _context('G64', grid, tiles='auto')
        try:
            ctx.reset_timings()
            _logits, probs, addition = ctx.em(6, 0.01, pen, doublets, fetch_logits=False)
            out[grid] = probs, addition, ctx.mstep_incremental()[:2], ctx.live_floor()[1], ctx.mstep_form()
        finally:
            ctx.close()
    assert np.array_equal(_bits(out[False][0]), _bits(out[True][0])) and np.array_equal(_bits(out[False][1]), _bits(out[True][1]))
    assert out[False][2:] == out[True][2:] and out[True][3] == 0 and out[True][4] in ('items_fixed', 'tiles'), (out[False][2:], out[True][2:])


def test_a_float64_form_rebuilds_grid_codes_once():
    """The exact additions switched on between an E-step that expected a fixed-point M-step and the M-step: the codes are rebuilt at 2^-80,
    one launch, and the sums are those of codes written there in the first place."""
    p, G, doublets, pen, _betas = _problem('G64')
    out = {}
    for grid in (False, True):
        ctx = _context('G64', grid, tiles='always')
        try:
            ctx.reset_timings()
            ctx.probs_from_betas(0.01, fetch=False)
            ctx.estep(pen, with_doublets=doublets, fetch_logits=False, fetch_probs=False)
            assert ctx.live_floor() == ((FLOOR_GRID if grid else FLOOR_F64), 0)
            ctx.set_exact_additions(True)
            addition = ctx.mstep()
            assert ctx.mstep_form() == 'items'
            out[grid] = addition, ctx.live_floor()
            # the next E-step knows: the exact additions are on, its codes are the float64 forms'
            ctx.probs_from_betas(0.01, fetch=False)
            ctx.estep(pen, with_doublets=doublets, fetch_logits=False, fetch_probs=False)
            ctx.mstep(fetch=False)
            assert ctx.live_floor() == out[grid][1]
        finally:
            ctx.close()
    assert out[True][1] == (FLOOR_F64, 1) and out[False][1] == (FLOOR_F64, 0), (out[True][1], out[False][1])
    assert np.array_equal(_bits(out[False][0]), _bits(out[True][0])), 'the exact additions behind rebuilt codes'


def test_a_weighted_mstep_rebuilds_grid_codes_once():
    """The M-step under ambient fractions behind an E-step that expected a fixed-point M-step (csrc/mstep_weighted.hip:
    begin_weighted_mstep): the codes are rebuilt at 2^-80, one launch.  At fraction 0 and a table clipped at 0.01 the weight's r is
    exactly 1, so the sums are the exact additions of the same posteriors - those of codes written at 2^-80 in the first place."""
    p, G, doublets, pen, _betas = _problem('G64')
    out = {}
    for grid in (False, True):
        ctx = _context('G64', grid, tiles='always')
        try:
            ctx.reset_timings()
            ctx.probs_from_betas(0.01, fetch=False)
            _logits, post = ctx.estep(pen, with_doublets=doublets, fetch_logits=False)
            assert ctx.live_floor() == ((FLOOR_GRID if grid else FLOOR_F64), 0)
            out[grid] = ctx.mstep_ambient(np.zeros(p.n_barcodes, np.float32)), ctx.live_floor()
            if not grid:
                _assert_not_vacuous('G64', post)  # (posteriors between the two floors: a skipped rebuild changes bits)
                ctx.set_exact_additions(True)
                exact = ctx.mstep()
                assert ctx.mstep_form() == 'items' and ctx.live_floor() == (FLOOR_F64, 0)
        finally:
            ctx.close()
    assert out[True][1] == (FLOOR_F64, 1) and out[False][1] == (FLOOR_F64, 0), (out[True][1], out[False][1])
    assert np.isfinite(exact).all() and exact.max() > 0
    assert np.array_equal(_bits(out[False][0]), _bits(out[True][0])), 'the weighted additions behind rebuilt codes'
    assert np.array_equal(_bits(out[False][0]), _bits(exact)), 'at fraction 0 the weighted M-step is the exact plain one'
    assert np.array_equal(_bits(out[True][0]), _bits(exact)), 'behind rebuilt codes too'


def test_an_attached_context_keeps_the_float64_floor():
    """One rank with a communicator attached: its codes travel to ranks whose M-step forms are theirs to know."""
    from demuxalot_amd import distributed
    from demuxalot_amd.device import DeviceContext
    p, G, doublets, pen, betas = _problem('G17')

    def rank_body(plane):
        ctx = DeviceContext(0)
        try:
            ctx.set_estep_mode('exact')
            ctx.set_exact_additions(False)
            ctx.set_mstep_tiles('always')
            ctx.set_live_floor_on_grid(True)
            distributed.attach_communicator(ctx, plane, force=True)
            ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
            ctx.set_betas(betas)
            ctx.set_addition(None)
            ctx.probs_from_betas(0.01, fetch=False)
            ctx.estep(pen, with_doublets=doublets, fetch_logits=False, fetch_probs=False)
            return ctx.live_floor()
        finally:
            ctx.close()

    assert ThreadWorld(1).run(rank_body) == [(FLOOR_F64, 0)]


def test_runner_up_posteriors_on_both_sides_of_the_floor():
    """A caller's table (dmx_set_probs): 32 barcodes of two calls each, genotype 0 certain, the runner-up's posterior swept across 2^-26,
    the other two genotypes at about 1e-8 - inside the band, below the floor.  The code's live count: 1 where the runner-up is below 2^-26,
    2 where it is not; 4 at the float64 forms' floor."""
    from demuxalot_amd.device import DeviceContext
    from oracle import demux_oracle
    B, G = 32, 4
    V = 2 * B
    variant_id = np.arange(V, dtype=np.int32)
    compressed_cb = (np.arange(V) // 2).astype(np.int32)
    p_base_wrong = np.zeros(V, dtype=np.float32)  # keep 1, floor 1e-4
    v2snp = (np.arange(V) // 2).astype(np.int32)
    table = np.zeros((V, G), dtype=np.float32)
    table[:, 0] = 1.0
    # posterior of genotype 1 ~ (x + 1e-4) 1e-4 / 1.0001^2: 2^-26 = 1.49e-8 at x = 4.9e-5
    table[0::2, 1] = np.linspace(3e-5, 7e-5, B).astype(np.float32)
    pen = np.zeros(G, dtype=np.float32)
    want = demux_oracle.softmax_rows(demux_oracle.barcode_logits(variant_id, compressed_cb, p_base_wrong, table, B, 0.0))
    assert 4 <= (want[:, 1] >= np.float32(2.0 ** -26)).sum() <= B - 4, 'the design no longer straddles the floor'
    for grid in (True, False):
        ctx = DeviceContext(0)
        try:
            ctx.set_estep_mode('exact')
            ctx.set_exact_additions(False)
            ctx.set_mstep_tiles('always')
            ctx.set_live_floor_on_grid(grid)
            ctx.set_problem(B, V, G, variant_id, compressed_cb, p_base_wrong, v2snp)
            ctx.set_probs(table)
            _logits, post = ctx.estep(pen, with_doublets=False, fetch_logits=False)
            counts = ctx.debug_live_counts()
            addition = ctx.mstep()
            assert ctx.mstep_form() == 'tiles' and ctx.live_floor()[1] == 0
        finally:
            ctx.close()
        above = post[:, 1] > FLOOR_GRID
        assert 4 <= above.sum() <= B - 4, 'runner-up posteriors on both sides of the floor'
        assert ((post[:, 2:] > FLOOR_F64) & (post[:, 2:] <= FLOOR_GRID)).all(), 'the other genotypes sit inside the band'
        assert np.array_equal(counts, np.where(above, 2, 1) if grid else np.full(B, 4)), (grid, counts)
        if grid:
            on = addition
        else:
            assert np.array_equal(_bits(on), _bits(addition)), 'the addition under both floors'
