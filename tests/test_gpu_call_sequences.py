"""The incremental M-step across separate C API calls, on every exchange.

The incremental M-step (kernels.h: MIncrArgs) keeps integer sums on the device between two M-steps and, after a full pass, rewrites
only the rows of the variants whose barcodes changed.  Whether that is right depends on host state (the context's incr_valid) staying
true to what the device buffers hold while OTHER calls land between two M-steps: fetches of the addition (which assemble the sliced
table), dmx_get_learnt_betas, dmx_set_addition, a switch of the M-step form.  One call sequence - em, run_iterations, the staged
iterations of distributed.staged_genotype_learning, fetches, a replaced addition, a form switch - runs identically on every rank of
each exchange, and after every step
  (a) posteriors and additions equal, bit for bit, the same sequence on contexts that never keep sums (_prepare);
  (b) every fetched addition is within the fixed-point bound of a float64 np.bincount of the gathered singlet posteriors of the E-step
      before it (tests/test_gpu_configs.py: addition_rows, in float64) - this catches lost contributions even if the control were
      wrong the same way;
  (c) the delta passes did happen across the fetches, wherever the incremental M-step applies.
The exact E-step (deterministic) with the exact additions off (the incremental M-step live), as a guarded run with
dmx_set_guard_adaptive(ctx, 0) does too."""
import functools
import hashlib

import numpy as np
import pytest

from tests import fixture_io as fio
from tests.thread_plane import ThreadWorld

pytestmark = pytest.mark.gpu

CLIP, POWER = 0.01, 2.0


@functools.lru_cache(maxsize=None)
def _workload(doublets):
    """Separable donors, 400 calls per barcode: the posteriors converge, so the later M-steps are delta passes."""
    from demuxalot_amd import Demultiplexer, synth
    G = 16 if doublets else 40
    p = synth.generate(9_000, 2_500, G, calls_per_barcode=400, doublets=doublets, seed=79 if doublets else 78)
    pen = Demultiplexer._doublet_penalties(G, 0.2 if doublets else 0.0)
    return p, pen


_REFERENCE = {}


def _reference_addition(p, post_singlets):
    """demux.py:113-118 in float64: contributions (posterior x (1 - p_base_wrong)) ** power in float32 as the reference forms them,
    summed per variant by np.bincount; kept per posterior table (every configuration with the same posteriors asks for the same)."""
    key = (id(p), hashlib.sha1(np.ascontiguousarray(post_singlets).tobytes()).hexdigest())
    if key not in _REFERENCE:
        keep = 1 - p.p_base_wrong
        cols = np.ascontiguousarray(post_singlets.T)
        out = np.empty((p.n_variants, cols.shape[0]), dtype=np.float64)
        for g in range(cols.shape[0]):
            w = cols[g][p.compressed_cb] * keep
            w **= np.float32(POWER)
            out[:, g] = np.bincount(p.variant_id, weights=w, minlength=p.n_variants)
        _REFERENCE[key] = out
    return _REFERENCE[key]


def assert_within_bound(got, want, p, ulps, what):
    """|got - want| <= ulps 2^-24 |want| + n(v) 2^-50 per entry (n(v) = calls of the variant).  The fixed-point sums
    (tests/test_gpu_mstep_tiles.py: assert_within_tile_bound) are within n(v) 2^-51 of the real sum, the float64 forms far closer;
    float64 on the wire: one rounding to float32 at the end, ulps = 2.  float32 on the wire: every rank rounds its partial sum
    (together at most 2^-24 of the total: the partials are non-negative), the world - 1 float32 additions of the reduce-scatter
    round once each (2^-24 of the total each), store_slice moves the result as it is: ulps = world + 1."""
    counts = np.bincount(p.variant_id, minlength=p.n_variants).astype(np.float64)[:, None]
    dev = np.abs(got.astype(np.float64) - want)
    bound = ulps * 2.0 ** -24 * np.abs(want) + counts * 2.0 ** -50
    bad = ~(dev <= bound)
    assert np.isfinite(got).all() and not bad.any(), (what, int(bad.sum()), float((dev - bound).max()), float(dev.max()))


def _staged(ctx, pen, doublets, fetch):
    """One iteration of distributed.staged_genotype_learning: P-step, E-step, M-step (with or without the addition)."""
    ctx.probs_from_betas(CLIP, fetch=False)
    _logits, probs = ctx.estep(pen, with_doublets=doublets, fetch_logits=False)
    return probs, ctx.mstep(POWER, fetch=fetch)


def _sequence(ctx, pen, doublets, p=None):
    """The call sequence; returns [(step, posteriors, addition, whether `addition` is the M-step of `posteriors`, learnt betas,
    (full, delta) M-step passes the step took)].  Identical on every rank (the fetches are collective).  `p`: a context without a
    communicator, which also takes the float64 M-step of aggregate_on_snps in between (it writes the whole addition)."""
    out = []
    ctx.reset_timings()
    seen = [(0, 0)]

    def passes():
        full, delta, _last = ctx.mstep_incremental()
        took = (full - seen[0][0], delta - seen[0][1])
        seen[0] = (full, delta)
        return took

    _l, probs, addition = ctx.em(4, CLIP, pen, doublets, fetch_logits=False)
    out.append(('1 em(4)', probs, addition, False, None, passes()))
    ctx.run_iterations(3, CLIP, POWER)
    addition = ctx.get_addition()
    out.append(('2 run_iterations(3), get_addition, get_probs', ctx.get_probs(), addition, True, None, passes()))
    for i in range(3):
        probs, addition = _staged(ctx, pen, doublets, True)
        out.append((f'3 staged iteration {i}, mstep(fetch=True)', probs, addition, True, None, passes()))
    learnt = ctx.get_learnt_betas()
    for i in range(2):
        probs, _none = _staged(ctx, pen, doublets, False)
    addition = ctx.get_addition()
    out.append(('4 get_learnt_betas, 2 staged iterations mstep(fetch=False), get_addition', probs, addition, True, learnt, passes()))
    ctx.set_addition(None)
    for i in range(2):
        probs, addition = _staged(ctx, pen, doublets, True)
        out.append((f'5 set_addition(None), staged iteration {i}', probs, addition, True, None, passes()))
    ctx.set_mstep_tiles('always')
    for i in range(2):
        probs, addition = _staged(ctx, pen, doublets, True)
        out.append((f'6 set_mstep_tiles(always), staged iteration {i}', probs, addition, True, None, passes()))
    if p is not None:
        from demuxalot_amd import Demultiplexer
        ctx.set_molecule_calls(p.variant_id, p.compressed_cb, p.p_base_wrong)
        ctx.probs_from_betas(CLIP, fetch=False)
        ctx.estep_snp(doublets, Demultiplexer.compensation_during_computing_barcode_logits)
        f64 = ctx.mstep_f64(POWER)
        out.append(('7 estep_snp, mstep_f64', None, f64, False, None, passes()))
        for i in range(2):
            probs, addition = _staged(ctx, pen, doublets, True)
            out.append((f'7 after mstep_f64, staged iteration {i}', probs, addition, True, None, passes()))
    return out


def _prepare(ctx, p, incremental, guarded, own_sums):
    """The control (incremental off) takes the full tile pass at every M-step where the incremental M-step would add the tile form's
    integers from the first M-step on (one context, a rank that reduce-scatters its sums); elsewhere both start on the float64 work items
    and take the tile-major records from the 8th M-step on."""
    ctx.set_mstep_incremental(incremental)
    ctx.set_mstep_tiles('always' if own_sums and not incremental else 'auto')
    if guarded:
        ctx.set_guard_adaptive(False)   # (else the guarded level is chosen on the device's timings: two runs need not agree)
    # the raw betas, so that dmx_get_learnt_betas has them; the molecule counts of ALL ranks (each holds only its barcodes' calls)
    ctx.set_prior_betas(p.raw_betas, p.default_prior, True, mol_per_variant=np.bincount(p.variant_id, minlength=p.n_variants).astype(np.int64),
                        fetch=False)


def _run_ranks(p, pen, doublets, world, wire, incremental, guarded):
    """[(lo, hi, sequence record, exchange mode)] of every rank."""
    from demuxalot_amd import distributed
    shared = ThreadWorld(world)

    def rank_body(plane):
        em = distributed.ShardedEM(plane, p.n_barcodes, p.v2snp, p.prior_betas(), p.variant_id, p.compressed_cb, p.p_base_wrong,
                                   reduce_dtype=wire)
        try:
            _prepare(em.ctx, p, incremental, guarded, world == 1 or em.ctx.exchange_mode() == 'reduce_scatter')
            return em.lo, em.hi, _sequence(em.ctx, pen, doublets, p if world == 1 else None), em.ctx.exchange_mode()
        finally:
            em.ctx.close()

    return shared.run(rank_body)


def _run_emulated(p, pen, nranks, incremental):
    from demuxalot_amd.device import DeviceContext
    with DeviceContext(0) as ctx:
        ctx.comm_init_emulated(0, nranks, reduce_dtype='f64')
        ctx.set_problem(p.n_barcodes, p.n_variants, p.n_genotypes, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        _prepare(ctx, p, incremental, False, True)
        return [(0, p.n_barcodes, _sequence(ctx, pen, False), ctx.exchange_mode())]


def _against_control(got, want):
    """(a): every rank, every step, bit for bit."""
    for (lo, hi, seq, mode), (lo_c, hi_c, seq_c, mode_c) in zip(got, want):
        assert (lo, hi, mode) == (lo_c, hi_c, mode_c)
        for (step, probs, addition, _own, learnt, _passes), (_s, probs_c, addition_c, _o, learnt_c, _p) in zip(seq, seq_c):
            where = f'rank rows [{lo}, {hi}), step {step}'
            if probs is not None:
                fio.assert_bitwise(probs, probs_c, f'{where}: posteriors against the control')
            fio.assert_bitwise(addition, addition_c, f'{where}: addition against the control')
            if learnt is not None:
                fio.assert_bitwise(learnt, learnt_c, f'{where}: learnt betas against the control')


def _against_reference(p, results, ulps):
    """(b): the gathered singlet posteriors of the E-step before each M-step, recomputed in float64."""
    G = p.n_genotypes
    for i, (step, _probs, _addition, own, _learnt, _passes) in enumerate(results[0][2]):
        if not own:
            continue
        post = np.concatenate([seq[i][1][:, :G] for _lo, _hi, seq, _mode in results])
        assert post.shape == (p.n_barcodes, G)
        want = _reference_addition(p, post)
        for lo, hi, seq, _mode in results:
            assert_within_bound(seq[i][2], want, p, ulps, f'rank rows [{lo}, {hi}), step {step}: addition against float64')


def _assert_delta_passes(results):
    """(c): the fetches of steps 2 - 4 leave the kept sums alone - every M-step of steps 3 and 4 a delta pass, step 2 has some; the
    replaced addition of step 5 asks for a full pass, and so does the one the float64 M-step wrote (step 7)."""
    for lo, hi, seq, _mode in results:
        per_step = {}
        for step, _probs, _addition, _own, _learnt, (full, delta) in seq:
            k = step[0]
            f, d = per_step.get(k, (0, 0))
            per_step[k] = (f + full, d + delta)
        where = f'rank rows [{lo}, {hi}): (full, delta) passes per step {per_step}'
        assert per_step['2'][1] >= 1, where
        assert per_step['3'] == (0, 3) and per_step['4'] == (0, 2), where
        assert per_step['5'][0] >= 1, where
        assert per_step.get('7', (1, 0))[0] >= 1, where


CONFIGS = [(1, None, 'f64')] + [(world, exchange, wire) for world in (2, 3)
                                for exchange, wire in (('variant', 'f64'), ('reduce_scatter', 'f64'), ('reduce_scatter', 'f32'), ('allreduce', 'f64'))]


@pytest.mark.parametrize('world,exchange,wire', CONFIGS)
def test_call_sequence_on_every_exchange(world, exchange, wire, monkeypatch):
    monkeypatch.setenv('DEMUXALOT_AMD_ESTEP', 'exact')
    monkeypatch.setenv('DEMUXALOT_AMD_EXACT_ADDITIONS', '0')
    if exchange is None:
        monkeypatch.delenv('DEMUXALOT_AMD_EXCHANGE', raising=False)
    else:
        monkeypatch.setenv('DEMUXALOT_AMD_EXCHANGE', exchange)
    _check_ranks(world, exchange, wire, doublets=False, guarded=False)


def test_call_sequence_with_doublets(monkeypatch):
    monkeypatch.setenv('DEMUXALOT_AMD_ESTEP', 'exact')
    monkeypatch.setenv('DEMUXALOT_AMD_EXACT_ADDITIONS', '0')
    monkeypatch.setenv('DEMUXALOT_AMD_EXCHANGE', 'reduce_scatter')
    _check_ranks(3, 'reduce_scatter', 'f64', doublets=True, guarded=False)


def test_call_sequence_guarded(monkeypatch):
    monkeypatch.setenv('DEMUXALOT_AMD_ESTEP', 'guarded')
    monkeypatch.setenv('DEMUXALOT_AMD_EXACT_ADDITIONS', '0')
    monkeypatch.setenv('DEMUXALOT_AMD_EXCHANGE', 'reduce_scatter')
    _check_ranks(2, 'reduce_scatter', 'f64', doublets=False, guarded=True)


def _check_ranks(world, exchange, wire, doublets, guarded):
    p, pen = _workload(doublets)
    got = _run_ranks(p, pen, doublets, world, wire, True, guarded)
    want = _run_ranks(p, pen, doublets, world, wire, False, guarded)
    modes = {mode for _lo, _hi, _seq, mode in got}
    assert modes == {None if world == 1 else exchange}, modes
    print(f'world {world} {exchange} {wire}: (full, delta) passes per step of rank 0', [s[5] for s in got[0][2]])
    _against_control(got, want)
    _against_reference(p, got, world + 1 if wire == 'f32' and world > 1 else 2)
    if world == 1 or exchange == 'reduce_scatter':
        _assert_delta_passes(got)
    if exchange == 'allreduce':  # (the all-reduce sums in place: nothing is kept)
        assert all(s[5] == (0, 0) for _lo, _hi, seq, _mode in got for s in seq), [s[5] for s in got[0][2]]


def test_call_sequence_on_the_emulated_wire(monkeypatch):
    """Rank 0 of 4 over the emulated wire with the reduce-scatter exchange (scripts/emulated_scaling.py times this path): no EM of any
    experiment, so only against the control, and the delta passes."""
    monkeypatch.setenv('DEMUXALOT_AMD_ESTEP', 'exact')
    monkeypatch.setenv('DEMUXALOT_AMD_EXACT_ADDITIONS', '0')
    monkeypatch.setenv('DEMUXALOT_AMD_EXCHANGE', 'reduce_scatter')
    p, pen = _workload(False)
    got = _run_emulated(p, pen, 4, True)
    want = _run_emulated(p, pen, 4, False)
    assert got[0][3] == 'reduce_scatter'
    print('emulated rank 0 of 4: (full, delta) passes per step', [s[5] for s in got[0][2]])
    _against_control(got, want)
    _assert_delta_passes(got)


def _foreign_writer_sequence(p, pen, incremental):
    """em(4), two staged iterations, a dense pooled E-step + mstep_ambient at fraction 0, two staged iterations, a dense pooled E-step +
    mstep_doublets on its rows, two staged iterations: [(step, posteriors, addition, (full, delta) passes of the step)]."""
    from demuxalot_amd.device import DeviceContext
    pools, pool_of, no_penalty = [list(range(p.n_genotypes))], np.zeros(p.n_barcodes, np.int32), np.zeros(1, np.float32)
    out = []
    with DeviceContext(0) as ctx:
        ctx.set_problem(p.n_barcodes, p.n_variants, p.n_genotypes, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        _prepare(ctx, p, incremental, False, True)
        ctx.reset_timings()
        seen = [(0, 0)]

        def passes():
            full, delta, _last = ctx.mstep_incremental()
            took = (full - seen[0][0], delta - seen[0][1])
            seen[0] = (full, delta)
            return took

        def two_staged(behind):
            for i in range(2):
                probs, addition = _staged(ctx, pen, False, True)
                out.append((f'staged iteration {i} behind {behind}', probs, addition, passes()))

        def dense_pooled_estep():
            ctx.probs_from_betas(CLIP, fetch=False)
            return ctx.estep_pools(pools, pool_of, False, no_penalty, fetch_logits=False, resident=True)

        _l, probs, addition = ctx.em(4, CLIP, pen, False, fetch_logits=False)
        out.append(('em(4)', probs, addition, passes()))
        two_staged('em(4)')
        dense_pooled_estep()
        addition = ctx.mstep_ambient(np.zeros(p.n_barcodes, np.float32), POWER, CLIP)
        out.append(('mstep_ambient', ctx.get_probs(), addition, passes()))
        two_staged('mstep_ambient')
        rows = dense_pooled_estep()['probs']
        addition = ctx.mstep_doublets(pools, pool_of, False, no_penalty, rows, contribution_power=POWER)
        out.append(('mstep_doublets', ctx.get_probs(), addition, passes()))
        two_staged('mstep_doublets')
    return out


def test_foreign_writers_of_the_addition_between_incremental_msteps(monkeypatch):
    """The table-weighted M-steps write the whole addition and keep no sums (ctx_state.h: addition_written_by_other_form): one
    context without a communicator, incremental on against the incremental-off control.  Every posterior table and every addition
    equal the control's bit for bit, and by dmx_get_mstep_incremental the first mstep() behind each of the two writers is a full pass,
    the one after it a delta pass.  The pooled calls score singlets over one pool of all donors, as the workload's E-steps do."""
    monkeypatch.setenv('DEMUXALOT_AMD_ESTEP', 'exact')
    monkeypatch.setenv('DEMUXALOT_AMD_EXACT_ADDITIONS', '0')
    monkeypatch.delenv('DEMUXALOT_AMD_EXCHANGE', raising=False)
    p, pen = _workload(False)
    got = _foreign_writer_sequence(p, pen, True)
    want = _foreign_writer_sequence(p, pen, False)
    print('(full, delta) passes per step', [(step, took) for step, _p, _a, took in got])
    assert [s[0] for s in got] == [s[0] for s in want] and len(got) == 9
    for (step, probs, addition, _took), (_s, probs_c, addition_c, _t) in zip(got, want):
        fio.assert_bitwise(probs, probs_c, f'{step}: posteriors against the control')
        fio.assert_bitwise(addition, addition_c, f'{step}: addition against the control')
    took = {step: passes for step, _p, _a, passes in got}
    for writer in ('mstep_ambient', 'mstep_doublets'):
        assert took[writer] == (0, 0), (writer, took)  # (no pass of the incremental M-step's)
        assert took[f'staged iteration 0 behind {writer}'] == (1, 0), (writer, took)
        assert took[f'staged iteration 1 behind {writer}'] == (0, 1), (writer, took)
