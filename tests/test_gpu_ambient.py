"""Ambient RNA fractions on the GPU (include/demux_hip_debug.h: dmx_ambient_profile; csrc/ambient_profile.hip; Demultiplexer.estimate_ambient).

The kernel has no tolerance arithmetic: everything is compared bit for bit.  The checker is tests/ambient_restatement.py - numpy and
the oracle, pinned to the reference's own logits in tests/test_ambient_cpu.py - and, for the alpha = 0 column of singlets, the
reference's captured predict_posteriors itself.  The shapes are the smallest at which the kernel can go wrong: grids of 1, 2, 63 and
64 values, rows on either side of the 8-call padding and of the 64-call chunk, singlets, pairs and skipped barcodes in one launch, barcodes without
calls."""
import functools

import numpy as np
import pytest

from tests import ambient_restatement as restated
from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests.pooled_helpers import at

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1, SMALL = helpers.F1, helpers.F3_SMALL[2]  # G = 20; G = 5
REFERENCE_FIXTURES = [F1, helpers.F2] + helpers.F3_SMALL
_resident = functools.lru_cache(maxsize=None)(helpers.new_resident)  # the contexts this module's own


def resident(name, clip=0.01, extra_barcodes=0):
    """(ctx, v, cb, e, prob, B, v2snp): a fixture's packed problem and its genotype table resident on a context of its own, one per
    (name, clip, extra_barcodes) however the call spells them; extra_barcodes: that many barcodes without any call behind the fixture's."""
    return _resident(name, float(clip), int(extra_barcodes))


def soup_of(name, clip=0.01):
    return _soup_of(name, float(clip))


@functools.lru_cache(maxsize=None)
def _soup_of(name, clip):
    _v, _cb, _e, _prob, _B, v2snp = restated.fixture_problem(name)
    return restated.derived_ambient(_v, v2snp, clip)


def mixed_assignment(B, G, period=3):
    """Singlets, pairs and skipped barcodes interleaved: b % period == 0 a singlet, 1 a pair, 2 skipped; the donors move along."""
    b = np.arange(B)
    d1 = (b * 7) % G
    d2 = np.where(b % period == 1, d1 + 1 + (b // period) % np.maximum(G - 1 - d1, 1), -1)
    pair_fits = d2 < G
    d2 = np.where(pair_fits, d2, -1)
    d1 = np.where(b % period == 2, -1, d1)
    return d1.astype(np.int32), np.where(d1 < 0, -1, d2).astype(np.int32)


def check(name, alphas, d1, d2, what, clip=0.01, extra=0, ambient=None):
    ctx, v, cb, e, prob, B, _v2snp = resident(name, 0.01, extra)
    soup = soup_of(name, clip) if ambient is None else ambient
    want = restated.restate(v, cb, e, prob, B, alphas, d1, d2, soup)
    got = ctx.ambient_profile(d1, d2, alphas, clip, ambient=ambient)
    restated.assert_same(got, want, what)
    return got, want


# ---- 1. the reference anchor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', REFERENCE_FIXTURES)
def test_alpha_zero_of_singlets_is_the_reference_logit(name):
    fx = fio.load(name)
    G = len(fx['genotype_names'])
    alphas = np.array([0.25, 0.0, 0.5], dtype=np.float32)
    for i in range(int(fx['n_predict'])):
        clip = float(fx[f'predict{i}_clip'])
        ctx, *_rest, B, _v2snp = resident(name, clip)
        reference = fx[f'predict{i}_logits']
        rows = np.arange(B)
        for shift in range(G):  # every (barcode, donor) once
            donor = ((rows + shift) % G).astype(np.int32)
            got = ctx.ambient_profile(donor, np.full(B, -1, np.int32), alphas, clip)
            fio.assert_bitwise(got['loglik'][:, 1], np.ascontiguousarray(reference[rows, donor]), f'{name} predict {i} shift {shift}')
            fio.assert_bitwise(got['ll_zero'], got['loglik'][:, 1], 'll_zero is that column')


# ---- 2. grid widths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', [1, 2, 63, 64])
def test_grid_widths(A):
    _ctx, *_rest, B, _v2snp = resident(SMALL)
    G = 5
    d1, d2 = mixed_assignment(B, G)
    rng = np.random.default_rng(A)
    # unsorted, with 0 (not in front where the grid has room) and with 1.0
    grid = np.linspace(0, 1, A, dtype=np.float32) if A > 1 else np.zeros(1, np.float32)
    grid = rng.permutation(grid)
    if A > 1 and grid[0] == 0:
        grid[[0, 1]] = grid[[1, 0]]
    got, want = check(SMALL, grid, d1, d2, f'{A} values, unsorted, with 0 and 1')
    assert not np.isnan(got['ll_zero'][d1 >= 0]).any() and (A == 1 or 1.0 in grid)
    # without 0: ll_zero is NaN for everybody
    no_zero = rng.permutation(np.linspace(0.05, 0.95, A, dtype=np.float32))
    got, _want = check(SMALL, no_zero, d1, d2, f'{A} values, no 0')
    assert np.isnan(got['ll_zero']).all() and (got['best'][d1 >= 0] >= 0).all()
    # one value A times: every column ties, best is the lowest index
    got, _want = check(SMALL, np.full(A, 0.125, np.float32), d1, d2, f'{A} equal values')
    assert (got['best'][d1 >= 0] == 0).all() and (got['best'][d1 < 0] == -1).all()
    # the maximum duplicated: the grid twice over, second copy first
    if A >= 2:
        half = np.linspace(0, 0.6, A // 2, dtype=np.float32)
        twice = np.concatenate([half[::-1], half, np.full(A - 2 * len(half), half[0], np.float32)])
        got, want = check(SMALL, twice, d1, d2, f'{A} values, every value twice')
        assert (got['best'][d1 >= 0] < len(half)).all(), 'the first of two equal maxima'
    # alpha = 1 alone: the soup explains every call, whatever the donor
    one = np.ones(1, np.float32)
    rows, none = np.arange(B), np.full(B, -1, np.int32)
    got, _want = check(SMALL, one, (rows % G).astype(np.int32), none, 'alpha = 1')
    other, _want = check(SMALL, one, ((rows + 1) % G).astype(np.int32), none, 'alpha = 1, the next donor')
    fio.assert_bitwise(got['loglik'], other['loglik'], 'alpha = 1 does not depend on the donor')


# ---- 3. singlets, pairs and skipped barcodes in one launch ----------------------------------------------------------------------
def test_singlets_pairs_and_skipped_interleaved():
    _ctx, *_rest, B, _v2snp = resident(F1)
    d1, d2 = mixed_assignment(B, 20)
    assert (d1 < 0).sum() >= B // 4 and (d2 >= 0).sum() >= B // 4 and ((d1 >= 0) & (d2 < 0)).sum() >= B // 4
    assert len({(a, b) for a, b in zip(d1, d2)}) > 20, 'many different options'
    grid = np.linspace(0, 0.63, 64, dtype=np.float32)
    got, want = check(F1, grid, d1, d2, 'mixed assignment')
    skipped = d1 < 0
    assert (got['best'][skipped] == -1).all() and np.isnan(got['loglik'][skipped]).all()
    assert np.isnan(got['ll_best'][skipped]).all() and np.isnan(got['ll_zero'][skipped]).all()
    # everybody skipped, and the context is as usable afterwards
    nobody = np.full(B, -1, np.int32)
    empty, _ = check(F1, grid, nobody, nobody, 'everybody skipped')
    assert np.isnan(empty['loglik']).all() and (empty['best'] == -1).all()
    again, _ = check(F1, grid, d1, d2, 'after the empty call')
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), f'{key}: two runs differ'
    # the highest pair of the table, the first and the last donor
    last, _ = check(F1, grid, np.where(np.arange(B) % 2, 18, 0).astype(np.int32), np.full(B, 19, np.int32),
                    'pairs (18, 19) and (0, 19)')
    assert (last['best'] >= 0).all()


# ---- 4. barcodes without calls --------------------------------------------------------------------------------------------------
def test_barcodes_without_calls():
    extra = 3
    _ctx, *_rest, B, _v2snp = resident(SMALL, 0.01, extra)
    d1, d2 = mixed_assignment(B, 5)
    d1[B - extra:], d2[B - extra:] = [2, 0, -1], [-1, 4, -1]
    grid = np.array([0.3, 0.0, 0.6, 1.0], dtype=np.float32)
    got, _want = check(SMALL, grid, d1, d2, 'with empty barcodes', extra=extra)
    for b in (B - 3, B - 2):
        assert got['loglik'][b].view(np.uint32).tolist() == [0, 0, 0, 0], '+0.0 in every column'
        assert got['best'][b] == 0 and got['ll_best'][b].view(np.uint32) == 0 and got['ll_zero'][b].view(np.uint32) == 0
    assert got['best'][B - 1] == -1 and np.isnan(got['loglik'][B - 1]).all()


# ---- 5. row lengths around the padding and the batch ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def designed():
    """A problem whose barcodes have exactly 1, 7, 8, 9, 17, 0, 16, 24 and 25 calls (rows are padded to 8 calls) and 57, 64, 65, 128 and
    130 calls (the kernel stages 64 calls at a time: one chunk exactly, one and a group, two, two and two groups), on 3 donors and 80
    biallelic SNPs; error probabilities at both ends of their range among them."""
    from demuxalot_amd.device import DeviceContext
    rng = np.random.default_rng(5)
    lengths = [1, 7, 8, 9, 17, 0, 16, 24, 25, 57, 64, 65, 128, 130]
    V, G = 160, 3
    v2snp = np.repeat(np.arange(V // 2, dtype=np.int32), 2)
    v = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lengths]).astype(np.int32)
    cb = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    e = rng.choice(np.array([0.0, 1e-5, 1e-4, 0.01, 0.3, 1.0], dtype=np.float32), size=len(v))
    order = np.lexsort((cb, v))
    v, cb, e = v[order], cb[order], e[order]
    prob = rng.uniform(0.01, 0.99, size=(V, G)).astype(np.float32)
    prob[0] = [0.0, 1.0, 0.5]  # (row 0 is what the padding calls point at; the ends of the range)
    ctx = DeviceContext(0)
    ctx.set_problem(len(lengths), V, G, v, cb, e, v2snp)
    ctx.set_probs(prob)
    return ctx, v, cb, e, prob, len(lengths), v2snp, lengths


def test_row_lengths_on_either_side_of_the_padding():
    ctx, v, cb, e, prob, B, v2snp, lengths = designed()
    assert np.bincount(cb, minlength=B).tolist() == lengths
    grid = np.array([0.4, 0.0, 0.05, 1.0, 0.8], dtype=np.float32)
    soup = restated.derived_ambient(v, v2snp, 0.01)
    for what, d1, d2 in (('singlets', np.arange(B) % 3, np.full(B, -1)), ('pairs', np.arange(B) % 2, np.arange(B) % 2 + 1),
                         ('mixed', *mixed_assignment(B, 3))):
        d1, d2 = np.asarray(d1, np.int32), np.asarray(d2, np.int32)
        want = restated.restate(v, cb, e, prob, B, grid, d1, d2, soup)
        restated.assert_same(ctx.ambient_profile(d1, d2, grid), want, f'designed rows, {what}')
    got = ctx.ambient_profile(np.zeros(B, np.int32), np.full(B, -1, np.int32), grid)
    assert got['loglik'][5].view(np.uint32).tolist() == [0] * 5 and got['best'][5] == 0, 'the barcode without calls'


# ---- 6. derived against supplied ambient ----------------------------------------------------------------------------------------
def test_derived_and_supplied_profiles():
    ctx, v, cb, e, prob, B, v2snp = resident(F1)
    d1, d2 = mixed_assignment(B, 20)
    grid = np.array([0.0, 0.1, 0.3, 0.9], dtype=np.float32)
    for clip in (0.01, 0.1):
        derived, want = check(F1, grid, d1, d2, f'derived, clip {clip}', clip=clip)
        fio.assert_bitwise(derived['ambient'], restated.derived_ambient(v, v2snp, clip), f'ambient_out, clip {clip}')
        back = ctx.ambient_profile(d1, d2, grid, 0.45, ambient=derived['ambient'])  # (the clip is the derived profile's alone)
        for key in derived:
            assert derived[key].tobytes() == back[key].tobytes(), f'{key}: the profile supplied back'
    assert np.unique(soup_of(F1, 0.01)).size > 2 and soup_of(F1, 0.01).tobytes() != soup_of(F1, 0.1).tobytes(), 'the clip bites, not everywhere'
    other = np.random.default_rng(6).uniform(0, 1, size=len(v2snp)).astype(np.float32)
    other[:3] = [0.0, 1.0, 0.5]
    supplied, want = check(F1, grid, d1, d2, 'another profile', ambient=other)
    fio.assert_bitwise(supplied['ambient'], other, 'ambient_out is the supplied profile')
    assigned = d1 >= 0
    fio.assert_bitwise(supplied['loglik'][assigned, 0], derived['loglik'][assigned, 0], 'alpha = 0 does not see the profile')
    assert (supplied['loglik'][assigned, 1:] != derived['loglik'][assigned, 1:]).any()
    # the problem's own M-step and E-step results are none of this pass's business
    penalties = restated.demux_oracle.doublet_penalties(ctx.G, 0.35)
    _logits, probs = ctx.estep(penalties, True)
    check(F1, grid, d1, d2, 'behind an E-step')
    fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() after dmx_ambient_profile')


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def raw_call(ctx, alphas, d1, d2, ambient=None, n_alphas=None, B=None, V=None):
    """dmx_ambient_profile with the arrays as given: (status, message, whether an output was written)."""
    from demuxalot_amd import _lib
    alphas = None if alphas is None else np.asarray(alphas, np.float32)
    d1, d2 = np.asarray(d1, np.int32), np.asarray(d2, np.int32)
    ambient = None if ambient is None else np.asarray(ambient, np.float32)
    B, V = ctx.B if B is None else B, ctx.V if V is None else V
    A = (len(alphas) if alphas is not None else 0) if n_alphas is None else n_alphas
    outputs = [np.full(B * max(min(A, 64), 1), 7, np.float32), np.full(B, 7, np.int32), np.full(B, 7, np.float32), np.full(B, 7, np.float32),
               np.full(V, 7, np.float32)]
    status = ctx._lib.dmx_ambient_profile(ctx._h, 0.01, 0.99, A, _lib.ptr(alphas), _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(ambient),
                                          *[_lib.ptr(o) for o in outputs])
    return status, _lib.load().dmx_last_error().decode(), any((o != 7).any() for o in outputs)


def test_refusals_return_their_code_and_write_nothing():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)  # G = 5
    d1, d2 = mixed_assignment(B, 5)
    grid = [0.0, 0.5]
    soup = soup_of(SMALL)
    status, _text, written = raw_call(ctx, grid, d1, d2)
    assert status == 0 and written
    singlet = int(np.flatnonzero((d1 >= 0) & (d2 < 0))[0])
    cases = [
        (dict(alphas=[]), DMX_ERR_INVALID, 'at least one'),
        (dict(n_alphas=-1), DMX_ERR_INVALID, 'at least one'),
        (dict(alphas=np.zeros(65)), DMX_ERR_UNSUPPORTED, 'more than 64'),
        (dict(alphas=[0.0, np.nan]), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=[np.inf, 0.0]), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=[0.0, 1.5]), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=[0.0, -0.1]), DMX_ERR_INVALID, 'grid value'),
        (dict(alphas=None, n_alphas=2), DMX_ERR_INVALID, 'null alphas'),
        (dict(ambient=at(soup, 3, np.nan)), DMX_ERR_INVALID, 'ambient value'),
        (dict(ambient=at(soup, len(soup) - 1, 2.0)), DMX_ERR_INVALID, 'ambient value'),
        (dict(ambient=at(soup, 0, -0.5)), DMX_ERR_INVALID, 'ambient value'),
        (dict(d1=at(d1, singlet, 5)), DMX_ERR_INVALID, 'donor1 / donor2'),
        (dict(d1=at(d1, singlet, -2)), DMX_ERR_INVALID, 'donor1 / donor2'),
        (dict(d1=at(d1, singlet, 2), d2=at(d2, singlet, 2)), DMX_ERR_INVALID, 'donor1 / donor2'),
        (dict(d1=at(d1, singlet, 3), d2=at(d2, singlet, 1)), DMX_ERR_INVALID, 'donor1 / donor2'),
        (dict(d1=at(d1, singlet, 3), d2=at(d2, singlet, 5)), DMX_ERR_INVALID, 'donor1 / donor2'),
        (dict(d1=at(d1, B - 1, 0), d2=at(d2, B - 1, -3)), DMX_ERR_INVALID, 'donor1 / donor2'),
    ]
    launches = ctx.timings()['estep']['launches']
    good = dict(alphas=grid, d1=d1, d2=d2)
    for change, code, message in cases:
        status, text, written = raw_call(ctx, **{**good, **change})
        assert status == code and message in text and 'dmx_ambient_profile' in text, (change, status, text)
        assert not written, (change, 'a refused call writes nothing')
        assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    from demuxalot_amd._lib import DemuxHipError
    with pytest.raises(DemuxHipError, match=r'more than 64.*status -5'):
        ctx.ambient_profile(d1, d2, np.zeros(65, np.float32))
    check(SMALL, np.array(grid, np.float32), d1, d2, 'a valid call after the refused ones')
    assert ctx.timings()['estep']['launches'] == launches + 1, 'the pass is counted as an E-step'


def test_needs_a_problem_a_table_and_no_communicator():
    _v, _cb, _e, prob, B, _v2snp = restated.fixture_problem('f3_small_0.npz')
    args = dict(alphas=[0.0, 0.5], d1=np.zeros(B, np.int32), d2=np.full(B, -1, np.int32), B=B, V=len(prob))
    helpers.check_needs_problem_table_no_communicator(raw_call, 'dmx_ambient_profile', args)


# ---- 8. the read-outs alone -----------------------------------------------------------------------------------------------------
def test_read_outs_without_the_profile():
    ctx, *_rest, B, _v2snp = resident(F1)
    d1, d2 = mixed_assignment(B, 20)
    grid = np.linspace(0, 0.63, 64, dtype=np.float32)
    full = ctx.ambient_profile(d1, d2, grid)
    lean = ctx.ambient_profile(d1, d2, grid, fetch_profile=False)
    assert lean['loglik'] is None
    for key in ('best', 'll_best', 'll_zero', 'ambient'):
        assert lean[key].tobytes() == full[key].tobytes(), key


# ---- 9. the front door ----------------------------------------------------------------------------------------------------------
def test_estimate_ambient_end_to_end():
    from demuxalot_amd import AmbientEstimate, Demultiplexer, ResidentCalls
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    v, cb, e, prob, B, v2snp = restated.fixture_problem(F1)
    assert B == len(barcodes)
    options = restated.demux_oracle.option_names(donors, 0.35)
    d1, d2 = mixed_assignment(B, len(donors))
    columns = np.where(d1 < 0, -1, np.where(d2 < 0, d1, [options.index(f'{donors[a]}+{donors[max(b, 0)]}') if b >= 0 else -1 for a, b in zip(d1, d2)]))
    assignments = {}
    for b, (bc, k) in enumerate(zip(barcodes, columns)):
        if b % 6 == 2:
            continue  # not mentioned: skipped, like None
        assignments[bc] = None if k < 0 else (int(k) if b % 4 == 0 else options[k])  # names and columns
    estimate = Demultiplexer.estimate_ambient(calls, genotypes, handler, assignments, keep_profile=True)
    assert isinstance(estimate, AmbientEstimate)
    want = restated.restate(v, cb, e, prob, B, restated.DEFAULT_GRID, d1, d2, restated.derived_ambient(v, v2snp, 0.01))
    got = dict(loglik=estimate.profile.values, best=estimate.best, ll_best=estimate.ll_best, ll_zero=estimate.ll_zero, ambient=estimate.ambient)
    restated.assert_same(got, want, 'end to end')
    fio.assert_bitwise(estimate.alphas, restated.DEFAULT_GRID)
    summary = estimate.summary()
    assert list(summary.index) == barcodes and list(summary.columns) == ['option', 'alpha', 'log_likelihood_ratio', 'at_grid_edge']
    assigned = d1 >= 0
    assert list(summary['option'][assigned]) == [options[k] for k in columns[assigned]] and summary['option'][~assigned].isna().all()
    assert np.array_equal(summary['alpha'].values[assigned], restated.DEFAULT_GRID[want['best'][assigned]].astype(np.float64))
    # a pandas Series, a grid of the caller's, a supplied profile, no profile kept; resident call sets in place of the containers
    series = summary['option'][assigned]
    grid = [0.5, 0.0, 0.2]
    resident_sets = {chromosome: ResidentCalls(c) for chromosome, c in calls.items()}
    try:
        lean = Demultiplexer.estimate_ambient(resident_sets, genotypes, handler, series, alphas=grid, ambient=want['ambient'])
    finally:
        for r_calls in resident_sets.values():
            r_calls.close()
    assert lean.profile is None
    want_lean = restated.restate(v, cb, e, prob, B, grid, d1, d2, want['ambient'])
    restated.assert_same(dict(best=lean.best, ll_best=lean.ll_best, ll_zero=lean.ll_zero, ambient=lean.ambient), want_lean, 'a Series, three values')
    with pytest.raises(ValueError, match='not an option'):
        Demultiplexer.estimate_ambient(calls, genotypes, handler, {barcodes[0]: 'nobody'})
    with pytest.raises(ValueError, match='not one of'):
        Demultiplexer.estimate_ambient(calls, genotypes, handler, {'no such barcode': donors[0]})


def test_known_contamination_is_recovered_on_the_device():
    from demuxalot_amd.device import DeviceContext
    sim, want = restated.simulated()
    with DeviceContext(0) as ctx:
        ctx.set_problem(sim['B'], len(sim['v2snp']), sim['prob'].shape[1], sim['v'], sim['cb'], sim['e'], sim['v2snp'])
        ctx.set_probs(sim['prob'])
        got = ctx.ambient_profile(sim['donor1'], sim['donor2'], restated.DEFAULT_GRID, ambient=sim['soup'])
    restated.assert_same(got, want, 'the simulation')
    medians = restated.recovery_condition(restated.DEFAULT_GRID, got['best'], sim['truth'])
    print('medians of the estimates at true fractions 0 / 0.2 / 0.4:', medians)
