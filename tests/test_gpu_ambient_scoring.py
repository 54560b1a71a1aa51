"""Posteriors under per-barcode ambient fractions on the GPU (include/demux_hip_debug.h: dmx_estep_ambient; csrc/estep_ambient.hip;
Demultiplexer.predict_posteriors_with_ambient / predict_posteriors_decontaminated).

The pass has no tolerance arithmetic: everything is compared bit for bit.  The checkers are tests/ambient_scoring_restatement.py -
numpy and the oracle, pinned to the reference's own posteriors in tests/test_ambient_scoring_cpu.py - and the two passes the new one
is the intersection of: dmx_estep_pools at alpha = 0, dmx_ambient_profile for an option with penalty 0.  The shapes are the smallest
at which the kernels can go wrong: option counts on either side of every slot boundary, rows on either side of the 8-call padding and
of the prologue's 64-call chunk, pools of several buckets and barcodes in no pool in one call, barcodes without calls."""
import functools

import numpy as np
import pandas as pd
import pytest

from tests import ambient_restatement as profile_restated
from tests import ambient_scoring_restatement as restated
from tests import fixture_io as fio
from tests import pooled_helpers as helpers
from tests import pools_restatement
from tests.pooled_helpers import at, exact_mode, spread_columns  # noqa: F401 (exact_mode is a fixture)

pytestmark = pytest.mark.gpu

DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED = helpers.DMX_ERR_INVALID, helpers.DMX_ERR_UNSUPPORTED
F1, F2, SMALL = helpers.F1, helpers.F2, helpers.F3_SMALL[2]  # G = 20, 4, 5
FRACTIONS = np.array([0.0, 1.0, 0.01, 0.37, 0.63], dtype=np.float32)
KEYS = ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass')
resident = functools.lru_cache(maxsize=None)(helpers.new_resident)  # (ctx, v, cb, e, prob, B, v2snp), the contexts this module's own


def mixed_fractions(B):
    return FRACTIONS[np.arange(B) % len(FRACTIONS)]


def assert_same(got, want, what):
    pools_restatement.assert_same(got, want, what)
    if 'ambient' in want and 'ambient' in got:
        fio.assert_bitwise(got['ambient'], want['ambient'], f'{what}: ambient_out')


# ---- 1. I1: at alpha = 0 the pass is dmx_estep_pools --------------------------------------------------------------------------
@pytest.mark.parametrize('name', [F1, F2])
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_all_zero_fractions_are_the_pooled_estep(name, doublet_prior):
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    pools, pool_of = [list(range(G))], np.zeros(B, np.int32)
    penalty = np.array([restated.demux_oracle.doublet_penalties(G, doublet_prior)[-1]], np.float32)
    plain = ctx.estep_pools(pools, pool_of, doublet_prior != 0, penalty)
    other = np.random.default_rng(1).uniform(0, 1, size=len(v2snp)).astype(np.float32)
    for what, alpha, ambient in (('derived profile', np.zeros(B, np.float32), None), ('-0 and a supplied profile', np.full(B, -0.0, np.float32), other)):
        got = ctx.estep_ambient(pools, pool_of, doublet_prior != 0, penalty, alpha, ambient=ambient)
        for key in KEYS:
            assert got[key].dtype == plain[key].dtype and got[key].tobytes() == plain[key].tobytes(), f'{name} {doublet_prior} {what}: {key}'
    # ... and through it the reference's own posteriors
    reference = pools_restatement.Restatement(v, cb, e, prob, B, doublet_prior)
    pools_restatement.assert_same(plain, reference(pools, pool_of), f'{name} {doublet_prior}: the pooled pass')


# ---- 2. against the restatement: mixed fractions, supplied and derived profiles -------------------------------------------------
@pytest.mark.parametrize('name', [F1, SMALL])
def test_mixed_fractions_with_supplied_and_derived_profiles(name):
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    pools = [list(range(G)), [0, 2, 3], [1]]
    pool_of = np.where(np.arange(B) % 7 == 6, -1, np.arange(B) % 3).astype(np.int32)
    penalty = np.array([-0.75, 0.5, 0.0], dtype=np.float32)
    alpha = mixed_fractions(B)
    assert set(alpha[pool_of == 0]) == set(FRACTIONS), 'the wide pool sees every fraction'
    for clip in (0.01, 0.1):
        soup = profile_restated.derived_ambient(v, v2snp, clip)
        want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, alpha, soup)
        got = ctx.estep_ambient(pools, pool_of, True, penalty, alpha, clip)
        assert_same(got, want, f'{name}: derived profile, clip {clip}')
        fio.assert_bitwise(got['ambient'], ctx.ambient_profile(np.zeros(B, np.int32), np.full(B, -1, np.int32), [0.0], clip)['ambient'],
                           'ambient_out is dmx_ambient_profile\'s')
        back = ctx.estep_ambient(pools, pool_of, True, penalty, alpha, 0.45, ambient=got['ambient'])  # (the clip is the derived profile's alone)
        for key in KEYS + ('ambient',):
            assert back[key].tobytes() == got[key].tobytes(), f'{key}: the profile supplied back'
    other = np.random.default_rng(6).uniform(0, 1, size=len(v2snp)).astype(np.float32)
    other[:3] = [0.0, 1.0, 0.5]
    for with_doublets in (True, False):
        want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, with_doublets, alpha, other)
        assert_same(ctx.estep_ambient(pools, pool_of, with_doublets, penalty, alpha, ambient=other), want, f'{name}: another profile, doublets {with_doublets}')
    # the fraction of a barcode in no pool is not looked at
    wild = np.where(pool_of < 0, np.nan, alpha).astype(np.float32)
    full = ctx.estep_ambient(pools, pool_of, False, penalty, wild, ambient=other)
    assert_same(full, want, 'NaN fractions outside the pools')
    lean = ctx.estep_ambient(pools, pool_of, False, penalty, alpha, ambient=other, fetch_logits=False, fetch_probs=False)
    assert lean['logits'] is None and lean['probs'] is None
    for key in ('best_option', 'best_prob', 'doublet_mass'):
        assert lean[key].tobytes() == full[key].tobytes(), key


# ---- 3. kernel-shape edges ------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129]  # calls of a barcode: either side of the 8-call padding and of the 64-call chunk
SINGLET_WIDTHS = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024]  # options of a pool without doublets: either side of every slot boundary
DOUBLET_SIZES = [1, 2, 10, 11, 16, 22, 23, 31, 32, 44]  # donors: 1, 3, 55 | 66 | 136, 253 | 276, 496 | 528, 990 options


DESIGNED = dict(lengths=LENGTHS, V=160, B=12 * len(LENGTHS), seed=11)


@functools.lru_cache(maxsize=None)
def designed():
    """144 barcodes, barcode i with LENGTHS[i % 12] calls, on 1024 donors and 80 biallelic SNPs; error probabilities at both ends of
    their range among them.  Group i // 12 of the barcodes is what the tests put into one pool (or into none)."""
    return helpers.install_arrays(*helpers.designed_arrays(**DESIGNED))


def check_designed(pools, with_doublets, penalty, what):
    ctx, v, cb, e, prob, B, v2snp, soup, lengths = designed()
    group = np.arange(B) // len(LENGTHS)
    pool_of = np.where(group < len(pools), group, -1).astype(np.int32)
    assert (pool_of < 0).any(), 'barcodes in no pool'
    alpha = mixed_fractions(B)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, with_doublets, alpha, soup)
    got = ctx.estep_ambient(pools, pool_of, with_doublets, penalty, alpha, ambient=soup)
    assert_same(got, want, what)
    none = pool_of < 0
    assert (got['best_option'][none] == -1).all() and np.isnan(got['best_prob'][none]).all() and np.isnan(got['doublet_mass'][none]).all()
    # barcodes without calls: logits = penalties, posteriors = their softmax
    for b in np.flatnonzero((lengths == 0) & ~none):
        p = pool_of[b]
        row = slice(got['row_ptr'][b], got['row_ptr'][b + 1])
        pen = np.zeros(row.stop - row.start, np.float32)
        pen[len(pools[p]):] = penalty[p]
        fio.assert_bitwise(got['logits'][row], pen, f'{what}: barcode {b} without calls')
        fio.assert_bitwise(got['probs'][row], restated.demux_oracle.softmax_rows(pen[None, :])[0], f'{what}: barcode {b} without calls, posteriors')
    # derived profile on the same shapes (the padded rows of the prologue, a profile entry per table row)
    derived = profile_restated.derived_ambient(v, v2snp, 0.01)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, with_doublets, alpha, derived)
    assert_same(ctx.estep_ambient(pools, pool_of, with_doublets, penalty, alpha), want, f'{what}: derived profile')


def test_singlet_pools_on_either_side_of_every_slot_boundary():
    rng = np.random.default_rng(3)
    pools = [spread_columns(rng, K, 1024) for K in SINGLET_WIDTHS]
    assert pools[-1] == list(range(1024))
    check_designed(pools, False, np.linspace(-1, 1, len(pools)).astype(np.float32), 'singlet pools')


def test_doublet_pools_of_every_bucket():
    rng = np.random.default_rng(4)
    pools = [spread_columns(rng, g, 1024) for g in DOUBLET_SIZES]
    widths = [g * (g + 1) // 2 for g in DOUBLET_SIZES]
    assert widths == [1, 3, 55, 66, 136, 253, 276, 496, 528, 990]
    check_designed(pools, True, np.linspace(-2, 1.5, len(pools)).astype(np.float32), 'doublet pools')


# ---- 4. I2: an option with penalty 0 is dmx_ambient_profile's log-likelihood ----------------------------------------------------
@pytest.mark.parametrize('name', [F2, F1])
def test_options_with_penalty_zero_are_the_profile_log_likelihoods(name):
    ctx, v, cb, e, prob, B, v2snp = resident(name)
    G = prob.shape[1]
    alpha = mixed_fractions(B)
    column = np.arange(B) % len(FRACTIONS)
    got = ctx.estep_ambient([list(range(G))], np.zeros(B, np.int32), True, np.zeros(1, np.float32), alpha)
    logits = got['logits'].reshape(B, -1)
    d1, d2 = restated.pool_options(list(range(G)), True)
    K = len(d1)
    assert logits.shape == (B, K)
    rows = np.arange(B)
    for shift in range(0, K, 1 if K <= 16 else 11):  # every barcode with another option per call; (barcode, option) pairs all over the triangle
        k = (rows + shift) % K
        donor1, donor2 = d1[k].astype(np.int32), np.where(d1[k] == d2[k], -1, d2[k]).astype(np.int32)
        profile = ctx.ambient_profile(donor1, donor2, FRACTIONS)
        fio.assert_bitwise(np.ascontiguousarray(logits[rows, k]), np.ascontiguousarray(profile['loglik'][rows, column]), f'{name}: shift {shift}')
        fio.assert_bitwise(got['ambient'], profile['ambient'], 'the same derived profile')


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def raw_call(ctx, with_doublets, pool_start, donors, penalty, pool_of, row_ptr, alpha, ambient=None, n_pools=None, B=None, V=None):
    """dmx_estep_ambient with the arrays as given: (status, message, whether an output was written)."""
    from demuxalot_amd import _lib
    pool_start, donors = np.asarray(pool_start, np.int64), np.asarray(donors, np.int32)
    penalty, pool_of, row_ptr = np.asarray(penalty, np.float32), np.asarray(pool_of, np.int32), np.asarray(row_ptr, np.int64)
    alpha = None if alpha is None else np.asarray(alpha, np.float32)
    ambient = None if ambient is None else np.asarray(ambient, np.float32)
    B, V = ctx.B if B is None else B, ctx.V if V is None else V
    n = max(int(row_ptr.max(initial=0)), 0) + 1
    outputs = [np.full(n, 7, np.float32), np.full(n, 7, np.float32), np.full(B, 7, np.int32), np.full(B, 7, np.float32), np.full(B, 7, np.float64),
               np.full(V, 7, np.float32)]
    status = ctx._lib.dmx_estep_ambient(ctx._h, with_doublets, len(pool_start) - 1 if n_pools is None else n_pools, _lib.ptr(pool_start),
                                        _lib.ptr(donors), _lib.ptr(penalty), _lib.ptr(pool_of), _lib.ptr(row_ptr), *[_lib.ptr(o) for o in outputs[:5]],
                                        0.01, 0.99, _lib.ptr(alpha), _lib.ptr(ambient), _lib.ptr(outputs[5]))
    return status, _lib.load().dmx_last_error().decode(), any((o != 7).any() for o in outputs)


def test_refusals_return_their_code_and_write_nothing():
    ctx, v, cb, e, prob, B, v2snp = resident(SMALL)  # G = 5
    pools = [[0, 1], [1, 2, 4]]
    pool_of = np.where(np.arange(B) % 5 == 4, -1, np.arange(B) % 2).astype(np.int32)
    penalty = np.array([0.25, -0.5], np.float32)
    alpha = mixed_fractions(B)
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, alpha, soup)
    good = dict(with_doublets=1, pool_start=[0, 2, 5], donors=[0, 1, 1, 2, 4], penalty=penalty, pool_of=pool_of, row_ptr=want['row_ptr'], alpha=alpha)
    status, _text, written = raw_call(ctx, **good)
    assert status == 0 and written
    pooled, outside = int(np.flatnonzero(pool_of >= 0)[3]), int(np.flatnonzero(pool_of < 0)[0])
    short_rows = want['row_ptr'].copy()
    short_rows[-1] -= 1
    cases = helpers.pool_refusal_cases(good, pool_of) + [
        (dict(pool_start=[0, 3, 2], donors=[0, 1, 2, 4, 4]), DMX_ERR_INVALID, 'decreases'),
        (dict(donors=[0, 0, 1, 2, 4]), DMX_ERR_INVALID, 'ascending'),
        (dict(donors=[-1, 1, 1, 2, 4]), DMX_ERR_INVALID, 'outside'),
        (dict(pool_of=at(pool_of, 1, -2)), DMX_ERR_INVALID, 'pool_of_barcode'),
        (dict(row_ptr=short_rows), DMX_ERR_INVALID, 'row_ptr'),
        (dict(with_doublets=0), DMX_ERR_INVALID, 'row_ptr'),  # (the rows were laid out for the pairs)
        (dict(alpha=None), DMX_ERR_INVALID, 'null alpha'),
        (dict(alpha=at(alpha, pooled, np.nan)), DMX_ERR_INVALID, 'alpha of a barcode'),
        (dict(alpha=at(alpha, pooled, np.inf)), DMX_ERR_INVALID, 'alpha of a barcode'),
        (dict(alpha=at(alpha, pooled, 1.5)), DMX_ERR_INVALID, 'alpha of a barcode'),
        (dict(alpha=at(alpha, B - 2, -0.1)), DMX_ERR_INVALID, 'alpha of a barcode'),
        (dict(ambient=at(soup, 3, np.nan)), DMX_ERR_INVALID, 'ambient value'),
        (dict(ambient=at(soup, len(soup) - 1, 2.0)), DMX_ERR_INVALID, 'ambient value'),
        (dict(ambient=at(soup, 0, -0.5)), DMX_ERR_INVALID, 'ambient value'),
    ]
    assert pool_of[B - 2] >= 0
    launches = ctx.timings()['estep']['launches']
    for change, code, message in cases:
        status, text, written = raw_call(ctx, **{**good, **change})
        assert status == code and message in text and 'dmx_estep_ambient' in text, (change, status, text)
        assert not written, (change, 'a refused call writes nothing')
        assert ctx.timings()['estep']['launches'] == launches, 'a refused call launches nothing'
    status, _text, written = raw_call(ctx, **{**good, 'alpha': at(alpha, outside, np.nan)})
    assert status == 0 and written, 'the fraction of a barcode in no pool is not looked at'
    assert ctx.timings()['estep']['launches'] == launches + 1, 'the pass is counted as one E-step'
    from demuxalot_amd._lib import DemuxHipError
    with pytest.raises(DemuxHipError, match=r'alpha of a barcode.*status -1'):
        ctx.estep_ambient(pools, pool_of, True, penalty, at(alpha, pooled, 2.0))
    assert_same(ctx.estep_ambient(pools, pool_of, True, penalty, alpha), want, 'a valid call after the refused ones')


def test_more_than_1024_options_are_refused():
    ctx, *_rest, B, _v2snp, _soup, _lengths = designed()
    alpha = np.zeros(B, np.float32)
    # 45 donors with doublets: 1035 options (the table has 1024 columns: 1025 singlets are the CPU walk's)
    status, text, written = raw_call(ctx, 1, [0, 45], np.arange(45), [0.0], np.zeros(B, np.int32), np.arange(B + 1) * 1035, alpha)
    assert status == DMX_ERR_UNSUPPORTED and 'more than 1024 options' in text and not written, (status, text)
    status, _text, written = raw_call(ctx, 1, [0, 44], np.arange(44), [0.0], np.zeros(B, np.int32), np.arange(B + 1) * 990, alpha)
    assert status == 0 and written


def test_needs_a_problem_a_table_and_no_communicator():
    _v, _cb, _e, prob, B, _v2snp = profile_restated.fixture_problem('f3_small_0.npz')
    args = dict(with_doublets=1, pool_start=[0, 2], donors=[0, 1], penalty=[0.0], pool_of=np.zeros(B, np.int32), row_ptr=np.arange(B + 1) * 3,
                alpha=np.full(B, 0.25, np.float32), B=B, V=len(prob))
    helpers.check_needs_problem_table_no_communicator(raw_call, 'dmx_estep_ambient', args)


# ---- 6. the resident results of an E-step are none of this pass's business ------------------------------------------------------
def test_leaves_the_resident_results_alone():
    ctx, v, cb, e, prob, B, v2snp = resident(F1)
    G = prob.shape[1]
    penalties = restated.demux_oracle.doublet_penalties(G, 0.35)
    logits, probs = ctx.estep(penalties, True)
    pools, pool_of = [[0, 3, 5], list(range(G))], (np.arange(B) % 2).astype(np.int32)
    first = ctx.estep_ambient(pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), mixed_fractions(B))
    fio.assert_bitwise(ctx.get_probs(), probs, 'get_probs() after dmx_estep_ambient')
    fio.assert_bitwise(ctx.get_logits(), logits, 'get_logits() after dmx_estep_ambient')
    again = ctx.estep_ambient(pools, pool_of, True, np.array([0.5, penalties[-1]], np.float32), mixed_fractions(B))
    for key in KEYS + ('ambient',):
        assert first[key].tobytes() == again[key].tobytes(), f'{key}: two runs differ'


# ---- 7. the front door (exact_mode: predict_posteriors in the exact arithmetic, what the new passes are compared with) ------------
@pytest.mark.parametrize('doublet_prior', [0.35, 0.0])
def test_predict_posteriors_with_ambient_end_to_end(doublet_prior, exact_mode):
    from demuxalot_amd import Demultiplexer
    fx = fio.load(F1)
    calls, genotypes, handler = fio.product_inputs(fx)
    barcodes = handler.ordered_barcodes
    v, cb, e, prob, B, v2snp = profile_restated.fixture_problem(F1)
    assert B == len(barcodes)
    alpha = mixed_fractions(B)
    given = {}
    for b, bc in enumerate(barcodes):
        if b % 10 == 0:
            assert alpha[b] == 0
            if b % 20:
                given[bc] = None if b % 30 else float('nan')  # (or not mentioned at all)
        else:
            given[bc] = float(alpha[b]) if b % 2 else alpha[b]
    soup = profile_restated.derived_ambient(v, v2snp, 0.01)
    want_logits, want_probs, _ = restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, alpha, soup)
    plain_logits, plain_probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=doublet_prior)
    logits, probs = Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, pd.Series(given, dtype=object), doublet_prior=doublet_prior)
    for frame, plain, want in ((logits, plain_logits, want_logits), (probs, plain_probs, want_probs)):
        assert list(frame.columns) == list(plain.columns) and list(frame.index) == barcodes and frame.index.name == 'BARCODE'
        assert frame.values.dtype == np.float32 and list(frame.dtypes) == list(plain.dtypes)
        fio.assert_bitwise(frame.values, want, f'doublet_prior {doublet_prior}')
    assert (logits.values != plain_logits.values).any()
    # no fraction known: predict_posteriors itself
    for nothing in ({bc: float('nan') for bc in barcodes}, {}):
        same_logits, same_probs = Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, nothing, doublet_prior=doublet_prior)
        fio.assert_bitwise(same_logits.values, plain_logits.values, 'all-NaN fractions: logits')
        fio.assert_bitwise(same_probs.values, plain_probs.values, 'all-NaN fractions: posteriors')
    other = np.random.default_rng(8).uniform(0, 1, size=len(v2snp)).astype(np.float32)
    supplied, _probs = Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, given, ambient=other, doublet_prior=doublet_prior)
    fio.assert_bitwise(supplied.values, restated.restate_all_donors(v, cb, e, prob, B, doublet_prior, alpha, other)[0], 'a supplied profile')
    with pytest.raises(ValueError, match='outside'):
        Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, {barcodes[0]: 1.01})
    with pytest.raises(ValueError, match='not one of'):
        Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, {'no such barcode': 0.1})


def test_predict_posteriors_with_ambient_in_pools():
    from demuxalot_amd import Demultiplexer, PooledPosteriors
    name = 'f6_shipped_example.npz'
    fx = fio.load(name)
    calls, genotypes, handler = fio.product_inputs(fx)
    donors = [str(s) for s in fx['genotype_names']]
    barcodes = handler.ordered_barcodes
    B = len(barcodes)
    pool2donors = {'A': [donors[1], donors[0]], 'B': [donors[3], donors[1], donors[2]]}  # (any order)
    barcode2pool = {bc: (None if i % 5 == 4 else 'AB'[i % 2]) for i, bc in enumerate(barcodes)}
    alpha = mixed_fractions(B)
    pooled = Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, dict(zip(barcodes, alpha)), doublet_prior=0.35,
                                                           barcode2pool=barcode2pool, pool2donors=pool2donors)
    assert isinstance(pooled, PooledPosteriors) and pooled.pools == ['A', 'B']
    v, cb, e, prob, n, v2snp = profile_restated.fixture_problem(name)
    assert n == B
    pools = [[0, 1], [1, 2, 3]]
    pool_of = np.array([-1 if i % 5 == 4 else i % 2 for i in range(B)], np.int32)
    penalty = pools_restatement.Restatement(v, cb, e, prob, B, 0.35).pair_penalty(pools)
    want = restated.restate(v, cb, e, prob, B, pools, pool_of, penalty, True, alpha, profile_restated.derived_ambient(v, v2snp, 0.01))
    raw = dict(row_ptr=pooled.row_ptr, logits=pooled.logits, probs=pooled.probs, best_option=pooled.best_option, best_prob=pooled.best_prob,
               doublet_mass=pooled.doublet_mass)
    pools_restatement.assert_same(raw, want, 'pools end to end')
    logits_df, _probs_df = pooled.to_dataframes('B')
    assert list(logits_df.columns) == restated.demux_oracle.option_names([donors[g] for g in pools[1]], 0.35) and logits_df.index.name == 'BARCODE'
    with pytest.raises(AssertionError, match='come together'):
        Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, {}, barcode2pool=barcode2pool)


def test_too_many_donors_point_to_the_pools():
    from demuxalot_amd import BarcodeHandler, Demultiplexer, ProbabilisticGenotypes
    genotypes = ProbabilisticGenotypes([f'd{i:02d}' for i in range(45)])
    handler = BarcodeHandler(['AAAC-1', 'AAAG-1'])
    for entry, extra in ((Demultiplexer.predict_posteriors_with_ambient, ({},)), (Demultiplexer.predict_posteriors_decontaminated, ())):
        with pytest.raises(ValueError, match='1035 options.*barcode2pool / pool2donors'):
            entry({}, genotypes, handler, *extra)


def test_decontaminated_posteriors_on_the_simulation(exact_mode):
    from demuxalot_amd import AmbientEstimate, Demultiplexer
    sim, _ = profile_restated.simulated()  # (genotypes whose betas are the allele probabilities times 1000)
    calls, genotypes, handler = helpers.user_inputs(sim, helpers.table_betas(sim), default_prior=1.0)
    G, B = sim['prob'].shape[1], sim['B']
    barcodes = handler.ordered_barcodes
    donors = list(genotypes.genotype_names)
    plain_logits, plain_probs = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.35)
    logits, probs, estimate = Demultiplexer.predict_posteriors_decontaminated(calls, genotypes, handler, doublet_prior=0.35)
    assert isinstance(estimate, AmbientEstimate)
    for frame, plain in ((logits, plain_logits), (probs, plain_probs)):
        assert list(frame.columns) == list(plain.columns) and list(frame.index) == barcodes and frame.index.name == 'BARCODE'
        assert frame.values.dtype == np.float32 and frame.shape == (B, G * (G + 1) // 2)
    # the three conditions of the CPU test, on what the device computed (the pair posteriors added in float64 in ascending order)
    mass = lambda frame: np.cumsum(frame.values[:, G:].astype(np.float64), axis=1)[:, -1]
    restated.workflow_conditions(sim, mass(plain_probs), mass(probs), probs.values.argmax(axis=1))
    # pass 2 is estimate_ambient for the best singlet of the plain pass, pass 3 predict_posteriors_with_ambient with its fractions
    singlet = restated.best_singlets(plain_logits.values, G)
    alone = Demultiplexer.estimate_ambient(calls, genotypes, handler, {bc: donors[d] for bc, d in zip(barcodes, singlet)})
    for key in ('best', 'll_best', 'll_zero', 'ambient', 'alphas'):
        assert getattr(estimate, key).dtype == getattr(alone, key).dtype and getattr(estimate, key).tobytes() == getattr(alone, key).tobytes(), key
    assert list(estimate.summary()['option']) == [donors[d] for d in singlet]
    fractions = estimate.fractions()
    assert list(fractions.index) == barcodes and not fractions.isna().any()
    again_logits, again_probs = Demultiplexer.predict_posteriors_with_ambient(calls, genotypes, handler, fractions, ambient=estimate.ambient,
                                                                              doublet_prior=0.35)
    fio.assert_bitwise(logits.values, again_logits.values, 'pass 3: logits')
    fio.assert_bitwise(probs.values, again_probs.values, 'pass 3: posteriors')
    print('medians of the estimated fractions at true 0 / 0.2 / 0.4:', [float(np.median(fractions.values[sim['truth'] == t])) for t in (0.0, 0.2, 0.4)])
