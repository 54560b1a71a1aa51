"""The aggregate_on_snps E-step and the float64 M-step (csrc/snp_aggregate.hip) at every kernel form, on the designed problems of
tests/aggregate_problems.py (what they hold, which form every case runs and that no barcode is near a tie:
tests/test_aggregate_problems_cpu.py).

E-step: K alone picks the form - a wavefront per barcode with 1 / 2 / 4 / 8 / 16 options per lane up to 1024 options, a workgroup
per barcode with 6 / 9 / 12 / 17 / 24 / 33 options per thread beyond; every form runs on both sides of its boundary, singlets and
doublets, against oracle.barcode_logits_aggregated and a float64 softmax on the table the test set.  The gate is the project's own,
check64 of tests/test_gpu_aggregate.py: arg-max identical on every barcode, posteriors within 1e-12, logits within 1e-11.

M-step: G picks 1 / 2 / 4 / 8 / 16 columns per lane, column groups of 1024 beyond 1024 columns.  It is deterministic given its
input, so it is fed the device's own posteriors, as estep_snp returned them, and compared with the numpy restatement on bits."""
import time

import numpy as np
import pytest

from tests import aggregate_problems as ap
from tests import fixture_io as fio
from tests.test_gpu_aggregate import check64

pytestmark = pytest.mark.gpu

EMPTY = (0, ap.B - 1)  # the barcodes of shape_problem without molecule calls


@pytest.fixture(scope='module')
def ctx():
    from demuxalot_amd.device import DeviceContext
    t0 = time.perf_counter()
    with DeviceContext(0) as context:
        yield context
    print(f'tests/test_gpu_aggregate_shapes.py: {time.perf_counter() - t0:.1f} s between the first test that used the device and the last')


def install(ctx, p):
    G = p['prob'].shape[1]
    ctx.set_problem(p['B'], p['V'], G, p['v'], p['cb'], p['e'], p['v2snp'])
    ctx.set_probs(p['prob'])
    ctx.set_molecule_calls(p['mv'], p['mcb'], p['mp'])
    return G


def launches(ctx):
    return {phase: t['launches'] for phase, t in ctx.timings().items()}


def assert_empty_rows(logits, probs, rows, want_logits=None):
    """Barcodes without molecule calls: logits exactly +0 (or exactly the prior), posteriors exactly 1 / K without a prior."""
    K = logits.shape[1]
    for b in rows:
        if want_logits is None:
            fio.assert_bitwise(logits[b], np.zeros(K), f'logits of the empty barcode {b}')
            fio.assert_bitwise(probs[b], np.full(K, 1 / K), f'posteriors of the empty barcode {b}')
        else:
            fio.assert_bitwise(logits[b], want_logits[b], f'logits of the empty barcode {b}: the prior itself')


# ---- E-step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ap.ESTEP_CASES, ids=ap.case_id)
def test_estep_form_against_the_oracle(ctx, oracle, case):
    G, doublets, form = case
    p = ap.shape_problem(G)
    install(ctx, p)
    logits, probs = ctx.estep_snp(doublets, 0.5)
    want_logits, want_probs = ap.expected(oracle, p, doublets)
    assert logits.shape == want_logits.shape == (p['B'], ap.n_options(G, doublets))
    assert np.isfinite(logits).all() and np.isfinite(probs).all()
    ulps = check64(logits, probs, want_logits, want_probs, ap.case_id(case))
    assert_empty_rows(logits, probs, EMPTY)
    print(f'{ap.case_id(case)}: float64 logits within {ulps:.1f} ulp of the oracle, posteriors within {np.abs(probs - want_probs).max():.2g}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['prior32', 'prior64'])
@pytest.mark.parametrize('case', ap.PRIOR_CASES, ids=ap.case_id)
def test_estep_form_with_a_prior(ctx, oracle, case, dtype):
    """logits = oracle + prior (numpy's float64 `logits += prior`, a float32 prior promoted), posteriors their float64 softmax."""
    G, doublets, form = case
    p = ap.shape_problem(G)
    install(ctx, p)
    prior = ap.prior_logits(G, doublets, dtype)
    logits, probs = ctx.estep_snp(doublets, 0.5, prior_logits=prior)
    want_logits = ap.expected(oracle, p, doublets)[0] + prior
    assert want_logits.dtype == np.float64
    want_probs = ap.softmax64(want_logits)
    ulps = check64(logits, probs, want_logits, want_probs, f'{ap.case_id(case)} {dtype.__name__} prior')
    assert_empty_rows(logits, probs, EMPTY, want_logits=prior.astype(np.float64))
    print(f'{ap.case_id(case)} {dtype.__name__} prior: float64 logits within {ulps:.1f} ulp of the oracle')


def test_estep_without_any_molecule_call(ctx):
    p = ap.shape_problem(5)
    install(ctx, p)
    ctx.set_molecule_calls(p['mv'][:0], p['mcb'][:0], p['mp'][:0])
    logits, probs = ctx.estep_snp(True, 0.5)
    assert logits.shape == (p['B'], 15)
    assert_empty_rows(logits, probs, range(p['B']))


@pytest.mark.parametrize('case', [(16, True, 'wave4'), (129, False, 'wave4'), (45, True, 'block6')], ids=ap.case_id)
def test_estep_at_two_compensations(ctx, oracle, case):
    """count ** compensation is the caller's table: 0.5 and 1.0 on one context, each against the oracle at that compensation."""
    G, doublets, form = case
    assert ap.estep_form(ap.n_options(G, doublets)) == form
    p = ap.shape_problem(G)
    install(ctx, p)
    got = {}
    for compensation in (0.5, 1.0, 0.5):
        logits, probs = ctx.estep_snp(doublets, compensation)
        want_logits, want_probs = ap.expected(oracle, p, doublets, compensation)
        ulps = check64(logits, probs, want_logits, want_probs, f'{ap.case_id(case)} compensation {compensation}')
        print(f'{ap.case_id(case)} compensation {compensation}: float64 logits within {ulps:.1f} ulp of the oracle')
        if compensation in got:
            fio.assert_bitwise(logits, got[compensation], 'the same call again')
        got[compensation] = logits
    assert np.abs(got[0.5] - got[1.0]).max() > 1e-3  # (barcode 2's pair of 300 calls is divided by 17.3 or by 300)


# ---- M-step ----------------------------------------------------------------------------------------------------------------------
def check_mstep(ctx, p, G, post64, what):
    """mstep_f64 on the posteriors the device holds (post64, as estep_snp returned them) against the restatement.
    power 2: one float64 product and its square per term, one accumulator per (variant, column) in call order - the restatement's
    operations one for one, so every bit is compared, before and after the float32 rounding.
    power 1.5: the terms pow(x, 1.5) come from the device library's pow here and from numpy's there.  Both take the same x (one
    product, identical) and are taken to be within one ulp of the true power, so a term differs by at most 2 ulp, relatively
    2 * 2^-52.  The n terms of a variant are non-negative, so every partial sum is at most the total S: the two sums start
    at most 2 * 2^-52 S apart and each of the n - 1 additions on either side rounds by at most 2^-53 S, together
    (2 + (n - 1)) 2^-52 S = (n + 1) 2^-52 S; second-order terms fit into (n + 4) 2^-52 S, with n the longest variant's
    call count.  That is far below half a float32 ulp, so the one float32 rounding moves by at most one step: rtol 2^-23."""
    args = (p['v'], p['cb'], p['e'], post64, p['V'], G)
    n = int(np.bincount(p['v']).max())
    uncalled = np.bincount(p['v'], minlength=p['V']) == 0
    assert uncalled.any()
    for power in (2., 1.5, 2.):
        got, sums = ctx.mstep_f64(power), ctx.mstep_f64(power, as_float64=True)
        assert got.dtype == np.float32 and sums.dtype == np.float64 and got.shape == sums.shape == (p['V'], G)
        want, want_sums = ap.mstep_f64_restated(*args, power), ap.mstep_f64_restated(*args, power, as_float64=True)
        if power == 2.:
            fio.assert_bitwise(got, want, f'{what}: addition at power 2')
            fio.assert_bitwise(sums, want_sums, f'{what}: unrounded sums at power 2')
        else:
            off32 = np.abs(got.astype(np.float64) - want) / np.where(want > 0, want, 1)
            off64 = np.abs(sums - want_sums) / np.where(want_sums > 0, want_sums, 1)
            print(f'{what}: power 1.5: float32 additions within {off32.max() * 2 ** 23:.2f} x 2^-23, {int((got != want).sum())} of {got.size} '
                  f'differ; float64 sums within {off64.max() * 2 ** 52:.1f} x 2^-52 (allowed {n + 4})')
            assert np.allclose(got, want, rtol=2.0 ** -23, atol=0), f'{what}: addition at power 1.5'
            assert (np.abs(sums - want_sums) <= (n + 4) * 2.0 ** -52 * want_sums).all(), f'{what}: unrounded sums at power 1.5'
        fio.assert_bitwise(got[uncalled], np.zeros((int(uncalled.sum()), G), dtype=np.float32), f'{what}: variants without calls')
        fio.assert_bitwise(sums[uncalled], np.zeros((int(uncalled.sum()), G)), f'{what}: variants without calls, float64')
        assert (want_sums[~uncalled] > 0).all()  # so that a column nobody wrote cannot pass for a sum
    return got


@pytest.mark.parametrize('case', ap.MSTEP_CASES, ids=ap.case_id)
def test_mstep_form_on_the_device_s_own_posteriors(ctx, case):
    G, doublets, form = case
    p = ap.shape_problem(G)
    install(ctx, p)
    _, post64 = ctx.estep_snp(doublets, 0.5)
    assert post64.shape[1] == ap.n_options(G, doublets)  # the row stride of the posteriors; the M-step reads the first G columns
    got = check_mstep(ctx, p, G, post64, ap.case_id(case))
    if G > 1024:
        assert (got[:, 1024:] > 0).any(axis=1).sum() == (np.bincount(p['v'], minlength=p['V']) > 0).sum()


def test_mstep_on_a_variant_of_several_work_items(ctx):
    """item_problem: 2 150 calls of one variant in three work items, walked in order by one wavefront per 64 A columns."""
    p = ap.item_problem()
    G = install(ctx, p)
    _, post64 = ctx.estep_snp(False, 0.5)
    got = check_mstep(ctx, p, G, post64, 'item problem')
    assert (got[p['hot']] > 0).all() and (got[p['uncalled']] == 0).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refused(ctx, call, status, match):
    """`call` raises with `status`, launches nothing that the context counts, and leaves the context's results as they were."""
    from demuxalot_amd._lib import DemuxHipError
    before = launches(ctx)
    with pytest.raises(DemuxHipError, match=match) as err:
        call()
    assert f'(status {status})' in str(err.value), err.value
    assert launches(ctx) == before


INVALID, UNSUPPORTED = -1, -5


@pytest.mark.parametrize('G, doublets', ap.REFUSED_CASES, ids=['G129-doublets', 'G8257-singlets'])
def test_more_options_than_the_estep_takes_are_refused(ctx, G, doublets):
    """One genotype more than the widest table: refused before anything is launched, and a valid problem afterwards is untouched."""
    small = ap.shape_problem(23)
    install(ctx, small)
    logits, probs = ctx.estep_snp(True, 0.5)
    addition = ctx.mstep_f64(2.)
    # the refused problem: the calls of the small one, a table of ones that is never read
    ctx.set_problem(small['B'], small['V'], G, small['v'], small['cb'], small['e'], small['v2snp'])
    ctx.set_probs(np.ones((small['V'], G), dtype=np.float32))
    ctx.set_molecule_calls(small['mv'], small['mcb'], small['mp'])
    refused(ctx, lambda: ctx.estep_snp(doublets, 0.5), UNSUPPORTED, 'options')
    refused(ctx, lambda: ctx.mstep_f64(2.), INVALID, 'call order')  # nothing was computed for this problem
    install(ctx, small)
    again = ctx.estep_snp(True, 0.5)
    fio.assert_bitwise(again[0], logits, 'logits after a refusal')
    fio.assert_bitwise(again[1], probs, 'posteriors after a refusal')
    fio.assert_bitwise(ctx.mstep_f64(2.), addition, 'addition after a refusal')


def test_bad_arguments_are_refused_and_change_nothing(ctx):
    import ctypes
    from demuxalot_amd._lib import check, ptr
    p = ap.shape_problem(23)
    install(ctx, p)
    K = ap.n_options(23, True)
    logits, probs = ctx.estep_snp(True, 0.5)
    addition = ctx.mstep_f64(2.)
    count_pow = np.ascontiguousarray(np.arange(ap.LONG_COUNT + 1, dtype=np.int64) ** 0.5)
    prior = np.zeros((p['B'], K), dtype=np.float32)
    out_logits, out_probs = np.full((p['B'], K), np.nan), np.full((p['B'], K), np.nan)

    def estep(n_count_pow, prior_dtype):
        check(ctx._lib.dmx_estep_snp(ctx._h, 1, ptr(count_pow), n_count_pow, ptr(prior), prior_dtype, ptr(out_logits), ptr(out_probs)))

    n = ctypes.c_int64(0)
    check(ctx._lib.dmx_get_max_pair_count(ctx._h, ctypes.byref(n)))
    assert n.value == ap.LONG_COUNT
    refused(ctx, lambda: estep(ap.LONG_COUNT, 0), INVALID, 'count_pow')  # one entry short: counts 0 .. 299
    refused(ctx, lambda: estep(ap.LONG_COUNT + 1, 7), INVALID, 'prior_dtype')
    assert np.isnan(out_logits).all() and np.isnan(out_probs).all()
    for power in (0., -1., np.inf, np.nan):
        refused(ctx, lambda: ctx.mstep_f64(power), INVALID, 'power')
        refused(ctx, lambda: ctx.mstep_f64(power, as_float64=True), INVALID, 'power')
    fio.assert_bitwise(ctx.mstep_f64(2.), addition, 'addition after the refusals')
    estep(ap.LONG_COUNT + 1, 0)  # the same arguments, valid: a float32 prior of zeros
    fio.assert_bitwise(out_logits, logits, 'logits after the refusals')
    fio.assert_bitwise(out_probs, probs, 'posteriors after the refusals')


def test_mstep_f64_before_estep_snp_is_refused():
    from demuxalot_amd.device import DeviceContext
    p = ap.shape_problem(23)
    with DeviceContext(0) as ctx:
        install(ctx, p)
        refused(ctx, lambda: ctx.mstep_f64(2.), INVALID, 'call order')
        refused(ctx, lambda: ctx.mstep_f64(2., as_float64=True), INVALID, 'call order')
        _, post64 = ctx.estep_snp(False, 0.5)
        fio.assert_bitwise(ctx.mstep_f64(2.), ap.mstep_f64_restated(p['v'], p['cb'], p['e'], post64, p['V'], 23, 2.), 'addition after the refusals')
