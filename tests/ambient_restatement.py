"""Ambient RNA fractions (include/demux_hip_debug.h: dmx_ambient_profile; Demultiplexer.estimate_ambient) restated with numpy and the
oracle, used as the checker by tests/test_ambient_cpu.py and tests/test_gpu_ambient.py.

For barcode b with the assigned option (d1) or (d1, d2) and grid value alpha, all in float32, every operation rounded:
    q = prob[v, d1]   or   (prob[v, d1] + prob[v, d2]) * 0.5
    m = q * (1 - alpha) + ambient[v] * alpha
    L[b, alpha] = f32( sum over the calls of b, in their stored order, of f64( log(m * (1 - e) + max(e, 1e-4)) ) )
with oracle.log_f32 for the log and np.bincount(cb, weights=t) for the ordered float64 sum - the reference's own barcode_logits
(demux.py:246-265) with the mixture in place of the genotype's term.  The derived profile is the reference's P-step
(oracle.probs_from_betas) on the one-column table of call counts + 1.  Nothing here knows the library."""
import functools

import numpy as np

from oracle import demux_oracle
from tests import fixture_io as fio


def fixture_problem(name, clip=0.01):
    """(v, cb, e, prob, B, v2snp) of a golden fixture as predict_posteriors sees it (prior betas without the data term)."""
    fx = fio.load(name)
    prob = demux_oracle.probs_from_betas(fx['pack_v2snp'], fx['pack0_betas'], clip)
    return fx['pack_bc_variant_id'], fx['pack_bc_cb'], fx['pack_bc_p'], prob, len(fx['barcodes']), fx['pack_v2snp']


def derived_ambient(v, v2snp, clip):
    """float32[V]: per SNP the share of every variant among the barcode-level calls, one pseudo-count each, clipped to [clip, 1 - clip]."""
    count = np.bincount(v, minlength=len(v2snp))
    assert count.max(initial=0) < 2 ** 24, 'the counts are float32'
    betas = (count + 1).astype(np.float32)[:, None]
    return np.ascontiguousarray(demux_oracle.probs_from_betas(v2snp, betas, clip)[:, 0])


def first_maximum(L):
    """(best int32[B], value float32[B]): the first maximum of every row, NaN never wins; a row of NaNs gives -1 / NaN."""
    nan = np.isnan(L)
    first = np.where(nan, -np.inf, L).argmax(axis=1)
    some = ~nan.all(axis=1)
    return np.where(some, first, -1).astype(np.int32), np.where(some, L[np.arange(len(L)), first], np.nan).astype(np.float32)


def restate(v, cb, e, prob, B, alphas, donor1, donor2, ambient):
    """dict(loglik, best, ll_best, ll_zero, ambient) as dmx_ambient_profile defines them."""
    v, cb = np.asarray(v), np.asarray(cb)
    e = np.asarray(e, dtype=np.float32)
    prob = np.asarray(prob, dtype=np.float32)
    alphas = np.asarray(alphas, dtype=np.float32)
    ambient = np.asarray(ambient, dtype=np.float32)
    donor1, donor2 = np.asarray(donor1, dtype=np.int64), np.asarray(donor2, dtype=np.int64)
    assert donor1.shape == (B,) and donor2.shape == (B,) and ambient.shape == (prob.shape[0],)
    keep = 1 - e
    floor = e.clip(1e-4)
    assert keep.dtype == np.float32 and floor.dtype == np.float32
    L = np.full((B, len(alphas)), np.nan, dtype=np.float32)
    options = {(int(a), int(b)) for a, b in zip(donor1, donor2) if a >= 0}
    for d1, d2 in sorted(options):
        rows = np.flatnonzero((donor1 == d1) & (donor2 == d2))
        col = prob[:, d1] if d2 < 0 else (prob[:, d1] + prob[:, d2]) * np.float32(0.5)
        mine = np.isin(cb, rows)  # (boolean selection keeps the stored order)
        vs, cbs, ks, fs = v[mine], cb[mine], keep[mine], floor[mine]
        for j, alpha in enumerate(alphas):
            w0 = np.float32(1) - alpha
            m = col[vs] * w0 + ambient[vs] * alpha
            t = demux_oracle.log_f32(m * ks + fs)
            assert m.dtype == np.float32 and t.dtype == np.float32
            sums = np.bincount(cbs, weights=t, minlength=B)  # float64, in the order of the calls
            L[rows, j] = sums[rows].astype(np.float32)
    best, ll_best = first_maximum(L)
    zero = np.flatnonzero(alphas == 0)
    ll_zero = L[:, zero[0]].copy() if len(zero) else np.full(B, np.nan, dtype=np.float32)
    return dict(loglik=L, best=best, ll_best=ll_best, ll_zero=ll_zero, ambient=ambient)


def assert_same(got, want, what):
    """Everything bit for bit; NaN on both sides for skipped rows (and for ll_zero of a grid without 0)."""
    keys = ['best', 'll_best', 'll_zero', 'ambient'] + (['loglik'] if got.get('loglik') is not None else [])
    assert got['best'].dtype == np.int32 and np.array_equal(got['best'], want['best']), f'{what}: best'
    for key in keys[1:]:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == np.float32 and g.shape == w.shape, (what, key, g.dtype, g.shape, w.shape)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), f'{what}: {key}: NaN in other places'
        fio.assert_bitwise(g[~nan], w[~nan], f'{what}: {key}')


# ---- the seeded simulation of the recovery tests ------------------------------------------------------------------------------
def simulate(seed=0, n_donors=8, n_snps=600, n_barcodes=96, calls_per_barcode=256, true_alphas=(0.0, 0.2, 0.4), error=0.01):
    """A problem whose ambient fractions are known: biallelic SNPs (two variants each), genotypes from {0.01, 0.5, 0.99} for the
    alternative allele, every barcode a singlet of donor b % n_donors with contamination true_alphas[b % 3] from a soup that is the
    mean genotype; calls_per_barcode distinct SNPs per barcode, one observed allele each.
    Returns dict(v, cb, e, prob, B, v2snp, donor1, donor2, truth, soup)."""
    rng = np.random.default_rng(seed)
    alt = rng.choice(np.array([0.01, 0.5, 0.99], dtype=np.float32), size=(n_snps, n_donors))
    prob = np.empty((2 * n_snps, n_donors), dtype=np.float32)  # variant 2 s: the reference allele of SNP s, 2 s + 1: the alternative
    prob[0::2] = np.float32(1) - alt
    prob[1::2] = alt
    soup = prob.astype(np.float64).mean(axis=1).astype(np.float32)
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    donor = np.arange(n_barcodes) % n_donors
    truth = np.asarray(true_alphas, dtype=np.float64)[np.arange(n_barcodes) % len(true_alphas)]
    vs, cbs = [], []
    for b in range(n_barcodes):
        snps = np.sort(rng.choice(n_snps, size=calls_per_barcode, replace=False))
        p_alt = (1 - truth[b]) * prob[2 * snps + 1, donor[b]] + truth[b] * soup[2 * snps + 1]
        is_alt = rng.random(calls_per_barcode) < p_alt
        wrong = rng.random(calls_per_barcode) < error  # a sequencing error flips the allele
        vs.append(2 * snps + (is_alt ^ wrong))
        cbs.append(np.full(calls_per_barcode, b))
    v, cb = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32)
    order = np.lexsort((cb, v))  # variant-major, as the pack leaves the calls
    v, cb = v[order], cb[order]
    e = np.full(len(v), error, dtype=np.float32)
    return dict(v=v, cb=cb, e=e, prob=prob, B=n_barcodes, v2snp=v2snp, donor1=donor.astype(np.int32),
                donor2=np.full(n_barcodes, -1, dtype=np.int32), truth=truth, soup=soup)


DEFAULT_GRID = np.linspace(0, 0.63, 64, dtype=np.float32)  # what estimate_ambient takes for alphas=None


@functools.lru_cache(maxsize=None)
def simulated():
    """(the simulation, its restatement on the default grid with the true soup): computed once, shared by the CPU and the GPU tests."""
    sim = simulate()
    return sim, restate(sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B'], DEFAULT_GRID, sim['donor1'], sim['donor2'], sim['soup'])


def recovery_condition(alphas, best, truth):
    """The medians of the estimates per true fraction; asserts that each lies within 0.1 of its truth and that they are strictly ordered."""
    estimates = np.asarray(alphas, dtype=np.float64)[best]
    levels = np.unique(truth)
    medians = np.array([np.median(estimates[truth == level]) for level in levels])
    assert (np.abs(medians - levels) <= 0.1).all(), (levels, medians)
    assert (np.diff(medians) > 0).all(), medians
    return medians
