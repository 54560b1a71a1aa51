"""The pooled E-step with every pair option summed over a grid of mixing shares (include/demux_hip_debug.h: dmx_estep_pair_shares;
Demultiplexer.predict_posteriors_with_doublet_shares) restated with numpy and the oracle, used as the checker by
tests/test_pair_shares_cpu.py and tests/test_gpu_pair_shares.py.  Nothing here knows the library.

S[b, k, j], the float64 sum of an option's log terms at grid point j, comes from np.bincount in call order, with
    q = prob[v, d1] * shares[j] + prob[v, d2] * (1 - shares[j])        float32, two products, one sum
for a pair and q = prob[v, d] for a singlet.  Across the grid a pair goes through tests/ambient_marginal_restatement.over_the_grid - the
recurrence of DESIGN.md 4.10 - with the shares where it has the fractions.  A singlet's logit is tests/pools_restatement's (the oracle's
barcode_logits on the pool's columns), its share_index -1 and its share_mean NaN.  The softmax goes through oracle.softmax_rows.

The second half is the seeded simulation of doublets of unequal shares and what is counted on it."""
import functools

import numpy as np

from oracle import demux_oracle
from tests import ambient_marginal_restatement as marginal
from tests import ambient_scoring_restatement as scoring
from tests import pools_restatement

over_the_grid = marginal.over_the_grid
log32 = marginal.log32
same_bits = marginal.same_bits
DEFAULT_SHARES = (np.arange(1, 10, dtype=np.float64) / 10).astype(np.float32)


def uniform_log_weights(n):
    """What the Python front door passes unless told otherwise."""
    return np.full(n, np.float32(-np.log(n)), dtype=np.float32)


def float64_sums(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, shares):
    """(row_ptr int64[B + 1], S float64[row_ptr[B], n_shares], pen float64[row_ptr[B]], single bool[row_ptr[B]]): per option and grid
    point the float64 sum of f64(log(q keep + floor)) over the barcode's calls in stored order (a singlet: the same sum at every grid
    point), the option's penalty, and whether it is a singlet."""
    v, cb = np.asarray(v), np.asarray(cb)
    e = np.asarray(e, dtype=np.float32)
    prob = np.asarray(prob, dtype=np.float32)
    shares = np.asarray(shares, dtype=np.float32)
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int64)
    pair_penalty = np.asarray(pair_penalty, dtype=np.float32)
    keep = 1 - e
    floor = e.clip(1e-4)
    assert keep.dtype == np.float32 and floor.dtype == np.float32
    widths = np.array([len(d) * (len(d) + 1) // 2 if with_doublets else len(d) for d in pools] + [0], dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(widths[pool_of_barcode])]).astype(np.int64)
    n = int(row_ptr[-1])
    S = np.full((n, len(shares)), np.nan, dtype=np.float64)
    pen = np.zeros(n, dtype=np.float64)
    single = np.zeros(n, dtype=bool)
    one = np.float32(1)
    for p, donors in enumerate(pools):
        rows = np.flatnonzero(pool_of_barcode == p)
        if not len(rows):
            continue
        mine = np.isin(cb, rows)  # (boolean selection keeps the stored order)
        vs, cbs, ks, fs = v[mine], cb[mine], keep[mine], floor[mine]
        d1, d2 = scoring.pool_options(donors, with_doublets)
        for k, (a, b) in enumerate(zip(d1, d2)):
            at = row_ptr[rows] + k
            single[at] = a == b
            pen[at] = np.float64(0 if a == b else pair_penalty[p])
            p1, p2 = prob[vs, a], prob[vs, b]
            for j, w in enumerate(shares):
                q = p1 if a == b else p1 * w + p2 * (one - w)
                t = demux_oracle.log_f32(q * ks + fs)
                assert q.dtype == np.float32 and t.dtype == np.float32
                S[at, j] = np.bincount(cbs, weights=t, minlength=B)[rows]  # float64, in the order of the calls
                if a == b:
                    S[at, :] = S[at, j][:, None]
                    break
    return row_ptr, S, pen, single


def restate(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, shares, log_weights=None):
    """dict(row_ptr, logits, probs, best_option, best_prob, doublet_mass, share_index, share_mean, best_share_index, best_share_mean,
    S, pen, single) as dmx_estep_pair_shares defines them."""
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int64)
    shares = np.asarray(shares, dtype=np.float32)
    row_ptr, S, pen, single = float64_sums(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, shares)
    n = len(pen)
    logits = np.full(n, np.nan, dtype=np.float32)
    share_index = np.full(n, -1, dtype=np.int32)
    share_mean = np.full(n, np.nan, dtype=np.float32)
    pairs = np.flatnonzero(~single)
    if len(pairs):
        logits[pairs], share_index[pairs], share_mean[pairs], _lam = over_the_grid(S[pairs], pen[pairs], shares, log_weights)
    singlets = pools_restatement.Restatement(v, cb, e, prob, B, 0)  # (a singlet's logit knows no penalty: the lists without pairs)
    probs = np.empty_like(logits)
    best_option = np.full(B, -1, dtype=np.int32)
    best_prob = np.full(B, np.nan, dtype=np.float32)
    doublet_mass = np.full(B, np.nan, dtype=np.float64)
    for p, donors in enumerate(pools):
        rows = np.flatnonzero(pool_of_barcode == p)
        if not len(rows):
            continue
        g = len(donors)
        K = g * (g + 1) // 2 if with_doublets else g
        first = row_ptr[rows][:, None]
        logits[(first + np.arange(g, dtype=np.int64)[None, :]).reshape(-1)] = singlets.pool_rows(donors)[0][rows].reshape(-1)
        take = (first + np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
        P = demux_oracle.softmax_rows(logits[take].reshape(len(rows), K))
        probs[take] = P.reshape(-1)
        masked = np.where(np.isnan(P), -np.inf, P)  # the first maximum; NaN never wins
        top = masked.argmax(axis=1)
        some = ~np.isnan(P).all(axis=1)
        best_option[rows] = np.where(some, top, -1)
        best_prob[rows] = np.where(some, P[np.arange(len(rows)), top], np.nan)
        mass = P[:, g:].astype(np.float64)  # added one after the other in ascending option order (cumsum is sequential)
        doublet_mass[rows] = np.cumsum(mass, axis=1)[:, -1] if mass.shape[1] else 0.0
    found = best_option >= 0
    best_share_index = np.full(B, -1, dtype=np.int32)
    best_share_index[found] = share_index[row_ptr[:-1][found] + best_option[found]]
    best_share_mean = np.full(B, np.nan, dtype=np.float32)
    best_share_mean[found] = share_mean[row_ptr[:-1][found] + best_option[found]]
    return dict(row_ptr=row_ptr, logits=logits, probs=probs, best_option=best_option, best_prob=best_prob, doublet_mass=doublet_mass,
                share_index=share_index, share_mean=share_mean, best_share_index=best_share_index, best_share_mean=best_share_mean,
                S=S, pen=pen, single=single)


def restate_all_donors(v, cb, e, prob, B, doublet_prior, shares, log_weights=None):
    """(logits, probs) [B, K] as predict_posteriors_with_doublet_shares returns them without pools (log_weights as given: None is
    all 0, not the front door's uniform prior), and the dict."""
    G = prob.shape[1]
    penalty = demux_oracle.doublet_penalties(G, doublet_prior)[-1] if G > 1 else 0.0
    out = restate(v, cb, e, prob, B, [list(range(G))], np.zeros(B, dtype=np.int32), np.array([penalty], dtype=np.float32), doublet_prior != 0,
                  shares, log_weights)
    return out['logits'].reshape(B, -1), out['probs'].reshape(B, -1), out


DESIGNED_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 40, 5]  # calls of a barcode: none, either side of the 8-call padding


@functools.lru_cache(maxsize=None)
def designed_problem():
    """(v, cb, e, prob, B, lengths, v2snp): 48 barcodes, barcode i with DESIGNED_LENGTHS[i % 12] calls (barcode 0 has none), on 1024
    donors and 24 biallelic SNPs (48 variants); error probabilities at both ends of their range and table entries of exactly 0 and 1
    among them.  The problem of tests/test_gpu_pair_shares.py's designed tests, without a device."""
    rng = np.random.default_rng(29)
    V, G, B = 48, 1024, 48
    lengths = [DESIGNED_LENGTHS[i % len(DESIGNED_LENGTHS)] for i in range(B)]
    v2snp = np.repeat(np.arange(V // 2, dtype=np.int32), 2)
    v = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lengths]).astype(np.int32)
    cb = np.repeat(np.arange(B), lengths).astype(np.int32)
    e = rng.choice(np.array([0.0, 1e-5, 1e-4, 0.01, 0.3, 1.0], dtype=np.float32), size=len(v))
    order = np.lexsort((cb, v))
    v, cb, e = v[order], cb[order], e[order]
    prob = rng.uniform(0.01, 0.99, size=(V, G)).astype(np.float32)
    prob[rng.random(size=prob.shape) < 0.05] = 0.0  # entries of exactly 0 ...
    prob[rng.random(size=prob.shape) < 0.02] = 1.0  # ... and of exactly 1
    prob[0, :3] = [0.0, 1.0, 0.5]                   # (row 0 is what the padding calls point at)
    assert np.bincount(cb, minlength=B).tolist() == lengths and lengths[0] == 0
    return v, cb, e, prob, B, np.asarray(lengths), v2snp


def half_shares_against_no_ambient(sizes, n, seed=12):
    """The two grid-summed passes where they are one computation: n shares of 0.5 against n ambient fractions of 0,
    under the same steep, unsorted log weights, on designed pools of `sizes` donors with doublets (the first pool's pair penalty -inf).
    p1 0.5 + p2 0.5 and (p1 + p2) 0.5 round alike for normal float32 and q 1 + a 0 is q, so every grid point has the same lambda and
    the two folds see the same t.  (pools, pool_of, penalty, shares, alphas, ambient, log_weights)."""
    v, cb, e, prob, B, _lengths, _v2snp = designed_problem()
    rng = np.random.default_rng(seed)
    pools = [sorted(int(d) for d in rng.choice(prob.shape[1], size=g, replace=False)) for g in sizes]
    pool_of = (np.arange(B) % (len(pools) + 1)).astype(np.int32)
    pool_of[pool_of == len(pools)] = -1
    penalty = np.linspace(-2, 1.5, len(pools)).astype(np.float32)
    penalty[0] = -np.inf
    weights = rng.uniform(-30, 2, size=n).astype(np.float32)
    weights[n // 2] = -60.0
    ambient = rng.uniform(0, 1, size=prob.shape[0]).astype(np.float32)
    return pools, pool_of, penalty, np.full(n, 0.5, np.float32), np.zeros(n, np.float32), ambient, weights


SHARED = ('row_ptr', 'logits', 'probs', 'best_option', 'best_prob', 'doublet_mass')
OWN = ('share_index', 'share_mean', 'best_share_index', 'best_share_mean')


def assert_same(got, want, what, keys=SHARED + OWN):
    """Everything dmx_estep_pair_shares returns, bit for bit (NaN payloads aside: a NaN is a NaN); `got` may lack the compact outputs
    that were not fetched."""
    for key in keys:
        if got.get(key) is None:
            continue
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {key}: {g.dtype}{g.shape} against {w.dtype}{w.shape}'
        if g.dtype.kind == 'f':
            assert np.array_equal(np.isnan(g), np.isnan(w)), f'{what}: {key}: NaN in other places'
            keep = ~np.isnan(w)
            same_bits(g[keep], w[keep], f'{what}: {key}')
        else:
            assert np.array_equal(g, w), f'{what}: {key}'


# ---- the seeded simulation of doublets of unequal shares ------------------------------------------------------------------------------
def simulate(share, calls_per_barcode, seed, n_donors=8, n_snps=600, n_singlets=96, n_doublets=48, error=0.01):
    """DESIGN.md 4.8's world without soup: 8 donors, 600 biallelic SNPs with the alternative-allele probability from {0.01, 0.5, 0.99};
    96 singlets (donor b % 8) and 48 doublets whose first donor is b % 8 and whose second is a random other donor, the first holding
    `share` of the droplet; distinct SNPs per barcode, one allele each, flipped with probability `error`."""
    rng = np.random.default_rng(seed)
    alt = rng.choice(np.array([0.01, 0.5, 0.99], dtype=np.float32), size=(n_snps, n_donors))
    prob = np.empty((2 * n_snps, n_donors), dtype=np.float32)
    prob[0::2] = np.float32(1) - alt
    prob[1::2] = alt
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    B = n_singlets + n_doublets
    first = np.arange(B) % n_donors
    second = np.full(B, -1)
    for b in range(n_singlets, B):
        second[b] = (first[b] + 1 + rng.integers(n_donors - 1)) % n_donors
    vs, cbs = [], []
    for b in range(B):
        snps = np.sort(rng.choice(n_snps, size=calls_per_barcode, replace=False))
        p_alt = prob[2 * snps + 1, first[b]].astype(np.float64)
        if second[b] >= 0:
            p_alt = share * p_alt + (1 - share) * prob[2 * snps + 1, second[b]]
        is_alt = rng.random(calls_per_barcode) < p_alt
        wrong = rng.random(calls_per_barcode) < error
        vs.append(2 * snps + (is_alt ^ wrong))
        cbs.append(np.full(calls_per_barcode, b))
    v, cb = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32)
    order = np.lexsort((cb, v))
    v, cb = v[order], cb[order]
    d1, d2 = scoring.pool_options(list(range(n_donors)), True)
    lo, hi = np.minimum(first, second), np.maximum(first, second)
    truth = np.array([int(np.flatnonzero((d1 == a) & (d2 == b))[0]) if a >= 0 else int(b) for a, b in zip(lo, hi)])
    return dict(v=v, cb=cb, e=np.full(len(v), error, dtype=np.float32), prob=prob, B=B, v2snp=v2snp, first=first, second=second,
                true_option=truth, share=share)


def counts_of(sim, doublet_mass, best_option):
    """dict(found, false): true doublets with pair mass above 0.5 whose best option is the right pair, of 48; singlets with pair mass
    above 0.5, of 96."""
    doublet_mass, best_option = np.asarray(doublet_mass), np.asarray(best_option)
    singlet = sim['second'] < 0
    called = doublet_mass > 0.5
    return dict(found=int((called & ~singlet & (best_option == sim['true_option'])).sum()), false=int((called & singlet).sum()))


@functools.lru_cache(maxsize=None)
def simulated(share, calls_per_barcode, seed, doublet_prior=0.35):
    """(sim, counts of the fixed 50 / 50 pass, counts of the marginal over DEFAULT_SHARES under the uniform prior, the marginal's
    dict), restated.  Computed once per shape, shared."""
    sim = simulate(share, calls_per_barcode, seed)
    G = sim['prob'].shape[1]
    fixed = pools_restatement.Restatement(sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B'], doublet_prior)([list(range(G))],
                                                                                                            np.zeros(sim['B'], np.int32))
    _l, _p, out = restate_all_donors(sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B'], doublet_prior, DEFAULT_SHARES,
                                     uniform_log_weights(len(DEFAULT_SHARES)))
    return sim, counts_of(sim, fixed['doublet_mass'], fixed['best_option']), counts_of(sim, out['doublet_mass'], out['best_option']), out


def value_conditions(share, fixed, grid):
    """The conditions at seed 0, 128 calls per barcode, doublet_prior 0.35, against the fixed pass of the same run.
    Share 0.8: at least 5 more of the 48 true doublets found, at most 6 of 96 singlets called doublets.  Share 0.5: no more than 3
    fewer found, at most 6 of 96 singlets called doublets."""
    print(f'share {share}: fixed {fixed}, grid {grid}')
    if share == 0.8:
        assert grid['found'] >= fixed['found'] + 5, (fixed, grid)
    elif share == 0.5:
        assert grid['found'] >= fixed['found'] - 3, (fixed, grid)
    else:
        raise AssertionError('no conditions for this share')
    assert grid['false'] <= 6, (fixed, grid)
