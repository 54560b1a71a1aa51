"""Designed problems of tests/test_gpu_ambient_learning.py (learning under ambient fractions), built with numpy alone so
that the CPU can say what a problem exercises before the device is asked.  Nothing here knows the library."""
import functools

import numpy as np


def shape_problem(G, seed=0):
    """A small learning problem for the kernel-shape edges: dict(v, cb, e, v2snp, betas, raw_betas, B) with variant-major calls, plus
    'pools', 'pool_of', 'alpha', 'row_lengths'.  Barcode 0 has no calls, barcode 1 is in no pool; the rows of barcodes 2 .. 7 have 1, 8,
    9, 16, 65 and 513 calls (padded lengths 8, 8, 16, 16, 72 and 520: one group, two, one more than a multiple of 64 calls and of 64
    groups), the others 20 .. 40; the last SNP's variants have no calls; the last donor is in no pool when there are several."""
    rng = np.random.default_rng(seed)
    n_snps, B = 300, 40
    V = 2 * n_snps
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    lengths = np.concatenate([[0, 30, 1, 8, 9, 16, 65, 513], rng.integers(20, 41, size=B - 8)])
    vs, cbs = [], []
    for b, n in enumerate(lengths):
        vs.append(rng.choice(V - 2, size=n, replace=False))  # (both alleles of a SNP may be called)
        cbs.append(np.full(n, b))
    v, cb = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32)
    order = np.lexsort((cb, v))  # variant-major, as the pack leaves the calls
    v, cb = v[order], cb[order]
    e = rng.choice(np.array([0.001, 0.01, 0.05, 0.3], dtype=np.float32), size=len(v))
    betas = rng.uniform(0.5, 6.0, size=(V, G)).astype(np.float32)
    donors = list(range(G - 1)) if G > 1 else [0]
    pools = [donors, donors[:min(5, len(donors))]]
    pool_of = (np.arange(B) % 2).astype(np.int32)
    pool_of[1] = -1
    alpha = np.array([0.0, 0.1, 0.37, 0.63, 1.0], dtype=np.float32)[np.arange(B) % 5]
    assert not np.isin(v, [V - 2, V - 1]).any()
    return dict(v=v, cb=cb, e=e, v2snp=v2snp, betas=betas, raw_betas=betas, B=B, pools=pools, pool_of=pool_of, alpha=alpha,
                row_lengths=lengths)


# ---- variants of several work items, sums at a float32 rounding tie -------------------------------------------------------------
HOT, MARKERS, KEEP_ERROR = 32, 64, np.float32(2.0 ** -7)


@functools.lru_cache(maxsize=None)
def tie_problem():
    """Two donors, 3 000 barcodes, a genotype table set by hand (dmx_set_probs), fractions 0 and 0.5, a supplied soup.
      barcodes 0 .. 2899    donor 0: 64 marker calls that leave posterior exactly (1, 0); alpha 0.5 for the first 700, else 0
      barcodes 2900 .. 2995 donor 1, likewise, alpha 0.5 for every other one
      barcodes 2996 .. 2999 donor 1 through two calls whose table entries leave posterior(donor 0) near 4e-7: a contribution of
                            about 1.6e-13 to column 0 of every hot variant
      hot variant j < 32    table row (0.5, 0.5), soup 0.5, p_base_wrong 2^-7, called by every barcode but the first j: about 2 990
                            calls, three work items of 1 024.  A donor-0 barcode contributes (127/128)^2 at alpha 0 and (127/256)^2
                            at 0.5 (r = 0.5 exactly), so the exact part of the sum is (4 m1 + m2) 16129 / 2^16 with m2 = 700 - j: a
                            float32 tie for two of the sixteen residues.  In call order the four late contributions are each below
                            half an ulp of the running float64 sum (2.3e-13 above 2048) and are lost: the sum stays ON the tie and
                            rounds to even.  Inside the third item's partial sum (below 1024: half an ulp 5.7e-14) they are kept, and
                            their total moves the sum of the partials above the tie: it rounds up.
    Returns dict(v, cb, e, v2snp, prob, B, alpha, soup, pools, pool_of, hot) - variant-major calls, hot: the hot variants' ids."""
    B, G = 3000, 2
    n_major, n_minor, n_late = 2900, 96, 4
    late = np.arange(B - n_late, B)
    marker0 = np.arange(0, MARKERS)                # SNP s < 128: variants 2 s, 2 s + 1
    marker1 = np.arange(MARKERS, 2 * MARKERS)
    window = np.arange(2 * MARKERS, 2 * MARKERS + 2)
    hot = np.arange(2 * MARKERS + 2, 2 * MARKERS + 2 + HOT)
    n_snps = 2 * MARKERS + 2 + HOT
    V = 2 * n_snps
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    prob = np.full((V, G), 0.5, dtype=np.float32)
    prob[2 * marker0] = [0.99, 0.01]
    prob[2 * marker0 + 1] = [0.01, 0.99]
    prob[2 * marker1] = [0.01, 0.99]
    prob[2 * marker1 + 1] = [0.99, 0.01]
    prob[2 * window] = [np.float32(4.69e-4), 0.9]
    prob[2 * window + 1] = [np.float32(1 - 4.69e-4), 0.1]
    soup = np.full(V, 0.5, dtype=np.float32)
    alpha = np.zeros(B, dtype=np.float32)
    alpha[:700] = 0.5
    alpha[n_major:n_major + n_minor:2] = 0.5
    vs, cbs, es = [], [], []
    for b in range(B):
        mine = 2 * (window if b >= B - n_late else marker0 if b < n_major else marker1)
        called_hot = 2 * hot[np.arange(HOT) <= b] if b < HOT else 2 * hot  # hot variant j is skipped by the barcodes below j
        vs.append(np.concatenate([mine, called_hot]))
        es.append(np.concatenate([np.zeros(len(mine), np.float32), np.full(len(called_hot), KEEP_ERROR)]))
        cbs.append(np.full(len(mine) + len(called_hot), b))
    v, cb, e = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32), np.concatenate(es).astype(np.float32)
    order = np.lexsort((cb, v))
    return dict(v=v[order], cb=cb[order], e=e[order], v2snp=v2snp, prob=prob, B=B, alpha=alpha, soup=soup, pools=[[0, 1]],
                pool_of=np.zeros(B, dtype=np.int32), hot=2 * hot, late=late)
