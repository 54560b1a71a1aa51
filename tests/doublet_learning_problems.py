"""Designed problems of tests/test_gpu_doublet_learning.py (learning from doublet posteriors), built with numpy alone so
that the CPU can say what a problem exercises before the device is asked.  Nothing here knows the library."""
import functools

import numpy as np

from tests import ambient_learning_problems


def shape_problem(G, seed=0):
    """tests/ambient_learning_problems.shape_problem's calls - barcode 0 has none, the rows of barcodes 2 .. 7 have 1, 8, 9, 16, 65 and
    513 calls, the last SNP's variants have no calls - with pools for doublets: dict(v, cb, e, v2snp, betas, raw_betas, B, pools,
    pool_of, row_lengths).
      pool 0   wide: the last 14 columns and the 22 columns below column 70 (or below G), so that with G = 130 its donors straddle
               the columns 63 | 64 and 127 | 128 and its 630 pair options take ten trips of 64 - at most 36 donors, 666 options
      pool 1   the first columns 0, 2, 3, 4
      pool 2   (G >= 13) twelve donors spread over all columns: 66 pair options, and the one-call barcode 2 is in it - with one call
               every pair's posterior is far above 1e-6, so its list takes two trips of 64 entries
    Column 1 is in no pool when G > 2; barcode 1 is in no pool."""
    problem = ambient_learning_problems.shape_problem(G, seed)
    B = problem['B']
    out_of_pools = {1} if G > 2 else set()
    wide = sorted((set(range(max(0, G - 14), G)) | set(range(max(0, min(G, 70) - 22), min(G, 70)))) - out_of_pools)
    pools = [wide, sorted(set(range(min(5, G))) - out_of_pools)]
    pool_of = (np.arange(B) % 2).astype(np.int32)
    if G >= 13:
        spread = sorted({int(x) for x in np.linspace(0, G - 1, 12)} - out_of_pools)
        assert len(spread) == 12
        pools.append(spread)
        pool_of[2::7] = 2
    pool_of[1] = -1
    assert all(len(p) * (len(p) + 1) // 2 <= 1024 for p in pools)
    problem.pop('alpha')
    return dict(problem, pools=pools, pool_of=pool_of)


# ---- pair posteriors of exactly 1; variants of several work items, sums at a float32 rounding tie -------------------------------
HOT, MARKERS, KEEP_ERROR = ambient_learning_problems.HOT, ambient_learning_problems.MARKERS, ambient_learning_problems.KEEP_ERROR
WINDOW = np.float32(5.4e-4)  # the late barcodes' table entry for donor 0: their posterior(donor 0) is 3.98e-7 beside the pair option


@functools.lru_cache(maxsize=None)
def tie_problem():
    """tests/ambient_learning_problems.tie_problem with doublets in the place of its contaminated droplets: two donors, one pool, 3 000
    barcodes, a genotype table set by hand (dmx_set_probs), scored with the pair option 0+1.
      barcodes 0 .. 699     doublets: the 64 marker calls of donor 0 AND the 64 of donor 1.  Either singlet explains half of them with
                            0.01 each, the pair every one with 0.5: the singlet posteriors underflow to 0 - the bitmap row is empty - and
                            the pair's is exactly 1
      barcodes 700 .. 2899  donor 0: 64 marker calls that leave the singlet posterior exactly 1 and the pair's near 1e-19
      barcodes 2900 .. 2995 donor 1, likewise
      barcodes 2996 .. 2999 donor 1 through two calls whose table entries leave posterior(donor 0) near 4e-7 and the pair's near 0.2:
                            at the test's threshold of 0.5 the pair is not credited, and the barcode contributes about 1.6e-13 to
                            column 0 of every hot variant
      hot variant j < 32    table row (0.5, 0.5), p_base_wrong 2^-7, called by every barcode but the first j: three work items of
                            1 024.  A donor-0 barcode contributes (127/128)^2; a doublet r = 0.5 exactly, credit 0 + 1 * 0.5, and
                            (127/256)^2 - the numbers of the ambient problem, so its float32 ties stand: in call order the four late
                            contributions are lost and the sum rounds to even, inside the third item's partial sum they are kept
                            and the sum of the partials rounds up.
    Returns dict(v, cb, e, v2snp, prob, B, pools, pool_of, hot, doublets, late) - variant-major calls."""
    B, G = 3000, 2
    n_doublets, n_major, n_late = 700, 2900, 4
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
    prob[2 * window] = [WINDOW, 0.9]
    prob[2 * window + 1] = [np.float32(1) - WINDOW, 0.1]
    vs, cbs, es = [], [], []
    for b in range(B):
        if b >= B - n_late:
            mine = 2 * window
        elif b < n_doublets:
            mine = np.concatenate([2 * marker0, 2 * marker1])
        else:
            mine = 2 * (marker0 if b < n_major else marker1)
        called_hot = 2 * hot[np.arange(HOT) <= b] if b < HOT else 2 * hot  # hot variant j is skipped by the barcodes below j
        vs.append(np.concatenate([mine, called_hot]))
        es.append(np.concatenate([np.zeros(len(mine), np.float32), np.full(len(called_hot), KEEP_ERROR)]))
        cbs.append(np.full(len(mine) + len(called_hot), b))
    v, cb, e = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32), np.concatenate(es).astype(np.float32)
    order = np.lexsort((cb, v))
    return dict(v=v[order], cb=cb[order], e=e[order], v2snp=v2snp, prob=prob, B=B, pools=[[0, 1]], pool_of=np.zeros(B, dtype=np.int32),
                hot=2 * hot, doublets=np.arange(n_doublets), late=np.arange(B - n_late, B))
