"""The designed problem of tests/test_gpu_soup_learning.py that decides between the two summation orders of the soup M-step's counts
(DESIGN.md 4.18), built with numpy alone so that the CPU can say what it exercises before the device is asked.
ambient_learning_problems.tie_problem does not decide for this step: its sums are of squares, and at power 1 they sit on no float32 tie.
Nothing here knows the library."""
import functools

import numpy as np

HOT, MARKERS, WINDOW, KEEP_ERROR = 32, 64, 30, np.float32(2.0 ** -20)
N_MAJOR, N_MINOR, N_LATE, N_MOSTLY_SOUP = 2900, 96, 4, 103
TIE_AT = 5  # the hot variant whose count of column 0 sits on the tie
LATE_ENTRY = np.float32(0.0242)  # table entry of donor 0 at the late barcodes' window calls: sets their posterior of donor 0


@functools.lru_cache(maxsize=None)
def tie_problem():
    """Two donors, 3 000 barcodes, a genotype table set by hand (dmx_set_probs), a supplied soup of 0.5 everywhere.
      barcodes 0 .. 2899    donor 0: 64 marker calls that leave posterior (1, ~0); alpha 0.75 for the first 103, else 0.5
      barcodes 2900 .. 2995 donor 1, alpha 0: they count nothing (s == 0)
      barcodes 2996 .. 2999 donor 1 through 30 window calls whose table entries leave posterior(donor 0) near 1.6e-13, alpha 0.5: a
                            contribution of about 8e-14 to column 0 of every hot variant
      hot variant j < 32    table row (0.5, 0.5), soup 0.5, p_base_wrong 2^-20, called by every barcode but the first j: about 2 990
                            calls, three work items of 1 024.  s is 0.75 exactly at alpha 0.75 (0.375 / 0.5) and 0.5 exactly at 0.5, so
                            a donor-0 barcode counts (1 - 2^-20) s for column 0 and the exact part of the sum is n (1 - 2^-20) / 4 with
                            n = 3 (103 - j) + 2 * 2797 = 5903 - 3 j: between 1024 and 2048, where float32 ties are the odd multiples
                            of 2^-14, it is a tie when n is an odd multiple of 256, and the even neighbour is the lower one when that
                            odd number is 3 mod 4: n = 5888 = 256 * 23 at j = 5.  In call order the four late contributions are each
                            below half an ulp of the running float64 sum (1.1e-13 above 1024) and are lost: the sum stays ON the tie and
                            rounds to even, down.  Inside the third item's partial sum (below 1024: half an ulp 5.7e-14) they are kept,
                            and their total moves the sum of the partials above the tie: it rounds up.
    Returns dict(v, cb, e, v2snp, prob, B, alpha, soup, pools, pool_of, hot, late) - variant-major calls, hot: the hot variants' ids."""
    B, G = N_MAJOR + N_MINOR + N_LATE, 2
    late = np.arange(B - N_LATE, B)
    marker0 = np.arange(0, MARKERS)                # SNP s: variants 2 s, 2 s + 1
    marker1 = np.arange(MARKERS, 2 * MARKERS)
    window = np.arange(2 * MARKERS, 2 * MARKERS + WINDOW)
    hot = np.arange(2 * MARKERS + WINDOW, 2 * MARKERS + WINDOW + HOT)
    n_snps = 2 * MARKERS + WINDOW + HOT
    V = 2 * n_snps
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    prob = np.full((V, G), 0.5, dtype=np.float32)
    prob[2 * marker0] = [0.99, 0.01]
    prob[2 * marker0 + 1] = [0.01, 0.99]
    prob[2 * marker1] = [0.01, 0.99]
    prob[2 * marker1 + 1] = [0.99, 0.01]
    prob[2 * window] = [LATE_ENTRY, 0.9]
    prob[2 * window + 1] = [np.float32(1) - LATE_ENTRY, 0.1]
    soup = np.full(V, 0.5, dtype=np.float32)
    alpha = np.zeros(B, dtype=np.float32)
    alpha[:N_MAJOR] = 0.5
    alpha[:N_MOSTLY_SOUP] = 0.75
    alpha[late] = 0.5
    vs, cbs, es = [], [], []
    for b in range(B):
        mine = 2 * (window if b >= B - N_LATE else marker0 if b < N_MAJOR else marker1)
        called_hot = 2 * hot[np.arange(HOT) <= b] if b < HOT else 2 * hot  # hot variant j is skipped by the barcodes below j
        vs.append(np.concatenate([mine, called_hot]))
        es.append(np.concatenate([np.zeros(len(mine), np.float32), np.full(len(called_hot), KEEP_ERROR)]))
        cbs.append(np.full(len(mine) + len(called_hot), b))
    v, cb, e = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32), np.concatenate(es).astype(np.float32)
    order = np.lexsort((cb, v))
    return dict(v=v[order], cb=cb[order], e=e[order], v2snp=v2snp, prob=prob, B=B, alpha=alpha, soup=soup, pools=[[0, 1]],
                pool_of=np.zeros(B, dtype=np.int32), hot=2 * hot, late=late)
