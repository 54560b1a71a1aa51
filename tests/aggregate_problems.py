"""Designed problems of tests/test_gpu_aggregate_shapes.py (the aggregate_on_snps E-step and the float64 M-step at every kernel form:
csrc/snp_aggregate.hip), built with numpy alone so that the CPU can say what a problem exercises before the device is asked, the
forms the dispatch picks restated as functions of K and G, and the M-step restated in numpy.  Nothing here knows the library."""
import functools

import numpy as np

# ---- the dispatch, restated (csrc/snp_aggregate.hip: dmx_estep_snp, mstep_f64) -----------------------------------------------------
MAX_OPTIONS = 8256  # the doublets of 128 genotypes


def n_options(G, doublets):
    return G * (G + 1) // 2 if doublets else G


def estep_form(K):
    """The E-step's kernel form for K options: 'wave<A>' (a wavefront per barcode, A options per lane, K <= 64 A) up to 1024 options,
    'block<A>' (a workgroup per barcode, A options per thread, K <= 256 A) beyond, None where the E-step refuses."""
    if K > MAX_OPTIONS:
        return None
    for A in (1, 2, 4, 8, 16):
        if K <= 64 * A:
            return f'wave{A}'
    for A in (6, 9, 12, 17, 24, 33):
        if K <= 256 * A:
            return f'block{A}'
    raise AssertionError(K)


def mstep_form(G):
    """The float64 M-step's form for G genotypes: 'm<A>' (A columns per lane, G <= 64 A), and beyond 1024 columns 'm16x<groups>':
    column groups of 1024, each with wavefronts of its own."""
    for A in (1, 2, 4, 8, 16):
        if G <= 64 * A:
            return f'm{A}'
    return f'm16x{(G + 1023) // 1024}'


# (G, doublets, the form the case is there for): both sides of every boundary of the E-step's dispatch
ESTEP_CASES = [
    (10, True, 'wave1'), (11, True, 'wave2'), (15, True, 'wave2'), (16, True, 'wave4'), (22, True, 'wave4'), (23, True, 'wave8'),
    (31, True, 'wave8'), (32, True, 'wave16'), (44, True, 'wave16'), (45, True, 'block6'), (54, True, 'block6'), (55, True, 'block9'),
    (67, True, 'block9'), (68, True, 'block12'), (77, True, 'block12'), (78, True, 'block17'), (92, True, 'block17'),
    (93, True, 'block24'), (110, True, 'block24'), (111, True, 'block33'), (128, True, 'block33'),
    (1, False, 'wave1'), (64, False, 'wave1'), (65, False, 'wave2'), (128, False, 'wave2'), (129, False, 'wave4'),
    (256, False, 'wave4'), (257, False, 'wave8'), (512, False, 'wave8'), (513, False, 'wave16'), (1024, False, 'wave16'),
    (1025, False, 'block6'),
]
PRIOR_CASES = [(11, True, 'wave2'), (45, True, 'block6'), (78, True, 'block17')]
# (G, doublets, the M-step's form): doublets for a row stride K != G
MSTEP_CASES = [
    (64, False, 'm1'), (65, False, 'm2'), (128, False, 'm2'), (129, False, 'm4'), (256, False, 'm4'), (257, False, 'm8'),
    (512, False, 'm8'), (513, False, 'm16'), (1024, False, 'm16'), (1025, False, 'm16x2'), (65, True, 'm2'), (128, True, 'm2'),
]
REFUSED_CASES = [(129, True), (8257, False)]


def case_id(case):
    G, doublets, form = case
    return f"G{G}-{'doublets' if doublets else 'singlets'}-{form}"


# ---- the E-step's shape problem ------------------------------------------------------------------------------------------------------
N_SNPS, B = 40, 9
LONG_SNP, LONG_COUNT = 5, 300  # barcode 2's pair of 300 calls
ZERO_SNP = 7                    # barcode 4's pair with options at -inf: its call on variant 2 * ZERO_SNP has p_base_wrong 0
OTHERS = {5: 5, 6: 33, 7: 65}   # calls of the other barcodes


def zeroed_columns(G):
    """The columns of the table that are 0 on variant 2 * ZERO_SNP: the first and the last, as far as another column stays."""
    return sorted({0, G - 1})[:min(2, G - 1)]


def options_at_minus_inf(G, doublets):
    """The options for which p + e == 0 on barcode 4's call: the singlets of the zeroed columns - two of them from G = 3 on - and,
    with doublets, the pair of the two, whose p is (0 + 0) / 2.  (G = 1 has none: a pair whose only option is at -inf has no
    log_softmax.)"""
    zero = zeroed_columns(G)
    out = list(zero)
    if doublets and len(zero) == 2:
        a, b = zero  # the options behind the singlets: (g1, g2) with g1 < g2, g1-major
        out.append(G + sum(G - 1 - g for g in range(a)) + (b - a - 1))
    return out


@functools.lru_cache(maxsize=None)
def shape_problem(G, seed=0):
    """A small aggregate_on_snps problem for the kernel-shape edges: dict(B, V, v2snp, v, cb, e, prob, mv, mcb, mp) - the barcode
    calls (v, cb, e) of set_problem, in shuffled order; a float32 table for set_probs, uniform in (0.02, 0.98), so that no two options
    tie; the molecule calls (mv, mcb, mp) of set_molecule_calls, the barcodes interleaved, every barcode's calls in the order below.
    40 SNPs of two variants, B = 9 - not a multiple of the four barcodes a workgroup of the wavefront forms walks.
      barcodes 0 and 8   no molecule calls
      barcode 1          one
      barcode 2          300 calls of SNP LONG_SNP, on both its variants (count_pow is indexed at 300, the longest run of
                         calls without a head flag is 299), and eleven pairs of a single call
      barcode 3          six pairs of 2 .. 7 calls that alternate between the SNP's two variants in molecule order, with other pairs'
                         calls in between: inside a pair the float64 accumulation goes in molecule order, which the stable sort by
                         (barcode, SNP) keeps
      barcode 4          a call with p_base_wrong 0 on variant 2 * ZERO_SNP, whose table entries are 0 in zeroed_columns(G): p + e == 0
                         and float32 log gives -inf at options_at_minus_inf(G, doublets), every other option of the pair stays finite
                         (the pair's second call, on the other variant, is finite everywhere); four more pairs
      barcodes 5, 6, 7   5, 33 and 65 calls in shuffled order on SNPs drawn with repetition: repeated (barcode, SNP) pairs
    The barcode calls are the molecule calls' distinct (variant, barcode) and two calls for each of barcodes 0 and 8 (a barcode
    call needs no molecule call here); the last SNP's variants have neither kind of call."""
    rng = np.random.default_rng(1000 * G + seed)
    V = 2 * N_SNPS
    v2snp = np.repeat(np.arange(N_SNPS, dtype=np.int32), 2)
    prob = rng.uniform(0.02, 0.98, size=(V, G)).astype(np.float32)
    prob[2 * ZERO_SNP, zeroed_columns(G)] = 0
    usable = np.setdiff1d(np.arange(N_SNPS - 1), [LONG_SNP, ZERO_SNP])  # (the last SNP has no calls)

    def either(snps):
        return 2 * np.asarray(snps) + rng.integers(0, 2, size=len(snps))

    per_barcode = {1: either(rng.choice(usable, size=1))}
    singles = rng.choice(usable, size=11, replace=False)
    per_barcode[2] = rng.permutation(np.concatenate([either(np.full(LONG_COUNT, LONG_SNP)), either(singles)]))
    snps3 = rng.choice(usable, size=6, replace=False)
    pairs3 = [list(2 * s + np.arange(n) % 2) for s, n in zip(snps3, range(2, 8))]
    calls3 = []
    while any(pairs3):  # round robin over the pairs: a pair's calls keep their order, other pairs' calls lie between them
        for pair in pairs3:
            if pair:
                calls3.append(pair.pop(0))
    per_barcode[3] = np.array(calls3)
    per_barcode[4] = np.concatenate([[2 * ZERO_SNP, 2 * ZERO_SNP + 1], either(rng.choice(usable, size=4, replace=False))])
    for b, n in OTHERS.items():
        per_barcode[b] = either(rng.choice(usable[:12], size=n))
    mv = np.concatenate([per_barcode[b] for b in sorted(per_barcode)]).astype(np.int32)
    mcb = np.concatenate([np.full(len(per_barcode[b]), b) for b in sorted(per_barcode)]).astype(np.int32)
    mp = rng.uniform(0.001, 0.2, size=len(mv)).astype(np.float32)
    mp[(mcb == 4) & (mv == 2 * ZERO_SNP)] = 0
    # molecule order: the barcodes interleaved, every barcode's calls in the order built above
    position = np.empty(len(mv))
    for b in per_barcode:
        position[mcb == b] = np.sort(rng.uniform(size=len(per_barcode[b])))
    order = np.argsort(position, kind='stable')
    mv, mcb, mp = mv[order], mcb[order], mp[order]

    distinct = np.unique(np.stack([mv, mcb], axis=1), axis=0)
    empty = np.array([[3, 0], [40, 0], [3, B - 1], [41, B - 1]])
    calls = rng.permutation(np.concatenate([distinct, empty]))
    v, cb = calls[:, 0].astype(np.int32), calls[:, 1].astype(np.int32)
    e = rng.choice(np.array([0.001, 0.01, 0.05, 0.3], dtype=np.float32), size=len(v))
    problem = dict(B=B, V=V, v2snp=v2snp, v=v, cb=cb, e=e, prob=prob, mv=mv, mcb=mcb, mp=mp)
    for a in problem.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return problem


# ---- a variant spread over several work items ------------------------------------------------------------------------------------
ITEM_CALLS = 1024  # the length of a work item at this number of calls (csrc/kernels.h: item_calls_for), as in
                   # tests/doublet_learning_problems.tie_problem
ITEM_G, ITEM_B, ITEM_HOT_CALLS = 65, 2200, 2150


@functools.lru_cache(maxsize=None)
def item_problem():
    """G = 65 (two columns per lane, the second slot nearly empty), 2 200 barcodes - a float64 posterior table of 1.1 MB - and 12 SNPs.
    Variant 0 is hot: the barcodes below 2 150 call it, which is three work items of 1 024, 1 024 and 102 calls that one wavefront
    walks one after the other.  Variants 1 (the hot SNP's other allele) and 22, 23 (the last SNP) have no calls.  Every barcode calls
    two more variants; the molecule calls are the barcode calls in shuffled order.  Same keys as shape_problem."""
    rng = np.random.default_rng(65)
    G, n_barcodes, n_snps = ITEM_G, ITEM_B, 12
    V = 2 * n_snps
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    prob = rng.uniform(0.02, 0.98, size=(V, G)).astype(np.float32)
    others = np.stack([rng.choice(np.arange(2, V - 2), size=2, replace=False) for _ in range(n_barcodes)])
    v = np.concatenate([np.zeros(ITEM_HOT_CALLS, dtype=np.int64), others.ravel()])
    cb = np.concatenate([np.arange(ITEM_HOT_CALLS), np.repeat(np.arange(n_barcodes), 2)])
    order = rng.permutation(len(v))
    v, cb = v[order].astype(np.int32), cb[order].astype(np.int32)
    e = rng.choice(np.array([0.001, 0.01, 0.05, 0.3], dtype=np.float32), size=len(v))
    order = rng.permutation(len(v))
    problem = dict(B=n_barcodes, V=V, v2snp=v2snp, v=v, cb=cb, e=e, prob=prob, mv=v[order], mcb=cb[order],
                   mp=rng.uniform(0.001, 0.2, size=len(v)).astype(np.float32), hot=0, uncalled=[1, V - 2, V - 1])
    for a in problem.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return problem


# ---- what the E-step should give --------------------------------------------------------------------------------------------------
_expected = {}


def expected(oracle, problem, doublets, compensation=0.5):
    """(logits, posteriors) float64 [B, K] of the oracle (oracle/demux_oracle.py: barcode_logits_aggregated, then scipy's softmax in
    float64 as em_aggregated spells it) on the problem's own table, computed once per (problem, doublets, compensation); read-only."""
    key = (id(problem), bool(doublets), compensation)
    if key not in _expected:
        with np.errstate(divide='ignore'):  # log(0) = -inf is barcode 4's design
            logits = oracle.barcode_logits_aggregated(problem['mv'], problem['mcb'], problem['mp'], problem['v2snp'], problem['prob'],
                                                      problem['B'], 0.5 if doublets else 0., compensation)
        logits.flags.writeable = False
        _expected[key] = (problem, logits, softmax64(logits))  # (the problem is kept alive: its id is the key)
    return _expected[key][1:]


def prior_logits(G, doublets, dtype):
    """Prior logits [B, K] for shape_problem(G): normal with deviation 2, so that the barcodes without calls have no tie either."""
    return np.random.default_rng(G).normal(0, 2, size=(B, n_options(G, doublets))).astype(dtype)


def softmax64(logits):
    shifted = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs = shifted / shifted.sum(axis=1, keepdims=True)
    probs.flags.writeable = False
    return probs


# ---- the float64 M-step, restated (demux.py:113-118 on float64 posteriors) ---------------------------------------------------------
def mstep_f64_restated(v, cb, e, post64, V, G, power, as_float64=False):
    """add[v, g] = float32( sum over the calls c of the variant, in their order, of (post64[cb_c, g] * float64(1 - e_c)) ** power ):
    the reference's loop over the singlet columns - a float64 product of the float64 posterior and the float32 (1 - e), numpy's own
    `**=` (a square at power 2), np.bincount's float64 sum in call order, one rounding to float32.  as_float64: the sums before
    that rounding."""
    assert post64.dtype == np.float64 and e.dtype == np.float32
    keep = 1 - e
    sums = np.zeros([V, G], dtype=np.float64)
    for g in range(G):
        w = post64[cb, g] * keep
        w **= power
        sums[:, g] = np.bincount(v, weights=w, minlength=V)
    return sums if as_float64 else sums.astype(np.float32)
