"""Designed problems of tests/test_gpu_snp_detection_edges.py (SNP detection at the edges of its kernels: csrc/snp_detect.hip), built with
numpy alone so that the CPU can say what a problem holds before the device is asked (tests/test_snp_detection_problems_cpu.py).  The
expectations come from the restatement of tests/test_snp_detection_cpu.py; what is here are inputs, closed forms where a design has one,
a way to read the whole overall ranking out of `select`, and two WRONG row sums that show which designs notice a wrong association.

A problem is a list of parts [(chrom number, CompressedSNPCalls)] - the explicit form of flat_calls / count - a donor_of_barcode
and a donor count.  containers() turns parts into what DeviceContext.snp_count takes."""
import numpy as np

from demuxalot_amd import CompressedSNPCalls

P_GOOD = np.float32(0.001)
COUNT_CHUNK, COUNT_BLOCK = 16, 4096  # sorted keys per lane and per workgroup of k_sd_accumulate


def containers(parts):
    return [(chrom, calls.snp_calls[:calls.n_snp_calls], calls.molecules[:calls.n_molecules]) for chrom, calls in parts]


def _calls(barcode, position, base, p, n_barcodes, rng=None):
    """A container with one molecule per barcode and the given calls, shuffled in input order when an rng is given."""
    barcode, position, base = np.asarray(barcode, dtype=np.int32), np.asarray(position, dtype=np.int64), np.asarray(base, dtype=np.uint8)
    p = np.broadcast_to(np.asarray(p, dtype=np.float32), barcode.shape)
    order = rng.permutation(len(barcode)) if rng is not None else np.arange(len(barcode))
    return CompressedSNPCalls.from_arrays(np.arange(n_barcodes, dtype=np.int32), barcode[order], position[order].astype(np.int32),
                                          base[order], p[order])


# ---- the row sum's association: positions that differ only in the order of their donors ------------------------------------------------
TWIN_P = 128
# both ends of the 8-lane block (8, 9, 127, 128), the first split and the halves it makes (129, 135, 136, 255 .. 257), deeper trees, and
# the lengths around the ones that are still longer than a block after six splits (overlong_block: 7689, 7951, 8191, not 7688, 8192)
TWIN_DONORS = (1, 7, 8, 9, 127, 128, 129, 135, 136, 255, 256, 257, 1000, 4097, 7688, 7689, 7951, 8191, 8192)
# seeds found by search_twin_seed (tests/test_snp_detection_problems_cpu.py asserts what they were searched for)
TWIN_SEEDS = {D: 1 if D == 8 else 0 for D in TWIN_DONORS}
TWIN_DUPLICATES = 4


def twin_positions(D, P=TWIN_P, seed=0):
    """P positions whose rows of importances are rotations of each other: one per-donor pattern - counts in {0, 1} on two bases, from
    one barcode per donor or two (the seed decides) - rolled by a different number of donors at every position (by p mod D where
    D < P), and TWIN_DUPLICATES positions that repeat another's roll exactly.  Every row sum is the same number mathematically; in
    float64 the sums take a handful of values an ulp or a few apart, so the overall ranking is decided by the association of the sum,
    and among equal rows by stability.  -> (parts, donor_of_barcode, counts int32[P, D, 4], rolls int64[P])."""
    rng = np.random.default_rng(seed)
    per_donor = 1 + int(rng.integers(0, 2))
    base_a, base_b = rng.permutation(4)[:2]
    pattern = rng.integers(0, 2, (D, 2))
    pattern[0] = (1, 0)
    rolls = rng.permutation(D)[:P] if D >= P else np.arange(P) % D
    twins = rng.permutation(P)[:2 * TWIN_DUPLICATES]
    rolls[twins[TWIN_DUPLICATES:]] = rolls[twins[:TWIN_DUPLICATES]]
    rolled = pattern[(np.arange(D)[None, :] - rolls[:, None]) % D]  # [P, D, 2]
    counts = np.zeros((P, D, 4), dtype=np.int32)
    counts[:, :, base_a], counts[:, :, base_b] = rolled[:, :, 0], rolled[:, :, 1]
    position, donor, base = np.nonzero(counts)
    barcode = donor + D * rng.integers(0, per_donor, len(donor))
    calls = _calls(barcode, 100 + 3 * position, base, P_GOOD, D * per_donor, rng)
    return [(0, calls)], (np.arange(D * per_donor) % D).astype(np.int32), counts, rolls


def ranking_via_select(select_fn, P):
    """The whole overall ranking, from a select(n_best, n_additional) alone: with n_best = 0 no position is a member, every position
    is new, and select(0, k) is exactly the first k of the ranking (as a sorted set): the k-th is the one that select(0, k + 1) adds."""
    ranking, before = [], set()
    for k in range(P + 1):
        selected = [int(i) for i in select_fn(0, k)]
        assert len(selected) == k and selected == sorted(selected) and before <= set(selected), (k, selected)
        ranking.extend(set(selected) - before)
        before = set(selected)
    return np.asarray(ranking, dtype=np.int64)


# Two WRONG stand-ins for importances.sum(axis=1) (test_snp_detection_cpu.select's row_sum), each over all rows at once.
def sequential_row_sum(importances):
    """Mutant (a): the elements added left to right."""
    total = importances[:, 0].copy()
    for d in range(1, importances.shape[1]):
        total = total + importances[:, d]
    return total


def tree_row_sum(importances, depth=None):
    """numpy's pairwise tree with at most `depth` splits; what is left after them is summed as ONE 8-lane block however long it is.
    depth=None is numpy's own sum; depth=6 is mutant (b), the kernel before the row sum moved to csrc/pairwise_sum.h."""
    n = importances.shape[1]
    if n < 8:
        total = np.zeros(len(importances))
        for d in range(n):
            total = total + importances[:, d]
        return total
    if depth == 0 or n <= 128:
        lanes = importances[:, :8].copy()
        full = n - n % 8
        for i in range(8, full, 8):
            lanes += importances[:, i:i + 8]
        total = ((lanes[:, 0] + lanes[:, 1]) + (lanes[:, 2] + lanes[:, 3])) + ((lanes[:, 4] + lanes[:, 5]) + (lanes[:, 6] + lanes[:, 7]))
        for d in range(full, n):
            total = total + importances[:, d]
        return total
    half = n // 2
    half -= half % 8
    below = None if depth is None else depth - 1
    return tree_row_sum(importances[:, :half], below) + tree_row_sum(importances[:, half:], below)


def depth6_row_sum(importances):
    return tree_row_sum(importances, 6)


def overlong_block(n, depth=6):
    """Whether `depth` splits of numpy's tree leave a node of n elements with more than 128: the lengths at which a recursion limited
    to that depth sums in another association than numpy."""
    if n <= 128:
        return False
    if depth == 0:
        return True
    half = n // 2
    half -= half % 8
    return overlong_block(half, depth - 1) or overlong_block(n - half, depth - 1)


def twin_mutants(D):
    """The wrong sums that the seed of twin_positions(D) must tell from numpy's: the sequential one from 8 donors on (below, numpy's sum
    is sequential itself), the depth-6 tree where it differs from numpy's at all."""
    return ([sequential_row_sum] if D >= 8 else []) + ([depth6_row_sum] if overlong_block(D) else [])


def search_twin_seed(D, score, tries=200):
    """The first seed at which the ranking of twin_positions(D) under each of twin_mutants(D) differs from the one under numpy's sum
    (how TWIN_SEEDS was found; `score` is the restatement's)."""
    for seed in range(tries):
        importances = score(twin_positions(D, seed=seed)[2])[0]
        ranking = np.argsort(-importances.sum(axis=1), kind='stable')
        if all(not np.array_equal(np.argsort(-mutant(importances), kind='stable'), ranking) for mutant in twin_mutants(D)):
            return seed
    raise AssertionError(f'no seed below {tries} separates the sums at D = {D}')


# ---- runs of equal keys against the cap, the 16-key chunk of a lane and the 4096 keys of a workgroup ------------------------------------
RUN_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097)
RUN_OFFSETS = tuple(range(17))
RUN_CAPS = (0, 1, 2, 15, 16, 17, 4096, 2 ** 31 - 1)
KEPT_TOTALS = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)


def run_problem(offset, lengths=RUN_LENGTHS, seed=0):
    """One run of equal (barcode, position, base) keys per entry of `lengths`: run i is barcode i of donor i with lengths[i] calls of
    base 4 i // len(lengths) at position 9, so the sorted key array (position, base, donor, barcode) holds the runs back to back in the
    order of `lengths`.  Position 5, which sorts ahead, holds `offset` single calls of distinct further barcodes (barcode
    len(lengths) + j: donor j mod D, base j mod 4), so every run starts `offset` keys later.  All calls are shuffled in input order.
    -> (parts, donor_of_barcode, D, starts: where each run begins in the sorted keys)."""
    rng = np.random.default_rng(seed)
    D = len(lengths)
    run = np.repeat(np.arange(D), lengths)
    single = np.arange(offset)
    barcode = np.concatenate([run, D + single])
    position = np.concatenate([np.full(len(run), 9), np.full(offset, 5)])
    base = np.concatenate([4 * run // D, single % 4])
    dob = np.concatenate([np.arange(D), single % D]).astype(np.int32)
    starts = offset + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return [(0, _calls(barcode, position, base, P_GOOD, D + offset, rng))], dob, D, starts


def run_counts(offset, lengths, cap):
    """The closed form of run_problem's counts, int32[P, D, 4] with P = 2 (1 without singles): min(length, cap) per run."""
    D = len(lengths)
    counts = np.zeros((2, D, 4), dtype=np.int32)
    for j in range(offset):
        counts[0, j % D, j % 4] += min(1, cap)
    for i, length in enumerate(lengths):
        counts[1, i, 4 * i // D] = min(length, cap)
    return counts if offset else counts[1:]


def kept_total_problem(m, seed=0):
    """Exactly m kept calls - random over 5 positions x 2 parts, 4 bases and 6 assigned barcodes of 3 donors - among m // 2 + 3 dropped
    ones (p_base_wrong float32(0.01), base N, or barcode 6, which has no donor).  -> (parts, donor_of_barcode, D, cap 2)."""
    rng = np.random.default_rng([m, seed])
    dob = np.array([0, 1, 2, 2, 0, 1, -1], dtype=np.int32)
    n_drop = m // 2 + 3
    split = int(rng.integers(0, m + 1))
    parts = []
    for chrom, kept, dropped in ((0, split, n_drop // 2), (1, m - split, n_drop - n_drop // 2)):
        why = rng.integers(0, 3, dropped)
        barcode = np.concatenate([rng.integers(0, 6, kept), np.where(why == 2, 6, rng.integers(0, 6, dropped))])
        base = np.concatenate([rng.integers(0, 4, kept), np.where(why == 1, 4, rng.integers(0, 4, dropped))])
        p = np.concatenate([np.full(kept, P_GOOD), np.where(why == 0, np.float32(0.01), P_GOOD)]).astype(np.float32)
        parts.append((chrom, _calls(barcode, 7 * rng.integers(0, 5, kept + dropped), base, p, len(dob), rng)))
    return parts, dob, 3, 2


# ---- the filter ---------------------------------------------------------------------------------------------------------------------------
P_VALUES = np.array([np.nan, -1., -0., 0., 0.0099, np.float32(0.01), 1., np.inf], dtype=np.float32)
BASE_VALUES = (0, 1, 2, 3, 4, 5, 255)
THRESHOLDS = (np.float32(0.01), np.float32(np.inf), np.float32(-0.), np.float32(0.))


def filter_problem():
    """Every p_base_wrong of P_VALUES x every base_index of BASE_VALUES x barcodes 0, 1, 2 (donors 0, none, 1), one call each, at position
    16 * (index of p) + (index of base): which positions appear says which (p, base) were kept.  -> (parts, donor_of_barcode, D)."""
    ip, ib, barcode = [a.ravel() for a in np.meshgrid(np.arange(len(P_VALUES)), np.arange(len(BASE_VALUES)), np.arange(3), indexing='ij')]
    calls = _calls(barcode, 16 * ip + ib, np.asarray(BASE_VALUES)[ib], P_VALUES[ip], 3, np.random.default_rng(1))
    return [(0, calls)], np.array([0, -1, 1], dtype=np.int32), 2


def nothing_kept_problems():
    """{name: (parts, donor_of_barcode, D, threshold)} of inputs that keep no call at all: no part, parts without calls (with and without
    molecules), every call dropped by one rule of the filter, and good calls (p_base_wrong 0, -0 and above) under thresholds 0 and NaN."""
    rng = np.random.default_rng(2)
    n = 40
    barcode, position, base = rng.integers(0, 4, n), rng.integers(-3, 3, n), rng.integers(0, 4, n)
    assigned, nobody = np.array([0, 1, 1, 0], dtype=np.int32), np.full(4, -1, dtype=np.int32)
    good = rng.choice(np.array([0., -0., 0.001, 0.0099], dtype=np.float32), n)
    bad = rng.choice(np.array([np.float32(0.01), 0.02, 1., np.inf, np.nan], dtype=np.float32), n)
    usual = np.float32(0.01)

    def two_parts(base, p):
        return [(0, _calls(barcode[:25], position[:25], base[:25], p[:25], 4)), (1, _calls(barcode[25:], position[25:], base[25:], p[25:], 4))]

    return {
        'no part': ([], assigned, 2, usual),
        'parts without calls': ([(0, _calls([], [], [], P_GOOD, 0)), (3, _calls([], [], [], P_GOOD, 4))], assigned, 2, usual),
        'p_base_wrong not below the threshold': (two_parts(base, bad), assigned, 2, usual),
        'base_index 4 and above': (two_parts(rng.choice(np.array([4, 5, 255]), n), good), assigned, 2, usual),
        'no barcode assigned': (two_parts(base, good), nobody, 2, usual),
        'threshold 0': (two_parts(base, good), assigned, 2, np.float32(0.)),
        'threshold NaN': (two_parts(base, good), assigned, 2, np.float32(np.nan)),
    }


# ---- keys and order -----------------------------------------------------------------------------------------------------------------------
EXTREME_POSITIONS = (-2 ** 31, -2 ** 31 + 1, -1, 0, 1, 2 ** 31 - 1)
EXTREME_CHROMS = (5, 0, 5, 2 ** 31 - 1)
SCATTERED_CHROMS = (7, 2 ** 31 - 1, 0, 7, 3, 0, 2 ** 31 - 2)


def positions_problem(chroms, positions, seed=0):
    """One part per entry of `chroms` (repeats merge; the order is the list's, not the values'), each with 3 calls per position of
    `positions` in shuffled order - 5 barcodes of 2 donors, one of them unassigned - plus, in every part, two calls of barcode 0 with base
    0 at positions[0]: parts of equal chrom make one run of them, which the cap (3) then cuts.  -> (parts, donor_of_barcode, D)."""
    rng = np.random.default_rng(seed)
    parts = []
    for chrom in chroms:
        position = np.concatenate([np.repeat(positions, 3), [positions[0]] * 2])
        barcode = rng.integers(0, 5, (len(positions), 3))
        barcode[:, 0] = rng.choice([0, 1, 3, 4], len(positions))  # (every position is kept in every part)
        barcode = np.concatenate([barcode.ravel(), [0, 0]])
        base = np.concatenate([rng.integers(0, 4, len(position) - 2), [0, 0]])
        parts.append((chrom, _calls(barcode, position, base, P_GOOD, 5, rng)))
    return parts, np.array([0, 1, -1, 1, 0], dtype=np.int32), 2


def one_donor_one_barcode():
    """D = 1 and B = 1: both the donor and the barcode field of the sorted key are zero bits wide.  4 positions, runs of 1 to 5."""
    position = np.repeat([4, -4, 0, 9], [5, 1, 3, 4])
    base = np.array([0, 0, 0, 0, 0, 3, 1, 1, 2, 0, 0, 3, 3])
    return [(0, _calls(np.zeros(len(position), dtype=int), position, base, P_GOOD, 1, np.random.default_rng(3)))], np.zeros(1, dtype=np.int32), 1


def one_position():
    """P = 1: 30 calls of 4 barcodes (3 donors) on one position, in two parts of the same chrom."""
    rng = np.random.default_rng(4)
    parts = [(2, _calls(rng.integers(0, 4, 15), np.full(15, -7), rng.integers(0, 4, 15), P_GOOD, 4)) for _ in range(2)]
    return parts, np.array([2, 0, 1, 0], dtype=np.int32), 3


def random_parts(rng, n_chrom, n_calls, n_barcodes, n_positions):
    """Random problems full of ties, as tests/test_gpu_snp_detection.py's _random_calls makes them, as parts."""
    parts = []
    for k in range(n_chrom):
        n = n_calls // n_chrom
        position = rng.integers(0, n_positions, n) * 3
        base = rng.choice(5, n, p=[0.35, 0.3, 0.15, 0.15, 0.05])
        p = rng.choice(np.asarray([0.001, 0.005, np.float32(0.01), 0.02, 0.0099], dtype=np.float32), n, p=[0.5, 0.2, 0.1, 0.1, 0.1])
        parts.append((k, _calls(rng.integers(0, n_barcodes, n), position, base, p, n_barcodes)))
    return parts
