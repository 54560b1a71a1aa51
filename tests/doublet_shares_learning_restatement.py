"""Learning from doublets of unequal shares (include/demux_hip_debug.h: dmx_em_doublet_shares, dmx_estep_pair_shares_resident,
dmx_mstep_doublet_shares; Demultiplexer.learn_genotypes_with_doublet_shares) restated with numpy and the oracle, used as
the checker by tests/test_doublet_shares_learning_cpu.py and tests/test_gpu_doublet_shares_learning.py.  Nothing here knows the library.

The loop of tests/doublet_learning_restatement.py with two changes.  The E-step is tests/pair_shares_restatement.restate - every pair
option summed over the grid of shares - and leaves share_mean beside the posteriors.  The M-step credits a live pair k = (d1, d2) of
barcode b, d1 ahead of d2 in the pool's option order, at w = share_mean[b, k]; float32, every operation rounded:
    w_own = w for g == d1, 1 - w for g == d2;  w_other = the other of the two
    a = prob[v, g] * w_own;  o = prob[v, h] * w_other;  r = 0 where a == 0, else a / (a + o);  credit = credit + post[k] * r
Everything else - the live dense credit, the threshold, the option order, (credit * (1 - e)) ** power, np.bincount's float64 sums in
call order - is doublet_learning_restatement's.  A live pair's share_mean is asserted to lie in [0, 1]: nothing clamps it.

The second half is the seeded simulation of DESIGN.md 4.17 and what is demanded on it."""
import functools

import numpy as np

from oracle import demux_oracle
from tests import doublet_learning_restatement as even
from tests import pair_shares_restatement as shares_restated
from tests import pools_learning_restatement as pooled

live_floor = even.live_floor
pair_index = even.pair_index
live_pairs = even.live_pairs
learnt_betas = even.learnt_betas
table_error = even.table_error


def pair_penalties(pools, doublet_prior):
    """float32[n_pools]: tests/pools_restatement.Restatement.pair_penalty."""
    return np.array([demux_oracle.doublet_penalties(len(d), doublet_prior)[-1] if len(d) > 1 else 0.0 for d in pools], dtype=np.float32)


def credits(v, cb, dense, rows, pools, pool_of_barcode, with_doublets, prob, g, power, threshold):
    """float32 credit per call for donor column g, in the stored order of the calls.  rows: 'row_ptr', 'probs', 'share_mean'."""
    pool_of_barcode = np.asarray(pool_of_barcode)
    d = dense[cb, g]
    credit = np.where(d <= live_floor(power), np.float32(0), d).astype(np.float32)
    if not with_doublets:
        return credit
    threshold, one = np.float32(threshold), np.float32(1)
    pool_of_call = pool_of_barcode[cb]
    for p, donors in enumerate(pools):
        donors = [int(x) for x in donors]
        if g not in donors:
            continue
        calls = np.flatnonzero(pool_of_call == p)
        if not len(calls):
            continue
        n, at = len(donors), donors.index(g)
        base = rows['row_ptr'][cb[calls]]
        own = prob[v[calls], g]
        for other in range(n):  # ascending option order: (i, at) for i < at, then (at, j) for j > at
            if other == at:
                continue
            k = pair_index(n, min(at, other), max(at, other))
            post = rows['probs'][base + k]
            live = post >= threshold
            w = rows['share_mean'][base + k]
            assert ((w[live] >= 0) & (w[live] <= 1)).all(), "a live pair's posterior mean share outside [0, 1]"
            with np.errstate(divide='ignore', invalid='ignore'):
                w_first, w_second = w, one - w
                w_own, w_other = (w_first, w_second) if at < other else (w_second, w_first)
                a = own * w_own
                o = prob[v[calls], donors[other]] * w_other
                r = np.where(a == 0, np.float32(0), a / (a + o)).astype(np.float32)
                term = post * r
            assert a.dtype == np.float32 and o.dtype == np.float32 and term.dtype == np.float32
            credit[calls] = np.where(live, credit[calls] + term, credit[calls])
    return credit


def weights(v, cb, e, dense, rows, pools, pool_of_barcode, with_doublets, prob, g, power, threshold):
    keep = 1 - np.asarray(e, dtype=np.float32)
    w = credits(v, cb, dense, rows, pools, pool_of_barcode, with_doublets, prob, g, power, threshold) * keep
    assert w.dtype == np.float32
    if power == 2:
        return w * w
    return np.power(w.astype(np.float64), np.float64(power)).astype(np.float32)


def pooled_columns(pools):
    return sorted({int(g) for donors in pools for g in donors})


def share_addition(v, cb, e, dense, rows, pools, pool_of_barcode, with_doublets, prob, power=2., threshold=1e-3):
    """float32[V, G]: the contract's addition.  (A column of no pool has an all-zero dense column and no pair: its sums are +0.)"""
    V, G = prob.shape
    add = np.zeros((V, G), dtype=np.float32)
    for g in pooled_columns(pools):
        add[:, g] = np.bincount(v, weights=weights(v, cb, e, dense, rows, pools, pool_of_barcode, with_doublets, prob, g, power, threshold), minlength=V)
    return add


def share_addition_of_items(v, cb, e, dense, rows, pools, pool_of_barcode, with_doublets, prob, item_calls, power=2., threshold=1e-3):
    """doublet_learning_restatement.doublet_addition_of_items with this weight: what a combining pass without the redo would write."""
    V, G = prob.shape
    assert (np.diff(v) >= 0).all(), 'variant-major calls'
    first = np.searchsorted(v, v, side='left')
    run = (np.arange(len(v)) - first) // item_calls
    new_item = np.ones(len(v), dtype=bool)
    new_item[1:] = (v[1:] != v[:-1]) | (run[1:] != run[:-1])
    item = np.cumsum(new_item) - 1
    n_items = int(item[-1]) + 1 if len(v) else 0
    item_variant = v[new_item]
    add = np.zeros((V, G), dtype=np.float32)
    for g in pooled_columns(pools):
        w = weights(v, cb, e, dense, rows, pools, pool_of_barcode, with_doublets, prob, g, power, threshold)
        partial = np.bincount(item, weights=w, minlength=n_items)
        add[:, g] = np.bincount(item_variant, weights=partial, minlength=V)
    return add


def estep(v, cb, e, prob, B, pools, pool_of_barcode, penalty, with_doublets, shares, log_weights):
    """(rows, dense): dmx_estep_pair_shares_resident's compact results and the [B, G] singlet posteriors it leaves."""
    rows = shares_restated.restate(v, cb, e, prob, B, pools, pool_of_barcode, penalty, with_doublets, shares, log_weights)
    return rows, pooled.dense_singlets(rows, pools, pool_of_barcode, B, prob.shape[1])


def learn(problem, pools, pool_of_barcode, n_iterations, clip, doublet_prior, shares, log_weights=None, threshold=1e-3, power=2., penalty=None):
    """Per iteration a dict: the E-step's rows (share outputs among them), `dense`, the `addition` its E-step used and the genotype
    table `prob_table`.  log_weights None: all 0, as the C entry reads NULL (the front door passes the uniform prior)."""
    v, cb, e, v2snp, betas, B = (problem[k] for k in ('v', 'cb', 'e', 'v2snp', 'betas', 'B'))
    penalty = pair_penalties(pools, doublet_prior) if penalty is None else penalty
    addition = np.zeros_like(betas)
    history = []
    for _it in range(n_iterations):
        prob = demux_oracle.probs_from_betas(v2snp, betas + addition, clip)
        rows, dense = estep(v, cb, e, prob, B, pools, pool_of_barcode, penalty, doublet_prior != 0, shares, log_weights)
        history.append(dict(rows, dense=dense, addition=addition, prob_table=prob))
        addition = share_addition(v, cb, e, dense, rows, pools, pool_of_barcode, doublet_prior != 0, prob, power=power, threshold=threshold)
    return history


def assert_same(got, want, what):
    """Everything the E-step returns, shares among them, bit for bit."""
    shares_restated.assert_same(got, want, what)


# ---- does it help?  the seeded simulation with doublets of a given share -----------------------------------------------------------
def simulated_problem(share, seed, n_singlets=96, n_doublets=96, calls_per_barcode=256):
    """doublet_learning_restatement.simulated_problem with the doublets' first donor holding `share` of the droplet: the same world,
    the same known / unknown entries (default_rng(1000 + seed))."""
    sim = shares_restated.simulate(share, calls_per_barcode, seed, n_singlets=n_singlets, n_doublets=n_doublets)
    n_snps, G = sim['prob'].shape[0] // 2, sim['prob'].shape[1]
    known = np.repeat(np.random.default_rng(1000 + seed).random((n_snps, G)) < 0.5, 2, axis=0)
    betas = np.where(known, np.float32(2) * sim['prob'], np.float32(1)).astype(np.float32)
    sim = dict(sim, unknown=~known)
    return dict(v=sim['v'], cb=sim['cb'], e=sim['e'], v2snp=sim['v2snp'], betas=betas, raw_betas=betas, B=sim['B']), sim


SEEDS = even.SEEDS
ITERATIONS, CLIP, DOUBLET_PRIOR, THRESHOLD = even.ITERATIONS, even.CLIP, even.DOUBLET_PRIOR, 1e-3
GRID = shares_restated.DEFAULT_SHARES


@functools.lru_cache(maxsize=None)
def simulated(share, seed):
    """(problem, sim, the yardstick's history - doublet_learning_restatement.learn -, this loop's history) at the defaults: nine shares
    0.1 .. 0.9 under the uniform prior, one all-donor pool.  Computed once per (share, seed), shared, read-only."""
    problem, sim = simulated_problem(share, seed)
    G = sim['prob'].shape[1]
    pools, pool_of = [list(range(G))], np.zeros(sim['B'], np.int32)
    yardstick = even.learn(problem, pools, pool_of, ITERATIONS, CLIP, DOUBLET_PRIOR, threshold=THRESHOLD)
    history = learn(problem, pools, pool_of, ITERATIONS, CLIP, DOUBLET_PRIOR, GRID, shares_restated.uniform_log_weights(len(GRID)), threshold=THRESHOLD)
    for records in (yardstick, history):
        for rec in records:
            for value in rec.values():
                value.flags.writeable = False
    return problem, sim, yardstick, history


def true_options(best_option, sim):
    return int((np.asarray(best_option) == sim['true_option']).sum())


# Measured on the CPU with this file (seeds 0 .. 4, 5 iterations, clip 0.01, doublet prior 0.35, threshold 1e-3, nine shares under the
# uniform prior, 96 singlets and 96 doublets of 256 calls; DESIGN.md 4.17 has the table): the error on the unknown entries of this
# loop against doublet_learning_restatement.learn's on the same problem, and the barcodes of 192 whose final arg-max is the true option.
#   share  seed   yardstick   this loop   ratio    arg-max true: yardstick   this loop
#   0.8    0      0.1224      0.1138      0.9296   115                       173
#   0.8    1      0.1213      0.1129      0.9308   116                       177
#   0.8    2      0.1198      0.1117      0.9321   110                       178
#   0.8    3      0.1228      0.1141      0.9292   107                       177
#   0.8    4      0.1204      0.1125      0.9342   118                       172
#   0.5    0      0.1176      0.1174      0.9984   192                       192
#   0.5    1      0.1159      0.1163      1.0033   192                       192
#   0.5    2      0.1159      0.1161      1.0013   192                       192
#   0.5    3      0.1165      0.1169      1.0033   192                       192
#   0.5    4      0.1150      0.1152      1.0017   192                       192
# The demanded ratio at share 0.8 is halfway between the worst measured one and 1 (half the measured gain is margin: DESIGN.md 4.13's
# rule); at share 0.5, where the grid has nothing to find, at most 1 plus that same half-gain.
WORST_MEASURED_RATIO = 0.9342
DEMANDED_RATIO = (WORST_MEASURED_RATIO + 1) / 2
DEMANDED_RATIO_EVEN = 1 + (1 - WORST_MEASURED_RATIO) / 2


def value_condition(share, yardstick_error, error, yardstick_best, best, sim):
    """At share 0.8 this loop's table is closer to the truth than the even loop's by at least half the measured gain, on the entries
    the prior did not know, and no fewer barcodes have their true option as the arg-max; at share 0.5 it is no further than that
    half-gain.  The yardstick is doublet_learning_restatement.learn's error on the same problem."""
    ratio = error / yardstick_error
    found, yardstick_found = true_options(best, sim), true_options(yardstick_best, sim)
    demanded = {0.8: DEMANDED_RATIO, 0.5: DEMANDED_RATIO_EVEN}[share]
    print(f'share {share}: mean |table - truth| on the unknown entries: even loop {yardstick_error:.5f}, this loop {error:.5f}, ratio {ratio:.4f} '
          f'(demanded: at most {demanded:.4f}); arg-max is the true option for {yardstick_found} and {found} of {sim["B"]} barcodes')
    assert ratio <= demanded, (error, yardstick_error)
    if share == 0.8:
        assert found >= yardstick_found, 'fewer barcodes with their true option than in the even loop'
