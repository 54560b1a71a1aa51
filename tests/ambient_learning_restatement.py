"""Learning under per-barcode ambient fractions (include/demux_hip_debug.h: dmx_em_ambient; Demultiplexer.learn_genotypes_with_ambient;
DESIGN.md 4.9) restated with numpy and the oracle, used as the checker by tests/test_ambient_learning_cpu.py and
tests/test_gpu_ambient_learning.py.

The loop of tests/pools_learning_restatement.py with two changes per iteration, all in float32, every operation rounded:
    rows     = ambient_scoring_restatement.restate on this iteration's table, with the caller's alpha[b] and the soup's profile ambient[v]
    dense    = pools_learning_restatement.dense_singlets(rows, ...)
    own = prob[v, g] * (1 - alpha[b]);  mix = own + ambient[v] * alpha[b];  r = 0 where own == 0, else own / mix
    w   = ((dense[b, g] * (1 - e)) * r) ** power       power 2: one float32 product; another power: f32(f64(base) ** f64(power)) - a
                                                       float32 `**` is libm's or a vector library's, whichever the host's numpy has
    addition[v, g] = f32( sum over the calls of v, in their stored order, of f64(w) )          (np.bincount: one float64 accumulator)
r is the probability that the call came from the donor and not from the soup.  With alpha == 0 it is q / q == 1 for every table entry
q != 0, so w is oracle.beta_addition's and the loop is pools_learning_restatement.learn bit for bit on a clipped table.  Nothing here
knows the library."""
import numpy as np

from oracle import demux_oracle
from tests import ambient_scoring_restatement as scoring
from tests import pools_learning_restatement as pooled


def donor_share(prob_vg, alpha_b, ambient_v):
    """r per call for one donor column: float32, the three roundings of the contract and one IEEE division."""
    own = prob_vg * (np.float32(1) - alpha_b)
    mix = own + ambient_v * alpha_b
    assert own.dtype == np.float32 and mix.dtype == np.float32
    with np.errstate(divide='ignore', invalid='ignore'):
        r = own / mix
    return np.where(own == 0, np.float32(0), r).astype(np.float32)


def weights(v, cb, e, dense, prob, alpha, ambient, g, power):
    """float32 w per call for donor column g, in the stored order of the calls."""
    keep = 1 - np.asarray(e, dtype=np.float32)
    w = (dense[cb, g] * keep) * donor_share(prob[v, g], alpha[cb], ambient[v])
    assert w.dtype == np.float32
    if power == 2:
        return w * w  # (what numpy's `w **= 2.` is: oracle.beta_addition's line)
    return np.power(w.astype(np.float64), np.float64(power)).astype(np.float32)


def ambient_addition(v, cb, e, dense, prob, alpha, ambient, power=2.):
    """float32[V, G]: oracle.beta_addition with every call weighted by its donor share."""
    V, G = prob.shape
    alpha, ambient = np.asarray(alpha, dtype=np.float32), np.asarray(ambient, dtype=np.float32)
    add = np.zeros((V, G), dtype=np.float32)
    for g in range(G):
        add[:, g] = np.bincount(v, weights=weights(v, cb, e, dense, prob, alpha, ambient, g, power), minlength=V)
    return add


def ambient_addition_of_items(v, cb, e, dense, prob, alpha, ambient, item_calls, power=2.):
    """float32[V, G]: the same sums formed as the float64 partial sums of runs of item_calls consecutive calls of a variant, added
    in run order - what a combining pass without the redo would write.  Differs from ambient_addition only in float32 rounding ties."""
    V, G = prob.shape
    alpha, ambient = np.asarray(alpha, dtype=np.float32), np.asarray(ambient, dtype=np.float32)
    assert (np.diff(v) >= 0).all(), 'variant-major calls'
    first = np.searchsorted(v, v, side='left')
    run = (np.arange(len(v)) - first) // item_calls
    new_item = np.ones(len(v), dtype=bool)
    new_item[1:] = (v[1:] != v[:-1]) | (run[1:] != run[:-1])
    item = np.cumsum(new_item) - 1
    n_items = int(item[-1]) + 1 if len(v) else 0
    item_variant = v[new_item]
    add = np.zeros((V, G), dtype=np.float32)
    for g in range(G):
        partial = np.bincount(item, weights=weights(v, cb, e, dense, prob, alpha, ambient, g, power), minlength=n_items)
        add[:, g] = np.bincount(item_variant, weights=partial, minlength=V)
    return add


def learn(problem, pools, pool_of_barcode, alpha, ambient, n_iterations, clip, doublet_prior, power=2., weighted=True):
    """Per iteration a dict: the pooled ambient E-step's rows, `dense`, the `addition` its E-step used and the genotype table
    `prob_table`.  weighted=False: the ambient E-step in front of the plain M-step (what the weights are measured against)."""
    v, cb, e, v2snp, betas, B = (problem[k] for k in ('v', 'cb', 'e', 'v2snp', 'betas', 'B'))
    V, G = betas.shape
    alpha, ambient = np.asarray(alpha, dtype=np.float32), np.asarray(ambient, dtype=np.float32)
    penalty = np.array([demux_oracle.doublet_penalties(len(d), doublet_prior)[-1] if len(d) > 1 else 0.0 for d in pools], dtype=np.float32)
    addition = np.zeros_like(betas)
    history = []
    for _it in range(n_iterations):
        prob = demux_oracle.probs_from_betas(v2snp, betas + addition, clip)
        rows = scoring.restate(v, cb, e, prob, B, pools, pool_of_barcode, penalty, doublet_prior != 0, alpha, ambient)
        dense = pooled.dense_singlets(rows, pools, pool_of_barcode, B, G)
        history.append(dict(rows, dense=dense, addition=addition, prob_table=prob))
        if weighted:
            addition = ambient_addition(v, cb, e, dense, prob, alpha, ambient, power=power)
        else:
            addition = demux_oracle.beta_addition(v, cb, e, dense, V, G, power=power)
    return history


def learnt_betas(problem, history):
    """genotypes.get_betas() + the addition the last E-step used (demux.py:65)."""
    return problem['raw_betas'] + history[-1]['addition']


# ---- the value condition on the seeded simulation -----------------------------------------------------------------------------
def simulated_problem(seed, n_barcodes=192, calls_per_barcode=256):
    """(problem, sim): ambient_restatement.simulate as a learning problem whose prior betas (0.5 prob + 0.25) 2 know half of the truth."""
    from tests import ambient_restatement
    sim = ambient_restatement.simulate(seed, n_barcodes=n_barcodes, calls_per_barcode=calls_per_barcode)
    betas = ((np.float32(0.5) * sim['prob'] + np.float32(0.25)) * np.float32(2)).astype(np.float32)
    return dict(v=sim['v'], cb=sim['cb'], e=sim['e'], v2snp=sim['v2snp'], betas=betas, raw_betas=betas, B=sim['B']), sim


def table_error(history, sim):
    """Mean absolute error of the last iteration's genotype table against the simulation's."""
    return float(np.abs(history[-1]['prob_table'].astype(np.float64) - sim['prob']).mean())


def value_condition(plain_error, weighted_error, best_option, sim):
    """The weighted loop's table is at least a tenth closer to the truth than the plain loop's, and every barcode keeps its donor."""
    print(f'mean |table - truth|: plain loop {plain_error:.5f}, weighted M-step {weighted_error:.5f}, ratio {weighted_error / plain_error:.3f}')
    assert weighted_error <= 0.9 * plain_error, (weighted_error, plain_error)
    assert np.array_equal(np.asarray(best_option), sim['donor1']), 'an arg-max is not the true donor'
