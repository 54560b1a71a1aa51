"""Learning the soup's allele profile (include/demux_hip_debug.h: dmx_mstep_soup, dmx_em_ambient_soup; Demultiplexer.learn_ambient_profile,
learn_genotypes_and_ambient) restated with numpy and the oracle, used as the checker by tests/test_soup_learning_cpu.py
and tests/test_gpu_soup_learning.py.

The third M-step of the ambient model.  For variant v, donor column g and the calls c of v in stored order, b = cb_c, all in float32,
every operation rounded:
    amb = ambient[v] * alpha[b];  own = prob[v, g] * (1 - alpha[b]);  mix = own + amb;  s = 0 where amb == 0, else amb / mix
    t   = (dense[b, g] * (1 - e)) * s                   power 1: expected counts
    count[v, g] = f32( sum over the calls with dense[b, g] != 0, in their stored order, of f64(t) )     (np.bincount: one float64 accumulator)
    total[v]    = f32( sum over g ascending of f64(count[v, g]) )
    beta[v]     = total[v] + pseudo_count
    ambient'[v] = oracle.probs_from_betas on the one column beta[:, None], clipped         (ambient_restatement.derived_ambient's line)
s is the probability that the call came from the soup and not from the donor: the complement of ambient_learning_restatement's
donor_share.  The loop is ambient_learning_restatement.learn with the profile replaced after every iteration; the genotype M-step of
an iteration reads the profile its E-step read.  Nothing here knows the library."""
import numpy as np

from oracle import demux_oracle
from tests import ambient_learning_restatement as learning
from tests import ambient_restatement
from tests import ambient_scoring_restatement as scoring
from tests import pools_learning_restatement as pooled


def soup_share(prob_vg, alpha_b, ambient_v):
    """s per call for one donor column: float32, the three roundings of the contract and one IEEE division."""
    amb = ambient_v * alpha_b
    own = prob_vg * (np.float32(1) - alpha_b)
    mix = own + amb
    assert amb.dtype == np.float32 and mix.dtype == np.float32
    with np.errstate(divide='ignore', invalid='ignore'):
        s = amb / mix
    return np.where(amb == 0, np.float32(0), s).astype(np.float32)


def terms(v, cb, e, dense, prob, alpha, ambient, g):
    """float32 t per call for donor column g, in the stored order of the calls; +0 where the posterior is not live (whatever the
    fraction of such a barcode is - that of a barcode in no pool is never looked at)."""
    keep = 1 - np.asarray(e, dtype=np.float32)
    post = dense[cb, g]
    with np.errstate(invalid='ignore'):
        t = (post * keep) * soup_share(prob[v, g], alpha[cb], ambient[v])
    assert t.dtype == np.float32
    return np.where(post != 0, t, np.float32(0)).astype(np.float32)


def totals(count):
    """float32[V]: the columns of count[V, G] added in ascending order into one float64 accumulator per variant."""
    acc = np.zeros(count.shape[0], dtype=np.float64)
    for g in range(count.shape[1]):
        acc = acc + count[:, g].astype(np.float64)
    return acc.astype(np.float32)


def soup_counts(v, cb, e, dense, prob, alpha, ambient):
    """(count float32[V, G], total float32[V]): the soup's expected calls per (variant, donor column) and per variant."""
    V, G = prob.shape
    alpha, ambient = np.asarray(alpha, dtype=np.float32), np.asarray(ambient, dtype=np.float32)
    count = np.zeros((V, G), dtype=np.float32)
    for g in range(G):
        count[:, g] = np.bincount(v, weights=terms(v, cb, e, dense, prob, alpha, ambient, g), minlength=V)
    return count, totals(count)


def soup_counts_of_items(v, cb, e, dense, prob, alpha, ambient, item_calls):
    """The same formed as the float64 partial sums of runs of item_calls consecutive calls of a variant, added in run order - what a
    combining pass without the redo would write.  Differs from soup_counts only where a float32 rounding boundary is near."""
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
    count = np.zeros((V, G), dtype=np.float32)
    for g in range(G):
        partial = np.bincount(item, weights=terms(v, cb, e, dense, prob, alpha, ambient, g), minlength=n_items)
        count[:, g] = np.bincount(item_variant, weights=partial, minlength=V)
    return count, totals(count)


def profile_from_totals(total, v2snp, pseudo_count, clip):
    """float32[V]: the P-step's formula on the one column total + pseudo_count."""
    betas = (np.asarray(total, dtype=np.float32) + np.float32(pseudo_count))[:, None]
    assert betas.dtype == np.float32
    return np.ascontiguousarray(demux_oracle.probs_from_betas(v2snp, betas, clip)[:, 0])


def soup_update(v, cb, e, dense, prob, alpha, ambient, v2snp, pseudo_count=1., clip=0.01):
    """(ambient' float32[V], total float32[V]): one soup M-step on the posteriors `dense` of an E-step that read `prob`, `alpha`, `ambient`."""
    _count, total = soup_counts(v, cb, e, dense, prob, alpha, ambient)
    return profile_from_totals(total, v2snp, pseudo_count, clip), total


def learn(problem, pools, pool_of_barcode, alpha, ambient, n_iterations, clip, doublet_prior, power=2., pseudo_count=1., fixed=False):
    """ambient_learning_restatement.learn with the soup's profile learnt: per iteration a dict with the pooled ambient E-step's rows
    (their 'ambient': the profile the E-step read), `dense`, the `addition` its E-step used, `prob_table`, and what the soup M-step
    behind this E-step gives: `counts` (total) and `next_ambient`.  fixed=True: the update is computed and ignored."""
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
        next_ambient, total = soup_update(v, cb, e, dense, prob, alpha, ambient, v2snp, pseudo_count, clip)
        history.append(dict(rows, dense=dense, addition=addition, prob_table=prob, counts=total, next_ambient=next_ambient))
        addition = learning.ambient_addition(v, cb, e, dense, prob, alpha, ambient, power=power)
        if not fixed:
            ambient = next_ambient
    return history


def learn_profile(problem, prob, pools, pool_of_barcode, alpha, ambient, n_iterations, clip, doublet_prior, pseudo_count=1.):
    """The genotypes fixed (the table `prob`): n_iterations of (ambient E-step, soup M-step).  Per iteration a dict: the E-step's rows,
    `dense`, `counts`, `next_ambient`."""
    v, cb, e, v2snp, B = (problem[k] for k in ('v', 'cb', 'e', 'v2snp', 'B'))
    G = prob.shape[1]
    alpha, ambient = np.asarray(alpha, dtype=np.float32), np.asarray(ambient, dtype=np.float32)
    penalty = np.array([demux_oracle.doublet_penalties(len(d), doublet_prior)[-1] if len(d) > 1 else 0.0 for d in pools], dtype=np.float32)
    history = []
    for _it in range(n_iterations):
        rows = scoring.restate(v, cb, e, prob, B, pools, pool_of_barcode, penalty, doublet_prior != 0, alpha, ambient)
        dense = pooled.dense_singlets(rows, pools, pool_of_barcode, B, G)
        ambient, total = soup_update(v, cb, e, dense, prob, alpha, ambient, v2snp, pseudo_count, clip)
        history.append(dict(rows, dense=dense, counts=total, next_ambient=ambient))
    return history


learnt_betas = learning.learnt_betas


# ---- the seeded simulation of the recovery tests ------------------------------------------------------------------------------
SOUP_WEIGHTS = (8, 1, 1, 1, 1, 1, 1, 1)  # one lysed sample dominates the soup


def simulate(seed=0, soup_weights=SOUP_WEIGHTS, n_snps=600, n_barcodes=384, calls_per_barcode=256, true_alphas=(0.0, 0.2, 0.4), error=0.01):
    """ambient_restatement.simulate with one change: the soup is the donors' mix weighted by soup_weights (one weight per donor)
    and not their even mean.  The random draws are taken in that function's order.
    Returns dict(v, cb, e, prob, B, v2snp, donor1, donor2, truth, soup)."""
    weights = np.asarray(soup_weights, dtype=np.float64)
    n_donors = len(weights)
    rng = np.random.default_rng(seed)
    alt = rng.choice(np.array([0.01, 0.5, 0.99], dtype=np.float32), size=(n_snps, n_donors))
    prob = np.empty((2 * n_snps, n_donors), dtype=np.float32)
    prob[0::2] = np.float32(1) - alt
    prob[1::2] = alt
    soup = (prob.astype(np.float64) @ (weights / weights.sum())).astype(np.float32)
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    donor = np.arange(n_barcodes) % n_donors
    truth = np.asarray(true_alphas, dtype=np.float64)[np.arange(n_barcodes) % len(true_alphas)]
    vs, cbs = [], []
    for b in range(n_barcodes):
        snps = np.sort(rng.choice(n_snps, size=calls_per_barcode, replace=False))
        p_alt = (1 - truth[b]) * prob[2 * snps + 1, donor[b]] + truth[b] * soup[2 * snps + 1]
        is_alt = rng.random(calls_per_barcode) < p_alt
        wrong = rng.random(calls_per_barcode) < error
        vs.append(2 * snps + (is_alt ^ wrong))
        cbs.append(np.full(calls_per_barcode, b))
    v, cb = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32)
    order = np.lexsort((cb, v))
    v, cb = v[order], cb[order]
    e = np.full(len(v), error, dtype=np.float32)
    return dict(v=v, cb=cb, e=e, prob=prob, B=n_barcodes, v2snp=v2snp, donor1=donor.astype(np.int32),
                donor2=np.full(n_barcodes, -1, dtype=np.int32), truth=truth, soup=soup)


def profile_error(profile, sim):
    """Mean absolute error of a profile against the simulation's soup."""
    return float(np.abs(np.asarray(profile, dtype=np.float64) - sim['soup']).mean())


RECOVERY_BOUND = 0.8  # the learnt profile's error against the derived profile's


def recovery_condition(derived_error, learnt_error, what=''):
    """After the updates the learnt profile's mean absolute error is at most 0.8 of the derived profile's."""
    print(f'{what}mean |profile - soup|: derived {derived_error:.5f}, learnt {learnt_error:.5f}, ratio {learnt_error / derived_error:.3f}')
    assert learnt_error <= RECOVERY_BOUND * derived_error, (learnt_error, derived_error)


def recovery_run(seed, n_updates=3, clip=0.01):
    """(sim, the derived profile, learn_profile's history): the true table and the true fractions, soft posteriors from the restated
    E-step, n_updates soup updates starting from the derived profile."""
    sim = simulate(seed)
    B, G = sim['B'], sim['prob'].shape[1]
    derived = ambient_restatement.derived_ambient(sim['v'], sim['v2snp'], clip)
    problem = dict(v=sim['v'], cb=sim['cb'], e=sim['e'], v2snp=sim['v2snp'], B=B)
    history = learn_profile(problem, sim['prob'], [list(range(G))], np.zeros(B, np.int32), sim['truth'].astype(np.float32), derived, n_updates, clip,
                            0.)
    return sim, derived, history
