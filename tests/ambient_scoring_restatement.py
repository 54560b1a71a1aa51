"""The pooled E-step under per-barcode ambient fractions (include/demux_hip_debug.h: dmx_estep_ambient;
Demultiplexer.predict_posteriors_with_ambient / predict_posteriors_decontaminated) restated with numpy and the oracle, used as the
checker by tests/test_ambient_scoring_cpu.py and tests/test_gpu_ambient_scoring.py.

For barcode b of pool p and option k = (d) or (d1, d2) of that pool, all in float32, every operation rounded:
    q = prob[v, d]   or   (prob[v, d1] + prob[v, d2]) * 0.5
    m = q * (1 - alpha[b]) + ambient[v] * alpha[b]
    logit[b, k] = f32( f64(pen) + sum over the calls of b, in their stored order, of f64( log(m * (1 - e) + max(e, 1e-4)) ) )
with oracle.log_f32 for the log and np.bincount(cb, weights=t) for the ordered float64 sum - the reference's own barcode_logits
(demux.py:246-265) with the mixture in place of the genotype's term - and oracle.softmax_rows for the posteriors.  Rows, first
arg-max and pair mass as tests/pools_restatement.py builds them.  Nothing here knows the library."""
import functools

import numpy as np

from oracle import demux_oracle
from tests import ambient_restatement


def pool_options(donors, with_doublets):
    """(d1, d2) per option of the genotype list `donors` (table columns): the singlets (d, d) in list order, then the pairs i < j, i-major."""
    g1, g2 = demux_oracle.option_pairs(len(donors), 1 if with_doublets else 0)
    donors = np.asarray(donors, dtype=np.int64)
    return donors[g1], donors[g2]


def restate(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, alpha, ambient):
    """dict(row_ptr, logits, probs, best_option, best_prob, doublet_mass, ambient) as dmx_estep_ambient defines them."""
    v, cb = np.asarray(v), np.asarray(cb)
    e = np.asarray(e, dtype=np.float32)
    prob = np.asarray(prob, dtype=np.float32)
    alpha = np.asarray(alpha, dtype=np.float32)
    ambient = np.asarray(ambient, dtype=np.float32)
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int64)
    pair_penalty = np.asarray(pair_penalty, dtype=np.float32)
    assert alpha.shape == (B,) and pool_of_barcode.shape == (B,) and ambient.shape == (prob.shape[0],) and pair_penalty.shape == (len(pools),)
    keep = 1 - e
    floor = e.clip(1e-4)
    assert keep.dtype == np.float32 and floor.dtype == np.float32
    widths = np.array([len(d) * (len(d) + 1) // 2 if with_doublets else len(d) for d in pools] + [0], dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(widths[pool_of_barcode])]).astype(np.int64)
    logits = np.empty(int(row_ptr[-1]), dtype=np.float32)
    probs = np.empty(int(row_ptr[-1]), dtype=np.float32)
    best_option = np.full(B, -1, dtype=np.int32)
    best_prob = np.full(B, np.nan, dtype=np.float32)
    doublet_mass = np.full(B, np.nan, dtype=np.float64)
    w0 = np.float32(1) - alpha
    for p, donors in enumerate(pools):
        rows = np.flatnonzero(pool_of_barcode == p)
        if not len(rows):
            continue
        mine = np.isin(cb, rows)  # (boolean selection keeps the stored order)
        vs, cbs, ks, fs = v[mine], cb[mine], keep[mine], floor[mine]
        soup_term = ambient[vs] * alpha[cbs]
        own_weight = w0[cbs]
        d1, d2 = pool_options(donors, with_doublets)
        K = len(d1)
        L = np.empty((len(rows), K), dtype=np.float32)
        for k, (a, b) in enumerate(zip(d1, d2)):
            col = prob[:, a] if a == b else (prob[:, a] + prob[:, b]) * np.float32(0.5)
            m = col[vs] * own_weight + soup_term
            t = demux_oracle.log_f32(m * ks + fs)
            assert m.dtype == np.float32 and t.dtype == np.float32
            sums = np.bincount(cbs, weights=t, minlength=B)  # float64, in the order of the calls
            pen = np.float64(0 if a == b else pair_penalty[p])
            L[:, k] = (pen + sums[rows]).astype(np.float32)
        P = demux_oracle.softmax_rows(L)
        take = (row_ptr[rows][:, None] + np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
        logits[take] = L.reshape(-1)
        probs[take] = P.reshape(-1)
        masked = np.where(np.isnan(P), -np.inf, P)  # the first maximum; NaN never wins
        first = masked.argmax(axis=1)
        some = ~np.isnan(P).all(axis=1)
        best_option[rows] = np.where(some, first, -1)
        best_prob[rows] = np.where(some, P[np.arange(len(rows)), first], np.nan)
        pairs = P[:, len(donors):].astype(np.float64)  # added one after the other in ascending option order (cumsum is sequential)
        doublet_mass[rows] = np.cumsum(pairs, axis=1)[:, -1] if pairs.shape[1] else 0.0
    return dict(row_ptr=row_ptr, logits=logits, probs=probs, best_option=best_option, best_prob=best_prob, doublet_mass=doublet_mass,
                ambient=ambient)


def restate_all_donors(v, cb, e, prob, B, doublet_prior, alpha, ambient):
    """(logits, probs) [B, K] as predict_posteriors_with_ambient returns them without pools: one pool of every donor, the
    reference's penalties."""
    G = prob.shape[1]
    penalty = demux_oracle.doublet_penalties(G, doublet_prior)[-1] if G > 1 else 0.0
    out = restate(v, cb, e, prob, B, [list(range(G))], np.zeros(B, dtype=np.int32), np.array([penalty], dtype=np.float32), doublet_prior != 0,
                  alpha, ambient)
    return out['logits'].reshape(B, -1), out['probs'].reshape(B, -1), out


def best_singlets(logits, G):
    """The first maximum over the singlet columns of the plain logits (the donors' log-likelihoods: their penalty is 0)."""
    return np.asarray(logits)[:, :G].argmax(axis=1)


# ---- the three-pass workflow on the seeded simulation ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def workflow(doublet_prior=0.35):
    """ambient_restatement.simulate() with its defaults through predict -> estimate -> re-score, all restated: dict(sim, plain_logits,
    plain_probs, plain (the pooled dict), singlet, estimate (ambient_restatement.restate's dict), fractions, logits, probs, rescored).
    The soup is the derived profile, as the library's workflow has it for ambient=None.  Computed once, shared."""
    sim, _ = ambient_restatement.simulated()
    v, cb, e, prob, B = sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B']
    G = prob.shape[1]
    soup = ambient_restatement.derived_ambient(v, sim['v2snp'], 0.01)
    plain_logits, plain_probs, plain = restate_all_donors(v, cb, e, prob, B, doublet_prior, np.zeros(B, np.float32), soup)
    singlet = best_singlets(plain_logits, G)
    estimate = ambient_restatement.restate(v, cb, e, prob, B, ambient_restatement.DEFAULT_GRID, singlet, np.full(B, -1), soup)
    fractions = ambient_restatement.DEFAULT_GRID[estimate['best']]
    logits, probs, rescored = restate_all_donors(v, cb, e, prob, B, doublet_prior, fractions, soup)
    return dict(sim=sim, soup=soup, plain_logits=plain_logits, plain_probs=plain_probs, plain=plain, singlet=singlet, estimate=estimate,
                fractions=fractions, logits=logits, probs=probs, rescored=rescored)


def workflow_conditions(sim, plain_doublet_mass, doublet_mass, best_option):
    """The three conditions on the simulation: plain scoring calls at least 24 of the 32 barcodes with alpha = 0.4 doublets (mass above
    0.5); after the workflow at most 2 of the 96 are, and at least 94 have the true donor as arg-max.  Returns the three counts."""
    heavy = sim['truth'] == 0.4
    assert heavy.sum() == 32 and sim['B'] == 96
    plain_doublets = int((np.asarray(plain_doublet_mass)[heavy] > 0.5).sum())
    doublets = int((np.asarray(doublet_mass) > 0.5).sum())
    right = int((np.asarray(best_option) == sim['donor1']).sum())
    print(f'plain: {plain_doublets} of the 32 barcodes with alpha = 0.4 called doublets; after the workflow: {doublets} of 96 called doublets, '
          f'{right} of 96 with the true donor as arg-max')
    assert plain_doublets >= 24, plain_doublets
    assert doublets <= 2, doublets
    assert right >= 94, right
    return plain_doublets, doublets, right
