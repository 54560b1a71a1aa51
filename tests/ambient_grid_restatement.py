"""The pooled E-step with every option at its own best ambient fraction (include/demux_hip_debug.h: dmx_estep_ambient_grid;
Demultiplexer.predict_posteriors_joint_ambient) restated with numpy and the oracle, used as the checker by
tests/test_ambient_grid_cpu.py and tests/test_gpu_ambient_grid.py.

Nothing new is computed here: lambda[., j] is tests/ambient_scoring_restatement.restate with the fraction alphas[j] for every barcode,
once per grid value, stacked; an option's logit is the float32 first maximum over j (ties to the lower j, NaN never wins); the
posteriors are oracle.softmax_rows of those logits; rows, first arg-max and pair mass as tests/pools_restatement.py builds them.
Nothing here knows the library.

The second half is the seeded simulation with true doublets behind the singlets (scripts/ambient_doublet_absorption.py prints its
table from the same function) and the conditions the joint pass has to meet on it."""
import functools

import numpy as np

from oracle import demux_oracle
from tests import ambient_restatement
from tests import ambient_scoring_restatement as scoring

DEFAULT_GRID = ambient_restatement.DEFAULT_GRID


def restate(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, alphas, ambient):
    """dict(row_ptr, logits, probs, best_option, best_prob, doublet_mass, ambient, alpha_index, best_alpha_index, profile) as
    dmx_estep_ambient_grid defines them; profile float32[row_ptr[B], A]."""
    alphas = np.asarray(alphas, dtype=np.float32)
    assert alphas.ndim == 1 and len(alphas) >= 1
    pool_of_barcode = np.asarray(pool_of_barcode, dtype=np.int64)
    columns = [scoring.restate(v, cb, e, prob, B, pools, pool_of_barcode, pair_penalty, with_doublets, np.full(B, alpha, dtype=np.float32), ambient)
               for alpha in alphas]
    row_ptr = columns[0]['row_ptr']
    profile = np.stack([c['logits'] for c in columns], axis=1)
    assert profile.dtype == np.float32 and profile.shape == (int(row_ptr[-1]), len(alphas))
    alpha_index, logits = ambient_restatement.first_maximum(profile) if len(profile) else (np.zeros(0, np.int32), np.zeros(0, np.float32))
    probs = np.empty_like(logits)
    best_option = np.full(B, -1, dtype=np.int32)
    best_prob = np.full(B, np.nan, dtype=np.float32)
    doublet_mass = np.full(B, np.nan, dtype=np.float64)
    for p, donors in enumerate(pools):
        rows = np.flatnonzero(pool_of_barcode == p)
        if not len(rows):
            continue
        K = len(donors) * (len(donors) + 1) // 2 if with_doublets else len(donors)
        take = (row_ptr[rows][:, None] + np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
        P = demux_oracle.softmax_rows(logits[take].reshape(len(rows), K))
        probs[take] = P.reshape(-1)
        masked = np.where(np.isnan(P), -np.inf, P)  # the first maximum; NaN never wins
        first = masked.argmax(axis=1)
        some = ~np.isnan(P).all(axis=1)
        best_option[rows] = np.where(some, first, -1)
        best_prob[rows] = np.where(some, P[np.arange(len(rows)), first], np.nan)
        pairs = P[:, len(donors):].astype(np.float64)  # added one after the other in ascending option order (cumsum is sequential)
        doublet_mass[rows] = np.cumsum(pairs, axis=1)[:, -1] if pairs.shape[1] else 0.0
    found = best_option >= 0
    best_alpha_index = np.full(B, -1, dtype=np.int32)
    best_alpha_index[found] = alpha_index[row_ptr[:-1][found] + best_option[found]]
    return dict(row_ptr=row_ptr, logits=logits, probs=probs, best_option=best_option, best_prob=best_prob, doublet_mass=doublet_mass,
                ambient=np.asarray(ambient, dtype=np.float32), alpha_index=alpha_index, best_alpha_index=best_alpha_index, profile=profile)


def restate_all_donors(v, cb, e, prob, B, doublet_prior, alphas, ambient):
    """(logits, probs) [B, K] as predict_posteriors_joint_ambient returns them without pools, and the dict: one pool of every donor,
    the reference's penalties."""
    G = prob.shape[1]
    penalty = demux_oracle.doublet_penalties(G, doublet_prior)[-1] if G > 1 else 0.0
    out = restate(v, cb, e, prob, B, [list(range(G))], np.zeros(B, dtype=np.int32), np.array([penalty], dtype=np.float32), doublet_prior != 0,
                  alphas, ambient)
    return out['logits'].reshape(B, -1), out['probs'].reshape(B, -1), out


def assert_same(got, want, what):
    """Everything dmx_estep_ambient_grid returns, bit for bit; `got` may lack alpha_index / profile (not fetched)."""
    from tests import fixture_io as fio
    from tests import pools_restatement
    pools_restatement.assert_same(got, want, what)
    if got.get('ambient') is not None:
        fio.assert_bitwise(got['ambient'], want['ambient'], f'{what}: ambient_out')
    assert got['best_alpha_index'].dtype == np.int32 and np.array_equal(got['best_alpha_index'], want['best_alpha_index']), f'{what}: best_alpha_index'
    if got.get('alpha_index') is not None:
        assert got['alpha_index'].dtype == np.int32 and np.array_equal(got['alpha_index'], want['alpha_index']), f'{what}: alpha_index'
    if got.get('profile') is not None:
        fio.assert_bitwise(got['profile'], want['profile'], f'{what}: profile')


# ---- the seeded simulation with true doublets -----------------------------------------------------------------------------------
def simulate(seed, calls_per_barcode, n_donors=8, n_snps=600, n_singlets=96, n_doublets=48, true_alphas=(0.0, 0.2, 0.4), error=0.01):
    """tests/ambient_restatement.simulate()'s world - 8 donors, 600 biallelic SNPs, genotypes from {0.01, 0.5, 0.99}, the soup the mean
    genotype, error 0.01, true fractions cycling 0 / 0.2 / 0.4 - with 48 true doublets (donors b % 8 and (b + 1 + b // 8) % 8 in equal
    shares) behind its 96 singlets."""
    rng = np.random.default_rng(seed)
    alt = rng.choice(np.array([0.01, 0.5, 0.99], dtype=np.float32), size=(n_snps, n_donors))
    prob = np.empty((2 * n_snps, n_donors), dtype=np.float32)
    prob[0::2] = np.float32(1) - alt
    prob[1::2] = alt
    soup = prob.astype(np.float64).mean(axis=1).astype(np.float32)
    v2snp = np.repeat(np.arange(n_snps, dtype=np.int32), 2)
    B = n_singlets + n_doublets
    b = np.arange(B)
    first = b % n_donors
    second = np.where(b < n_singlets, -1, (first + 1 + (b // n_donors) % (n_donors - 1)) % n_donors)
    truth = np.asarray(true_alphas, dtype=np.float64)[b % len(true_alphas)]
    vs, cbs = [], []
    for i in range(B):
        snps = np.sort(rng.choice(n_snps, size=calls_per_barcode, replace=False))
        own = prob[2 * snps + 1, first[i]].astype(np.float64)
        if second[i] >= 0:
            own = 0.5 * (own + prob[2 * snps + 1, second[i]])
        p_alt = (1 - truth[i]) * own + truth[i] * soup[2 * snps + 1]
        is_alt = rng.random(calls_per_barcode) < p_alt
        wrong = rng.random(calls_per_barcode) < error
        vs.append(2 * snps + (is_alt ^ wrong))
        cbs.append(np.full(calls_per_barcode, i))
    v, cb = np.concatenate(vs).astype(np.int32), np.concatenate(cbs).astype(np.int32)
    order = np.lexsort((cb, v))
    v, cb = v[order], cb[order]
    return dict(v=v, cb=cb, e=np.full(len(v), error, dtype=np.float32), prob=prob, B=B, v2snp=v2snp, first=first, second=second, truth=truth,
                soup=soup)


def true_options(sim):
    """int[B]: the option column of every barcode's true donor or pair, in the all-donor list with doublets."""
    G = sim['prob'].shape[1]
    d1, d2 = scoring.pool_options(list(range(G)), True)
    lo, hi = np.minimum(sim['first'], sim['second']), np.maximum(sim['first'], sim['second'])
    return np.array([int(np.flatnonzero((d1 == a) & (d2 == b))[0]) if a >= 0 else int(b) for a, b in zip(lo, hi)])


@functools.lru_cache(maxsize=None)
def simulated(calls_per_barcode, seed=0, doublet_prior=0.35):
    """(sim, the joint pass restated on it: default grid, derived profile).  Computed once per shape, shared."""
    sim = simulate(seed, calls_per_barcode)
    soup = ambient_restatement.derived_ambient(sim['v'], sim['v2snp'], 0.01)
    _logits, _probs, out = restate_all_donors(sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B'], doublet_prior, DEFAULT_GRID, soup)
    return sim, out


def joint_counts(sim, doublet_mass, best_option, best_alpha):
    """What the conditions are about: dict(singlets_called_doublets, singlets_right, doublets_called (total), doublets_called_by_level,
    doublets_right_pair, clean_doublet_median_alpha).  "Doublet": pair mass above 0.5; best_alpha: the fraction at the winning option."""
    doublet_mass, best_option, best_alpha = np.asarray(doublet_mass), np.asarray(best_option), np.asarray(best_alpha, dtype=np.float64)
    singlet = sim['second'] < 0
    called = doublet_mass > 0.5
    right = best_option == true_options(sim)
    by_level = [int((called & ~singlet & (sim['truth'] == level)).sum()) for level in (0.0, 0.2, 0.4)]
    clean = ~singlet & (sim['truth'] == 0.0)
    return dict(singlets_called_doublets=int((called & singlet).sum()), singlets_right=int((right & singlet).sum()),
                doublets_called=int((called & ~singlet).sum()), doublets_called_by_level=by_level,
                doublets_right_pair=int((called & right & ~singlet).sum()), clean_doublet_median_alpha=float(np.median(best_alpha[clean])))


def joint_conditions(calls_per_barcode, sim, doublet_mass, best_option, best_alpha):
    """The conditions on seed 0, default grid, derived profile, doublet_prior 0.35 - conditions with slack, not measurements (measured on
    the CPU restatement in brackets).  256 calls: at most 2 of 96 singlets called doublets (0), at least 94 right (96), at least 38 of 48
    true doublets called doublets (42), median fraction at the winning option of the 16 clean doublets at most 0.1 (0.01).  64 calls:
    at least 20 of 48 true doublets called doublets (27; the three-pass workflow: 1).  Returns the counts."""
    assert sim['B'] == 144 and int((sim['second'] < 0).sum()) == 96
    counts = joint_counts(sim, doublet_mass, best_option, best_alpha)
    print(f'{calls_per_barcode} calls per barcode:', counts)
    if calls_per_barcode == 256:
        assert counts['singlets_called_doublets'] <= 2, counts
        assert counts['singlets_right'] >= 94, counts
        assert counts['doublets_called'] >= 38, counts
        assert counts['clean_doublet_median_alpha'] <= 0.1, counts
    elif calls_per_barcode == 64:
        assert counts['doublets_called'] >= 20, counts
    else:
        raise AssertionError('no conditions for this shape')
    return counts
