"""What the three-pass workflow (predict -> estimate the fraction under the best singlet -> re-score) does to TRUE
doublets, on the CPU restatement alone (tests/ambient_scoring_restatement.py, tests/ambient_restatement.py: numpy and the oracle,
float32 as the device computes; no GPU, no library).

    python scripts/ambient_doublet_absorption.py [--seed 0] [--calls 256]

The simulation is tests/ambient_restatement.simulate()'s - 8 donors, 600 biallelic SNPs, genotypes from {0.01, 0.5, 0.99}, the soup
the mean genotype, error 0.01, true fractions cycling 0 / 0.2 / 0.4 - with 48 true doublets (donors b % 8 and (b + 1 + b // 8) % 8 in
equal shares) behind its 96 singlets.  The fraction is estimated under the singlet hypothesis, so part of a doublet's second donor can
be absorbed as contamination: the table says how much, and what it costs."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def simulate(seed, calls_per_barcode, n_donors=8, n_snps=600, n_singlets=96, n_doublets=48, true_alphas=(0.0, 0.2, 0.4), error=0.01):
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


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--calls', type=int, default=256, help='calls per barcode')
    parser.add_argument('--doublet-prior', type=float, default=0.35)
    args = parser.parse_args()
    from tests import ambient_restatement as profile_restated
    from tests import ambient_scoring_restatement as restated
    sim = simulate(args.seed, args.calls)
    v, cb, e, prob, B = sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B']
    G = prob.shape[1]
    soup = profile_restated.derived_ambient(v, sim['v2snp'], 0.01)
    _l, _p, plain = restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, np.zeros(B, np.float32), soup)
    singlet = restated.best_singlets(plain['logits'].reshape(B, -1), G)
    estimate = profile_restated.restate(v, cb, e, prob, B, profile_restated.DEFAULT_GRID, singlet, np.full(B, -1), soup)
    fractions = profile_restated.DEFAULT_GRID[estimate['best']]
    _l, _p, rescored = restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, fractions, soup)
    _l, _p, oracle = restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, sim['truth'].astype(np.float32), soup)
    d1, d2 = restated.pool_options(list(range(G)), True)
    lo, hi = np.minimum(sim['first'], sim['second']), np.maximum(sim['first'], sim['second'])
    true_option = np.array([int(np.flatnonzero((d1 == a) & (d2 == b))[0]) if a >= 0 else int(b) for a, b in zip(lo, hi)])
    print(f'seed {args.seed}, {args.calls} calls per barcode, doublet_prior {args.doublet_prior}; "doublet": posterior pair mass > 0.5; "right": the arg-max is the true option')
    print(f'{"kind":<8} {"alpha":>5} {"n":>3} | {"plain":>17} | {"workflow":>17} | {"true alpha":>17} | estimated alpha: median (min .. max)')
    for kind, members in (('singlet', sim['second'] < 0), ('doublet', sim['second'] >= 0)):
        for level in (0.0, 0.2, 0.4):
            rows = members & (sim['truth'] == level)
            cells = [f'{int((out["doublet_mass"][rows] > 0.5).sum()):3d} doublet {int((out["best_option"][rows] == true_option[rows]).sum()):3d} right'
                     for out in (plain, rescored, oracle)]
            got = fractions[rows]
            print(f'{kind:<8} {level:5.1f} {int(rows.sum()):3d} | ' + ' | '.join(cells) + f' | {np.median(got):.2f} ({got.min():.2f} .. {got.max():.2f})')


if __name__ == '__main__':
    main()
