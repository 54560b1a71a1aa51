"""What the three-pass workflow (predict -> estimate the fraction under the best singlet -> re-score) does to TRUE
doublets, on the CPU restatement alone (tests/ambient_scoring_restatement.py, tests/ambient_restatement.py: numpy and the oracle,
float32 as the device computes; no GPU, no library).

    python scripts/ambient_doublet_absorption.py [--seed 0] [--calls 256]

The simulation is tests/ambient_restatement.simulate()'s - 8 donors, 600 biallelic SNPs, genotypes from {0.01, 0.5, 0.99}, the soup
the mean genotype, error 0.01, true fractions cycling 0 / 0.2 / 0.4 - with 48 true doublets (donors b % 8 and (b + 1 + b // 8) % 8 in
equal shares) behind its 96 singlets.  The fraction is estimated under the singlet hypothesis, so part of a doublet's second donor can
be absorbed as contamination: the table says how much, and what it costs.  The last columns are the joint pass (DESIGN.md 4.8;
tests/ambient_grid_restatement.py, which also holds the simulation): every option, singlets and pairs, at its own best fraction."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--calls', type=int, default=256, help='calls per barcode')
    parser.add_argument('--doublet-prior', type=float, default=0.35)
    args = parser.parse_args()
    from tests import ambient_grid_restatement as joint_restated
    from tests import ambient_restatement as profile_restated
    from tests import ambient_scoring_restatement as restated
    sim = joint_restated.simulate(args.seed, args.calls)  # (the simulation lives with the restatement the tests use)
    v, cb, e, prob, B = sim['v'], sim['cb'], sim['e'], sim['prob'], sim['B']
    G = prob.shape[1]
    soup = profile_restated.derived_ambient(v, sim['v2snp'], 0.01)
    _l, _p, plain = restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, np.zeros(B, np.float32), soup)
    singlet = restated.best_singlets(plain['logits'].reshape(B, -1), G)
    estimate = profile_restated.restate(v, cb, e, prob, B, profile_restated.DEFAULT_GRID, singlet, np.full(B, -1), soup)
    fractions = profile_restated.DEFAULT_GRID[estimate['best']]
    _l, _p, rescored = restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, fractions, soup)
    _l, _p, oracle = restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, sim['truth'].astype(np.float32), soup)
    # every option at its own best fraction of the grid, one softmax: no assignment step in between
    _l, _p, joint = joint_restated.restate_all_donors(v, cb, e, prob, B, args.doublet_prior, profile_restated.DEFAULT_GRID, soup)
    joint_fractions = np.where(joint['best_alpha_index'] >= 0, profile_restated.DEFAULT_GRID[np.maximum(joint['best_alpha_index'], 0)], np.nan)
    d1, d2 = restated.pool_options(list(range(G)), True)
    lo, hi = np.minimum(sim['first'], sim['second']), np.maximum(sim['first'], sim['second'])
    true_option = np.array([int(np.flatnonzero((d1 == a) & (d2 == b))[0]) if a >= 0 else int(b) for a, b in zip(lo, hi)])
    print(f'seed {args.seed}, {args.calls} calls per barcode, doublet_prior {args.doublet_prior}; "doublet": posterior pair mass > 0.5; "right": the arg-max is the true option')
    print(f'{"kind":<8} {"alpha":>5} {"n":>3} | {"plain":>17} | {"workflow":>17} | {"true alpha":>17} | {"joint":>17} | estimated alpha: median (min .. max) | joint, at the winning option')
    for kind, members in (('singlet', sim['second'] < 0), ('doublet', sim['second'] >= 0)):
        for level in (0.0, 0.2, 0.4):
            rows = members & (sim['truth'] == level)
            cells = [f'{int((out["doublet_mass"][rows] > 0.5).sum()):3d} doublet {int((out["best_option"][rows] == true_option[rows]).sum()):3d} right'
                     for out in (plain, rescored, oracle, joint)]
            got, at_winner = fractions[rows], joint_fractions[rows]
            print(f'{kind:<8} {level:5.1f} {int(rows.sum()):3d} | ' + ' | '.join(cells) + f' | {np.median(got):.2f} ({got.min():.2f} .. {got.max():.2f})'
                  f' | {np.nanmedian(at_winner):.2f} ({np.nanmin(at_winner):.2f} .. {np.nanmax(at_winner):.2f})')


if __name__ == '__main__':
    main()
