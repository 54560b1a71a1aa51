"""Times the pooled E-step with every pair option summed over a grid of mixing shares (DeviceContext.estep_pair_shares;
include/demux_hip_debug.h: dmx_estep_pair_shares) next to two passes this one does not touch, in the same process: the
pooled pass (dmx_estep_pools) on the same pools - n_shares of them are what the grid would cost one share at a time - and the ambient
marginal pass (dmx_estep_ambient_grid_marginal) at the same grid length.  Merges its rows into profiles/estep_pair_shares.json.

One invocation measures one variant (shape, grid length); every variant runs in a process of its own under a time limit of its own,
and nothing more is started after one that did not end well:

    timeout -k 10 300 python scripts/estep_pair_shares_timing.py one_slot 9 &&
    timeout -k 10 300 python scripts/estep_pair_shares_timing.py two_slot 9 &&
    timeout -k 10 300 python scripts/estep_pair_shares_timing.py wide 9 &&
    timeout -k 10 300 python scripts/estep_pair_shares_timing.py wide 64

Input and protocol are DESIGN.md 4.8's: synth.generate(20_000, 20_000, 64, doublets=True); 'one_slot': 8 pools of 8 donors with
doublets (36 options: the one-slot form, 4 grid points per walk), 'two_slot': 5 pools of 11 of the donors with doublets (66 options: the
two-slot form, 2 grid points per walk), 'wide': 2 pools of 32 donors with doublets (528 options: the 16-slot form, 1 grid point per
walk); shares 0.1 .. 0.9 in equal steps under the uniform prior; nothing of size row_ptr[B] downloaded; two
warm-up repeats, then --repeats repeats, the passes taking turns; of each the library's own phase timer of the E-step slot
(dmx_get_timings, DMX_T_ESTEP: events around the launches) and the host clock around the call; medians of both."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM_UP = 2
B, S, G = 20_000, 20_000, 64
SHAPES = {'one_slot': (8, 8, 36, 4), 'two_slot': (5, 11, 66, 2), 'wide': (2, 32, 528, 1)}  # pools, donors per pool, options, grid points per walk


def run_variant(shape, n_shares, repeats):
    import numpy as np
    from demuxalot_amd import synth
    from demuxalot_amd.device import DeviceContext
    n_pools, per_pool, options, points_per_walk = SHAPES[shape]
    assert per_pool * (per_pool + 1) // 2 == options and n_pools * per_pool <= G
    p = synth.generate(B, S, G, doublets=True)
    ctx = DeviceContext(0)
    try:
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_betas(p.prior_betas(add_data_prior=False))
        ctx.set_addition(None)
        ctx.probs_from_betas(0.01, fetch=False)
        calls_per_barcode = np.bincount(p.compressed_cb, minlength=B)
        padded_calls = int(((calls_per_barcode + 7) // 8 * 8).sum())
        pools = ([list(range(i * per_pool, (i + 1) * per_pool)) for i in range(n_pools)], (np.arange(B) % n_pools).astype(np.int32), True,
                 np.full(n_pools, -0.5, np.float32))
        everybody = ([list(range(G))], np.zeros(B, np.int32), False, np.zeros(1, np.float32))
        soup = ctx.estep_ambient(*everybody, np.zeros(B, np.float32), fetch_logits=False, fetch_probs=False)['ambient']
        shares = np.linspace(0.1, 0.9, n_shares, dtype=np.float32)
        weights = np.full(n_shares, np.float32(-np.log(n_shares)), np.float32)
        alphas = np.linspace(0, 0.63, n_shares, dtype=np.float32)
        ctx.set_phase_timers(True)
        calls = {
            'pair_shares': lambda: ctx.estep_pair_shares(*pools, shares, log_weights=weights, fetch_logits=False, fetch_probs=False,
                                                         fetch_share_index=False, fetch_share_mean=False),
            'pools': lambda: ctx.estep_pools(*pools, fetch_logits=False, fetch_probs=False),
            'ambient_marginal': lambda: ctx.estep_ambient_grid(*pools, alphas, ambient=soup, over_grid='marginal', log_weights=weights,
                                                               fetch_logits=False, fetch_probs=False, fetch_alpha_index=False, fetch_alpha_mean=False),
        }
        phase, host = {step: [] for step in calls}, {step: [] for step in calls}
        for i in range(WARM_UP + repeats):
            for step, call in calls.items():  # the passes take turns: what drifts during a run drifts for all of them
                ctx.reset_timings()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                estep = ctx.timings()['estep']
                assert estep['launches'] == 1, estep
                if i >= WARM_UP:
                    phase[step].append(estep['ms'])
                    host[step].append(wall)
        rows = [dict(step=step, shape=shape, pools=n_pools, options=options, n_shares=n_shares, points_per_walk=points_per_walk, barcodes=B,
                     calls=int(p.n_calls), padded_calls=padded_calls, pass_ms_median=statistics.median(phase[step]), pass_ms_min=min(phase[step]),
                     pass_ms_max=max(phase[step]), pass_ms=phase[step], call_ms_median=statistics.median(host[step]), call_ms=host[step],
                     repeats=repeats, warm_up=WARM_UP) for step in calls]
        fused, pooled, ambient = (next(row for row in rows if row['step'] == step) for step in ('pair_shares', 'pools', 'ambient_marginal'))
        fused['n_shares_pooled_passes_ms'] = n_shares * pooled['pass_ms_median']
        fused['ratio_to_n_shares_pooled_passes'] = fused['pass_ms_median'] / fused['n_shares_pooled_passes_ms']
        fused['ratio_to_ambient_marginal'] = fused['pass_ms_median'] / ambient['pass_ms_median']
        return rows
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('shape', choices=sorted(SHAPES))
    parser.add_argument('n_shares', type=int)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'estep_pair_shares.json'))
    args = parser.parse_args()
    rows = run_variant(args.shape, args.n_shares, args.repeats)
    for row in rows:
        print(f'{row["step"]:<17} {args.shape:<8} {args.n_shares:2d} shares  pass median {row["pass_ms_median"]:9.3f} ms '
              f'(min {row["pass_ms_min"]:.3f}, max {row["pass_ms_max"]:.3f})  call {row["call_ms_median"]:9.3f} ms', flush=True)
    fused = rows[0]
    print(f'the fused pass: x{fused["ratio_to_n_shares_pooled_passes"]:.3f} of {args.n_shares} pooled passes '
          f'({fused["n_shares_pooled_passes_ms"]:.3f} ms), x{fused["ratio_to_ambient_marginal"]:.3f} of the ambient marginal pass', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G}, doublets=True)', grids='shares 0.1 .. 0.9 in equal steps under the uniform prior',
                  clock='dmx_get_timings, DMX_T_ESTEP (pass_ms); host clock around the call and a synchronise (call_ms)', steps=[])
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result['steps'] = [row for row in result['steps'] if (row['shape'], row['n_shares']) != (args.shape, args.n_shares)] + rows
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
