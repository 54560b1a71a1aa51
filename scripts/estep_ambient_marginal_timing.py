"""Times the pooled E-step with the grid of ambient fractions summed (DeviceContext.estep_ambient_grid(over_grid='marginal');
include/demux_hip_debug.h: dmx_estep_ambient_grid_marginal) next to the max pass (dmx_estep_ambient_grid) of the same
run: the same resident problem, the same pools, the same grid, the two passes taking turns.  Writes
profiles/estep_ambient_marginal.json.

    python scripts/estep_ambient_marginal_timing.py [--repeats 12] [--timeout 300] [--out profiles/estep_ambient_marginal.json]

Input and protocol are scripts/estep_ambient_grid_timing.py's: synth.generate(20_000, 20_000, 64); one pool of all 64 donors without
doublets (64 options: the one-slot form, 4 grid points per walk) and 2 pools of 32 donors with doublets (528 options: the 16-slot
form, 1 grid point per walk); grids of 8 and 64 values (0 .. 0.63 in equal steps); the profile supplied, nothing of size row_ptr[B]
downloaded; two warm-up repeats, then --repeats repeats; of each the library's own phase timer of the E-step slot (dmx_get_timings,
DMX_T_ESTEP: events around the launches) and the host clock around the call; medians of both.  Every variant (shape, grid) runs in a
child process of its own under its own time limit; this process never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM_UP = 2
B, S, G = 20_000, 20_000, 64
GRIDS = (8, 64)
SHAPES = ('singlets', 'doublets')
POINTS_PER_WALK = {'singlets': 4, 'doublets': 1}  # csrc/estep_grid_device.h: GridPoints of the form each shape runs
PARENT_MAX_MS = {('singlets', 8): 2.005, ('singlets', 64): 15.148, ('doublets', 8): 28.286, ('doublets', 64): 223.020}  # DESIGN.md 4.8's table


def run_variant(shape, n_alphas, repeats):
    import numpy as np
    from demuxalot_amd import synth
    from demuxalot_amd.device import DeviceContext
    p = synth.generate(B, S, G)
    ctx = DeviceContext(0)
    try:
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_betas(p.prior_betas(add_data_prior=False))
        ctx.set_addition(None)
        ctx.probs_from_betas(0.01, fetch=False)
        calls_per_barcode = np.bincount(p.compressed_cb, minlength=B)
        padded_calls = int(((calls_per_barcode + 7) // 8 * 8).sum())
        rows = np.arange(B)
        singlets = ([list(range(G))], np.zeros(B, np.int32), False, np.zeros(1, np.float32))
        options, pools = {
            'singlets': (64, singlets),
            'doublets': (528, ([list(range(0, 32)), list(range(32, 64))], (rows % 2).astype(np.int32), True, np.array([-0.5, -0.5], np.float32))),
        }[shape]
        lean = dict(fetch_logits=False, fetch_probs=False, fetch_alpha_index=False)
        soup = ctx.estep_ambient(*singlets, np.zeros(B, np.float32), fetch_logits=False, fetch_probs=False)['ambient']
        grid = np.linspace(0, 0.63, n_alphas, dtype=np.float32)
        weights = np.linspace(0, -2, n_alphas, dtype=np.float32)
        ctx.set_phase_timers(True)
        calls = {
            'max': lambda: ctx.estep_ambient_grid(*pools, grid, ambient=soup, **lean),
            'marginal': lambda: ctx.estep_ambient_grid(*pools, grid, ambient=soup, over_grid='marginal', fetch_alpha_mean=False, **lean),
            'marginal_prior': lambda: ctx.estep_ambient_grid(*pools, grid, ambient=soup, over_grid='marginal', log_weights=weights,
                                                             fetch_alpha_mean=False, **lean),
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
        return [dict(step=step, shape=shape, options=options, n_alphas=n_alphas, points_per_walk=POINTS_PER_WALK[shape], barcodes=B,
                     calls=int(p.n_calls), padded_calls=padded_calls, terms=options * padded_calls * n_alphas,
                     pass_ms_median=statistics.median(phase[step]), pass_ms_min=min(phase[step]), pass_ms_max=max(phase[step]), pass_ms=phase[step],
                     call_ms_median=statistics.median(host[step]), call_ms=host[step], repeats=repeats, warm_up=WARM_UP) for step in calls]
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--timeout', type=float, default=300.0, help='seconds one variant\'s process may take')
    parser.add_argument('--run', nargs=2, metavar=('SHAPE', 'N_ALPHAS'), help='(internal) measure one variant and print the JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'estep_ambient_marginal.json'))
    args = parser.parse_args()
    if args.run:
        print('RESULT ' + json.dumps(run_variant(args.run[0], int(args.run[1]), args.repeats)), flush=True)
        return
    results = []
    for shape in SHAPES:
        for n_alphas in GRIDS:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--run', shape, str(n_alphas), '--repeats', str(args.repeats)],
                                  capture_output=True, text=True, timeout=args.timeout)
            if done.returncode != 0:  # (nothing more is started on the GPU after a variant that did not end well)
                sys.stderr.write(done.stdout + done.stderr)
                raise SystemExit(f'{shape} x {n_alphas}: the measurement ended with status {done.returncode}')
            rows = json.loads(next(line for line in done.stdout.splitlines() if line.startswith('RESULT '))[len('RESULT '):])
            against = next(row for row in rows if row['step'] == 'max')
            for row in rows:
                row['ratio_to_max_of_the_same_run'] = row['pass_ms_median'] / against['pass_ms_median']
                row['parent_max_ms'] = PARENT_MAX_MS[(shape, n_alphas)]
                print(f'{row["step"]:<14} {shape:<9} {n_alphas:2d} grid values  pass median {row["pass_ms_median"]:9.3f} ms '
                      f'(min {row["pass_ms_min"]:.3f}, max {row["pass_ms_max"]:.3f})  call {row["call_ms_median"]:9.3f} ms  '
                      f'{row["terms"] / row["pass_ms_median"] / 1e6:7.1f} G terms/s  x{row["ratio_to_max_of_the_same_run"]:.3f} of the max pass '
                      f'(the max pass before this mode existed: {row["parent_max_ms"]:.3f} ms)', flush=True)
            results += rows
    result = dict(input=f'synth.generate({B}, {S}, {G})', grids='0 .. 0.63 in equal steps, 8 and 64 values',
                  clock='dmx_get_timings, DMX_T_ESTEP (pass_ms); host clock around the call and a synchronise (call_ms)',
                  steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
