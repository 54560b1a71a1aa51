"""Times the pooled E-step with every option at its own best ambient fraction (DeviceContext.estep_ambient_grid;
include/demux_hip_debug.h: dmx_estep_ambient_grid) next to its yardstick: what the library offered for the same
result before - one call of the pooled E-step under per-barcode fractions (dmx_estep_ambient) per grid value, with that value for every
barcode, on the same pools - on the same resident problem in the same process.  Writes profiles/estep_ambient_grid.json.

    python scripts/estep_ambient_grid_timing.py [--repeats 12] [--timeout 600] [--out profiles/estep_ambient_grid.json]

Input: synth.generate(20_000, 20_000, 64).  Two pool shapes - one pool of all 64 donors without doublets (64 options: the one-slot
form, 4 grid points per walk), every barcode in one of 2 pools of 32 donors with doublets (528 options: the 16-slot form, 1 grid point
per walk) - and grids of 8 and 64 values (0 .. 0.63 in equal steps).  Steps, all in ONE child process under one time limit (this
process never opens the GPU); per shape and grid:
    grid       dmx_estep_ambient_grid, the profile supplied, nothing of size row_ptr[B] downloaded
    repeated   n_alphas calls of dmx_estep_ambient with alpha = alphas[j] for every barcode, the same profile supplied; the time of
               a repeat is the SUM of the n_alphas pass times
Per step: two warm-up repeats, then --repeats repeats; of each the library's own phase timer of the E-step slot (dmx_get_timings,
DMX_T_ESTEP: events around the launches; uploads and downloads outside) and the host clock around the calls; medians of both."""
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
POINTS_PER_WALK = {'singlets': 4, 'doublets': 1}  # csrc/estep_grid_device.h: GridPoints of the form each shape runs


def run_steps(repeats):
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
        shapes = {
            'singlets': (64, ([list(range(G))], np.zeros(B, np.int32), False, np.zeros(1, np.float32))),
            'doublets': (528, ([list(range(0, 32)), list(range(32, 64))], (rows % 2).astype(np.int32), True, np.array([-0.5, -0.5], np.float32))),
        }
        lean = dict(fetch_logits=False, fetch_probs=False)
        soup = ctx.estep_ambient(*shapes['singlets'][1], np.zeros(B, np.float32), **lean)['ambient']
        ctx.set_phase_timers(True)
        results = []

        def pass_ms(call, expected_launches):
            ctx.reset_timings()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            estep = ctx.timings()['estep']
            assert estep['launches'] == expected_launches, estep
            return estep['ms'], host

        for shape, (options, pools) in shapes.items():
            for n_alphas in GRIDS:
                grid = np.linspace(0, 0.63, n_alphas, dtype=np.float32)
                constant = [np.full(B, value, np.float32) for value in grid]

                def fused():
                    ctx.estep_ambient_grid(*pools, grid, ambient=soup, fetch_alpha_index=False, **lean)

                def repeated():
                    for alpha in constant:
                        ctx.estep_ambient(*pools, alpha, ambient=soup, **lean)

                for step, call, launches in (('grid', fused, 1), ('repeated', repeated, n_alphas)):
                    phase, host = [], []
                    for i in range(WARM_UP + repeats):
                        ms, wall = pass_ms(call, launches)
                        if i >= WARM_UP:
                            phase.append(ms)
                            host.append(wall)
                    results.append(dict(step=step, shape=shape, options=options, n_alphas=n_alphas, points_per_walk=POINTS_PER_WALK[shape],
                                        barcodes=B, calls=int(p.n_calls), padded_calls=padded_calls, terms=options * padded_calls * n_alphas,
                                        pass_ms_median=statistics.median(phase), pass_ms_min=min(phase), pass_ms_max=max(phase), pass_ms=phase,
                                        call_ms_median=statistics.median(host), call_ms=host, repeats=repeats, warm_up=WARM_UP))
        return results
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--timeout', type=float, default=600.0, help='seconds the measuring process may take')
    parser.add_argument('--run', action='store_true', help='(internal) measure and print the JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'estep_ambient_grid.json'))
    args = parser.parse_args()
    if args.run:
        print('RESULT ' + json.dumps(run_steps(args.repeats)), flush=True)
        return
    done = subprocess.run([sys.executable, os.path.abspath(__file__), '--run', '--repeats', str(args.repeats)], capture_output=True, text=True,
                          timeout=args.timeout)
    if done.returncode != 0:
        sys.stderr.write(done.stdout + done.stderr)
        raise SystemExit(f'the measurement ended with status {done.returncode}')
    results = json.loads(next(line for line in done.stdout.splitlines() if line.startswith('RESULT '))[len('RESULT '):])
    medians = {(row['step'], row['shape'], row['n_alphas']): row['pass_ms_median'] for row in results}
    for row in results:
        against = medians[('repeated', row['shape'], row['n_alphas'])]
        row['yardstick'] = 'repeated'
        row['ratio_to_yardstick'] = row['pass_ms_median'] / against
        print(f'{row["step"]:<9} {row["shape"]:<9} {row["n_alphas"]:2d} grid values  pass median {row["pass_ms_median"]:9.3f} ms '
              f'(min {row["pass_ms_min"]:.3f}, max {row["pass_ms_max"]:.3f})  call {row["call_ms_median"]:9.3f} ms  '
              f'{row["terms"] / row["pass_ms_median"] / 1e6:7.1f} G terms/s  x{row["ratio_to_yardstick"]:.3f} of the repeated passes', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G})', grids='0 .. 0.63 in equal steps, 8 and 64 values',
                  clock='dmx_get_timings, DMX_T_ESTEP (pass_ms; for "repeated" the sum over the grid); host clock around the calls and a synchronise (call_ms)',
                  steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)
    slower = [row for row in results if row['step'] == 'grid' and row['ratio_to_yardstick'] > 1.0]
    if slower:
        raise SystemExit('the fused pass is slower than the repeated passes on: ' + ', '.join(f'{r["shape"]} x {r["n_alphas"]}' for r in slower))


if __name__ == '__main__':
    main()
