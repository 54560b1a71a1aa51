"""Times the ambient-fraction pass (DeviceContext.ambient_profile; include/demux_hip_debug.h: dmx_ambient_profile) next to its
yardstick, the exact singlet E-step (dmx_estep) on the same resident problem in the same process.  Writes profiles/ambient_profile.json.

    python scripts/ambient_profile_timing.py [--repeats 12] [--timeout 300] [--out profiles/ambient_profile.json]

Input: synth.generate(20_000, 20_000, 64); a grid of 64 values.  Both passes walk every padded call of every barcode once with
64 lanes: the E-step a donor per lane, this pass a grid value per lane - the same number of terms, calls x 64, and the same
arithmetic per term plus the mixture (two products and a sum).  Steps, all in ONE child process under one time limit (this process
never opens the GPU):
    ambient_singlets   every barcode assigned a singlet (donor b % 64), the profile derived from the calls, [B, 64] not downloaded
    ambient_pairs      every barcode assigned a pair
    ambient_supplied   singlets, the profile supplied by the caller (no counting, no normalisation)
    ambient_fetched    singlets with the [B, 64] profile downloaded (the host clock only differs)
    estep_exact        dmx_estep, DMX_ESTEP_EXACT, without doublets (K = 64), nothing downloaded
Per step: two warm-up calls, then --repeats calls; of each call the library's own phase timer of the E-step slot (dmx_get_timings,
DMX_T_ESTEP: events around the launch; uploads, the profile's derivation and downloads outside) and the host clock around the
whole call; medians of both."""
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
B, S, G, A = 20_000, 20_000, 64, 64
STEPS = ('ambient_singlets', 'ambient_pairs', 'ambient_supplied', 'ambient_fetched', 'estep_exact')


def run_steps(repeats):
    import numpy as np
    from demuxalot_amd import synth
    from demuxalot_amd.device import DeviceContext
    p = synth.generate(B, S, G)
    ctx = DeviceContext(0)
    try:
        ctx.set_estep_mode('exact')
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_betas(p.prior_betas(add_data_prior=False))
        ctx.set_addition(None)
        ctx.probs_from_betas(0.01, fetch=False)
        calls_per_barcode = np.bincount(p.compressed_cb, minlength=B)
        padded_calls = int(((calls_per_barcode + 7) // 8 * 8).sum())
        rows = np.arange(B)
        singlets = (rows % G).astype(np.int32), np.full(B, -1, np.int32)
        pairs = (rows % (G - 1)).astype(np.int32), (rows % (G - 1) + 1).astype(np.int32)
        alphas = np.linspace(0, 0.63, A, dtype=np.float32)
        soup = ctx.ambient_profile(*singlets, alphas, fetch_profile=False)['ambient']
        penalties = np.zeros(G, dtype=np.float32)
        calls = {
            'ambient_singlets': lambda: ctx.ambient_profile(*singlets, alphas, fetch_profile=False),
            'ambient_pairs': lambda: ctx.ambient_profile(*pairs, alphas, fetch_profile=False),
            'ambient_supplied': lambda: ctx.ambient_profile(*singlets, alphas, ambient=soup, fetch_profile=False),
            'ambient_fetched': lambda: ctx.ambient_profile(*singlets, alphas, fetch_profile=True),
            'estep_exact': lambda: ctx.estep(penalties, with_doublets=False, fetch_logits=False, fetch_probs=False),
        }
        ctx.set_phase_timers(True)
        results = []
        for step in STEPS:
            phase_ms, call_ms = [], []
            for i in range(WARM_UP + repeats):
                ctx.reset_timings()
                t0 = time.perf_counter()
                calls[step]()
                ctx.synchronize()
                host = (time.perf_counter() - t0) * 1e3
                estep = ctx.timings()['estep']
                assert estep['launches'] == 1, estep
                if i >= WARM_UP:
                    phase_ms.append(estep['ms'])
                    call_ms.append(host)
            results.append(dict(step=step, lanes=64, barcodes=B, calls=int(p.n_calls), padded_calls=padded_calls, terms=64 * padded_calls,
                                pass_ms_median=statistics.median(phase_ms), pass_ms_min=min(phase_ms), pass_ms_max=max(phase_ms), pass_ms=phase_ms,
                                call_ms_median=statistics.median(call_ms), call_ms=call_ms, repeats=repeats, warm_up=WARM_UP))
        return results
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--timeout', type=float, default=300.0, help='seconds the measuring process may take')
    parser.add_argument('--run', action='store_true', help='(internal) measure and print the JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ambient_profile.json'))
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
    yardstick = next(row for row in results if row['step'] == 'estep_exact')['pass_ms_median']
    for row in results:
        row['ratio_to_estep_exact'] = row['pass_ms_median'] / yardstick
        print(f'{row["step"]:<17} pass median {row["pass_ms_median"]:8.3f} ms (min {row["pass_ms_min"]:.3f}, max {row["pass_ms_max"]:.3f})  '
              f'call {row["call_ms_median"]:8.3f} ms  {row["terms"] / 1e9:6.3f} G terms  {row["terms"] / row["pass_ms_median"] / 1e6:7.1f} G terms/s  '
              f'x{row["ratio_to_estep_exact"]:.2f} of the exact E-step', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G})', grid=f'{A} values, 0 .. 0.63',
                  clock='dmx_get_timings, DMX_T_ESTEP (pass_ms); host clock around the call and a synchronise (call_ms)', steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
