"""Times the pooled E-step under per-barcode ambient fractions (DeviceContext.estep_ambient; include/demux_hip_debug.h:
dmx_estep_ambient) next to its yardstick, the pooled E-step (dmx_estep_pools) with one all-donor pool without doublets, on the same
resident problem in the same process.  Writes profiles/estep_ambient.json.

    python scripts/estep_ambient_timing.py [--repeats 12] [--timeout 300] [--out profiles/estep_ambient.json]

Input: synth.generate(20_000, 20_000, 64).  Both passes walk every padded call of every barcode once with 64 lanes, a donor per
lane; the new pass forms the mixture per term (two packed operations per pair of calls more: 18 VALU instructions per call and lane
against 16), fetches 8 bytes more per pair of calls, and runs a prologue with a lane per padded call in front.  Steps, all in ONE
child process under one time limit (this process never opens the GPU):
    pools_singlets     dmx_estep_pools, one pool of all 64 donors, without doublets: the yardstick
    ambient_singlets   dmx_estep_ambient on the same pool, fractions cycling over 0 .. 0.63, the profile supplied
    ambient_derived    ... the profile derived from the calls (the derivation is outside the timer)
    pools_doublets     dmx_estep_pools, every barcode in one of 2 pools of 32 donors, with doublets (528 options)
    ambient_doublets   dmx_estep_ambient on the same pools
Nothing of size row_ptr[B] is downloaded.  Per step: two warm-up calls, then --repeats calls; of each call the library's own phase
timer of the E-step slot (dmx_get_timings, DMX_T_ESTEP: events around the launches - for the new pass the prologue and the walk;
uploads, the profile's derivation and downloads outside) and the host clock around the whole call; medians of both."""
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
STEPS = ('pools_singlets', 'ambient_singlets', 'ambient_derived', 'pools_doublets', 'ambient_doublets')
YARDSTICK = {'ambient_singlets': 'pools_singlets', 'ambient_derived': 'pools_singlets', 'ambient_doublets': 'pools_doublets'}


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
        alpha = np.linspace(0, 0.63, 64, dtype=np.float32)[rows % 64]
        everybody = ([list(range(G))], np.zeros(B, np.int32), False, np.zeros(1, np.float32))
        halves = ([list(range(0, 32)), list(range(32, 64))], (rows % 2).astype(np.int32), True, np.array([-0.5, -0.5], np.float32))
        lean = dict(fetch_logits=False, fetch_probs=False)
        soup = ctx.estep_ambient(*everybody, alpha, **lean)['ambient']
        calls = {
            'pools_singlets': (64, lambda: ctx.estep_pools(*everybody, **lean)),
            'ambient_singlets': (64, lambda: ctx.estep_ambient(*everybody, alpha, ambient=soup, **lean)),
            'ambient_derived': (64, lambda: ctx.estep_ambient(*everybody, alpha, **lean)),
            'pools_doublets': (528, lambda: ctx.estep_pools(*halves, **lean)),
            'ambient_doublets': (528, lambda: ctx.estep_ambient(*halves, alpha, ambient=soup, **lean)),
        }
        ctx.set_phase_timers(True)
        results = []
        for step in STEPS:
            options, call = calls[step]
            phase_ms, call_ms = [], []
            for i in range(WARM_UP + repeats):
                ctx.reset_timings()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                host = (time.perf_counter() - t0) * 1e3
                estep = ctx.timings()['estep']
                assert estep['launches'] == 1, estep
                if i >= WARM_UP:
                    phase_ms.append(estep['ms'])
                    call_ms.append(host)
            results.append(dict(step=step, options=options, barcodes=B, calls=int(p.n_calls), padded_calls=padded_calls, terms=options * padded_calls,
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
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'estep_ambient.json'))
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
    medians = {row['step']: row['pass_ms_median'] for row in results}
    for row in results:
        against = YARDSTICK.get(row['step'])
        row['yardstick'] = against
        row['ratio_to_yardstick'] = row['pass_ms_median'] / medians[against] if against else 1.0
        print(f'{row["step"]:<17} pass median {row["pass_ms_median"]:8.3f} ms (min {row["pass_ms_min"]:.3f}, max {row["pass_ms_max"]:.3f})  '
              f'call {row["call_ms_median"]:8.3f} ms  {row["terms"] / 1e9:6.3f} G terms  {row["terms"] / row["pass_ms_median"] / 1e6:7.1f} G terms/s  '
              f'x{row["ratio_to_yardstick"]:.2f} of {against or "itself"}', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G})', fractions='0 .. 0.63 in steps of 0.01, cycling over the barcodes',
                  clock='dmx_get_timings, DMX_T_ESTEP (pass_ms); host clock around the call and a synchronise (call_ms)', steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
