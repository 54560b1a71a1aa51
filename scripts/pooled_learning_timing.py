"""Times learning within pools (DeviceContext.em_pools; include/demux_hip_debug.h: dmx_em_pools) next to its yardstick, the only way to
learn with doublets without pools: the full-table EM call (DeviceContext.em with doublets, what learn_genotypes(doublet_prior=0.35)
runs) on the same resident problem.  Writes profiles/pooled_learning.json.

    python scripts/pooled_learning_timing.py [--repeats 12] [--step-timeout 300] [--out profiles/pooled_learning.json]

Input: synth.generate(20_000, 20_000, 64, doublets=True); 8 pools of 8 consecutive donors, barcodes assigned round-robin (the input
of scripts/pooled_posteriors_timing.py); 5 iterations.  Steps, each in a process of its own under its own time limit (this process
never opens the GPU):
    pools_exact / pools_default     dmx_em_pools with exact additions (DEMUXALOT_AMD_ESTEP=exact) / with the default additions
    full_exact / full_default       dmx_em, K = 2080, in the exact / the default E-step mode with the additions that go with it
    estep_pools / estep_pools_resident   one pooled E-step without / with the dense singlet rows and the rebuild of the M-step's
                                    bitmaps: the difference of their E-step timers is what the dense form adds per iteration
Nothing of size rows x options is downloaded in any step; the EM steps download the read-outs of the last iteration only.
Per step: two warm-up calls, then --repeats calls; of each call the library's phase timers (dmx_get_timings: E-step, M-step, combine,
P-step - events around the launches, summed over the call's iterations) and the host clock around the whole call; medians of each."""
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
B, S, G, POOLS, POOL_SIZE, ITERATIONS = 20_000, 20_000, 64, 8, 8, 5
STEPS = ('pools_exact', 'pools_default', 'full_exact', 'full_default', 'estep_pools', 'estep_pools_resident')
PHASES = ('pstep', 'estep', 'mstep', 'mcombine')


def run_step(step, repeats):
    import numpy as np
    from demuxalot_amd import Demultiplexer, synth
    from demuxalot_amd.device import DEFAULT_ESTEP_MODE, DeviceContext
    p = synth.generate(B, S, G, doublets=True)
    exact = step.endswith('_exact')
    ctx = DeviceContext(0)
    try:
        ctx.set_estep_mode('exact' if exact else DEFAULT_ESTEP_MODE)
        ctx.set_exact_additions(exact)
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_betas(p.prior_betas(add_data_prior=True))
        pools = [list(range(POOL_SIZE * i, POOL_SIZE * (i + 1))) for i in range(POOLS)]
        pool_of = (np.arange(B) % POOLS).astype(np.int32)
        penalty = np.full(POOLS, Demultiplexer._doublet_penalties(POOL_SIZE, 0.35)[-1], dtype=np.float32)
        penalties = Demultiplexer._doublet_penalties(G, 0.35)
        iterations = ITERATIONS
        if step.startswith('pools'):
            options = POOL_SIZE * (POOL_SIZE + 1) // 2

            def call():
                ctx.em_pools(ITERATIONS, 0.01, pools, pool_of, True, penalty, fetch_logits=False, fetch_probs=False, fetch_addition=False)
        elif step.startswith('full'):
            options = G * (G + 1) // 2
            ctx.set_logits_needed(False)  # as learn_genotypes runs it

            def call():
                ctx.em(ITERATIONS, 0.01, penalties, with_doublets=True, fetch_logits=False, fetch_probs=False, fetch_addition=False)
        else:
            options, iterations = POOL_SIZE * (POOL_SIZE + 1) // 2, 1
            ctx.set_addition(None)
            ctx.probs_from_betas(0.01, fetch=False)

            def call():
                ctx.estep_pools(pools, pool_of, True, penalty, fetch_logits=False, fetch_probs=False, resident=step == 'estep_pools_resident')
        ctx.set_phase_timers(True)
        phase_ms, call_ms = {name: [] for name in PHASES}, []
        for i in range(WARM_UP + repeats):
            ctx.reset_timings()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            timings = ctx.timings()
            assert timings['estep']['launches'] == iterations, timings
            if i >= WARM_UP:
                for name in PHASES:
                    phase_ms[name].append(timings[name]['ms'] if timings[name]['launches'] else 0.0)
                call_ms.append(host)
        row = dict(step=step, estep_mode='exact arithmetic (no modes)' if 'pools' in step else 'exact' if exact else DEFAULT_ESTEP_MODE,
                   exact_additions=exact, iterations=iterations, options_per_barcode=options, barcodes=B, calls=int(p.n_calls),
                   mstep_form=ctx.mstep_form() if iterations > 1 else None, call_ms_median=statistics.median(call_ms), call_ms=call_ms,
                   repeats=repeats, warm_up=WARM_UP)
        for name in PHASES:
            row[f'{name}_ms_median'] = statistics.median(phase_ms[name])
            row[f'{name}_ms'] = phase_ms[name]
        return row
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--step-timeout', type=float, default=300.0, help='seconds a step may take')
    parser.add_argument('--step', default='', help='(internal) run this step and print its JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pooled_learning.json'))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(run_step(args.step, args.repeats), default=str), flush=True)
        return
    results = []
    for step in STEPS:  # a step that fails or runs out of time ends the measurement: nothing more is started on the GPU
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--repeats', str(args.repeats)],
                              capture_output=True, text=True, timeout=args.step_timeout)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            raise SystemExit(f'step {step} ended with status {done.returncode}')
        row = json.loads(next(line for line in done.stdout.splitlines() if line.startswith('RESULT '))[len('RESULT '):])
        results.append(row)
        print(f'{step:<21} {row["iterations"]} x {row["options_per_barcode"]:5d} options  call {row["call_ms_median"]:9.3f} ms  E-step '
              f'{row["estep_ms_median"]:9.3f}  M-step {row["mstep_ms_median"]:8.3f}  combine {row["mcombine_ms_median"]:7.3f}  P-step '
              f'{row["pstep_ms_median"]:7.3f}', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G}, doublets=True)', pools=f'{POOLS} pools of {POOL_SIZE} consecutive donors, round-robin',
                  iterations=ITERATIONS,
                  clock='dmx_get_timings, summed over the iterations of a call (*_ms); host clock around the call and a synchronise (call_ms)',
                  steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
