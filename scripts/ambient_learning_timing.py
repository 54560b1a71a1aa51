"""Times learning under per-barcode ambient fractions (DeviceContext.em_ambient; include/demux_hip_debug.h: dmx_em_ambient) next to its
yardstick, learning within pools with exact additions (DeviceContext.em_pools: code the ambient loop does not touch) on the same resident
problem.  Writes profiles/ambient_learning.json.

    python scripts/ambient_learning_timing.py [--repeats 12] [--step-timeout 300] [--out profiles/ambient_learning.json]

Input and pools: those of scripts/pooled_learning_timing.py - synth.generate(20_000, 20_000, 64, doublets=True); 8 pools of 8 consecutive
donors, barcodes assigned round-robin; 5 iterations, doublets on.  Steps, each in a process of its own under its own time limit (this
process never opens the GPU):
    pools_exact      dmx_em_pools with exact additions: the yardstick
    ambient_zero     dmx_em_ambient with every fraction 0 (the same posteriors and additions, bit for bit), the soup derived
    ambient_mixed    dmx_em_ambient with the fractions cycling 0 / 0.2 / 0.4 over the barcodes, the soup derived
Nothing of size rows x options is downloaded in any step; the read-outs of the last iteration are.
Per step: two warm-up calls, then --repeats calls; of each call the library's phase timers (dmx_get_timings: E-step, M-step, combine,
P-step - events around the launches, summed over the call's iterations) and the host clock around the whole call; medians of each.
Also per step: the sums the last M-step redid in call order (dmx_get_redo_count) next to the sums of variants of several work items."""
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
STEPS = ('pools_exact', 'ambient_zero', 'ambient_mixed')
PHASES = ('pstep', 'estep', 'mstep', 'mcombine')
MIN_ITEM_CALLS, MAX_ITEM_CALLS = 1024, 16384  # csrc/kernels.h: item_calls_for


def item_calls_for(n_calls):
    length = MIN_ITEM_CALLS
    while length < MAX_ITEM_CALLS and length * 6000 < n_calls:
        length *= 2
    return length


def run_step(step, repeats):
    import numpy as np
    from demuxalot_amd import Demultiplexer, synth
    from demuxalot_amd.device import DeviceContext
    p = synth.generate(B, S, G, doublets=True)
    ctx = DeviceContext(0)
    try:
        ctx.set_estep_mode('exact')
        ctx.set_exact_additions(True)
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_betas(p.prior_betas(add_data_prior=True))
        pools = [list(range(POOL_SIZE * i, POOL_SIZE * (i + 1))) for i in range(POOLS)]
        pool_of = (np.arange(B) % POOLS).astype(np.int32)
        penalty = np.full(POOLS, Demultiplexer._doublet_penalties(POOL_SIZE, 0.35)[-1], dtype=np.float32)
        cycle = {'ambient_zero': [0.0], 'ambient_mixed': [0.0, 0.2, 0.4]}.get(step)
        if cycle is None:
            def call():
                ctx.em_pools(ITERATIONS, 0.01, pools, pool_of, True, penalty, fetch_logits=False, fetch_probs=False, fetch_addition=False)
        else:
            alpha = np.asarray(cycle, dtype=np.float32)[np.arange(B) % len(cycle)]

            def call():
                ctx.em_ambient(ITERATIONS, 0.01, pools, pool_of, True, penalty, alpha, fetch_logits=False, fetch_probs=False, fetch_addition=False)
        ctx.set_phase_timers(True)
        phase_ms, call_ms = {name: [] for name in PHASES}, []
        for i in range(WARM_UP + repeats):
            ctx.reset_timings()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            timings = ctx.timings()
            assert timings['estep']['launches'] == ITERATIONS and timings['mstep']['launches'] == ITERATIONS - 1, timings
            if i >= WARM_UP:
                for name in PHASES:
                    phase_ms[name].append(timings[name]['ms'] if timings[name]['launches'] else 0.0)
                call_ms.append(host)
        calls_of_variant = np.bincount(p.variant_id, minlength=p.n_variants)
        several = int((calls_of_variant > item_calls_for(int(p.n_calls))).sum()) * G
        row = dict(step=step, fractions=cycle, iterations=ITERATIONS, options_per_barcode=POOL_SIZE * (POOL_SIZE + 1) // 2, barcodes=B,
                   calls=int(p.n_calls), mstep_form=ctx.mstep_form(), sums_of_several_items=several, sums_redone_last_mstep=ctx.redo_count(),
                   call_ms_median=statistics.median(call_ms), call_ms=call_ms, repeats=repeats, warm_up=WARM_UP)
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
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ambient_learning.json'))
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
        print(f'{step:<14} call {row["call_ms_median"]:9.3f} ms  E-step {row["estep_ms_median"]:9.3f}  M-step {row["mstep_ms_median"]:8.3f}  combine '
              f'{row["mcombine_ms_median"]:7.3f}  P-step {row["pstep_ms_median"]:7.3f}  redone {row["sums_redone_last_mstep"]} of '
              f'{row["sums_of_several_items"]} sums of several items', flush=True)
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
