"""Times learning from doublet posteriors (DeviceContext.em_doublets; include/demux_hip_debug.h: dmx_em_doublets) next to its yardstick,
learning within pools with exact additions (DeviceContext.em_pools: code the new loop does not touch) on the same resident problem.
Writes profiles/doublet_learning.json.

    python scripts/doublet_learning_timing.py [--repeats 12] [--step-timeout 300] [--out profiles/doublet_learning.json]

Input and pools: those of scripts/ambient_learning_timing.py - synth.generate(20_000, 20_000, 64, doublets=True); 8 pools of 8 consecutive
donors, barcodes assigned round-robin; 5 iterations, doublets on.  Steps, each in a process of its own under its own time limit (this
process never opens the GPU):
    pools_exact        dmx_em_pools with exact additions: the yardstick
    doublets_2.0       dmx_em_doublets with min_pair_posterior 2.0: no pair is credited (the same posteriors and additions, bit for bit)
    doublets_1e-3      dmx_em_doublets at the default threshold
    doublets_1e-6      dmx_em_doublets at a threshold that keeps nearly every pair a droplet's calls do not rule out
Nothing of size rows x options is downloaded in a timed call; the read-outs of the last iteration are.
Per step: two warm-up calls, then --repeats calls; of each call the library's phase timers (dmx_get_timings: E-step, M-step, combine,
P-step - events around the launches, summed over the call's iterations) and the host clock around the whole call; medians of each.  In
the E-step slot a dmx_em_doublets call has the spans of its E-steps AND of its list builds; the list build is therefore timed on its
own as well: after the fused calls, one resident E-step and then two warm-up and --repeats calls of dmx_mstep_doublets, whose E-step
slot holds the list build alone (list_ms), next to its walk (step_mstep_ms) and its combine + redo (step_mcombine_ms).
Also per step: the entries of the list (counted on the host from that E-step's rows), and the sums the last M-step redid in call
order (dmx_get_redo_count) next to the sums of variants of several work items."""
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
THRESHOLDS = {'doublets_2.0': 2.0, 'doublets_1e-3': 1e-3, 'doublets_1e-6': 1e-6}
STEPS = ('pools_exact',) + tuple(THRESHOLDS)
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
        threshold = THRESHOLDS.get(step)
        if threshold is None:
            def call():
                ctx.em_pools(ITERATIONS, 0.01, pools, pool_of, True, penalty, fetch_logits=False, fetch_probs=False, fetch_addition=False)
        else:
            def call():
                ctx.em_doublets(ITERATIONS, 0.01, pools, pool_of, True, penalty, threshold, fetch_logits=False, fetch_probs=False, fetch_addition=False)
        estep_spans = ITERATIONS if threshold is None else 2 * ITERATIONS - 1  # (the list builds are spans of the E-step slot)
        ctx.set_phase_timers(True)
        phase_ms, call_ms = {name: [] for name in PHASES}, []
        for i in range(WARM_UP + repeats):
            ctx.reset_timings()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            timings = ctx.timings()
            assert timings['estep']['launches'] == estep_spans and timings['mstep']['launches'] == ITERATIONS - 1, timings
            if i >= WARM_UP:
                for name in PHASES:
                    phase_ms[name].append(timings[name]['ms'] if timings[name]['launches'] else 0.0)
                call_ms.append(host)
        calls_of_variant = np.bincount(p.variant_id, minlength=p.n_variants)
        several = int((calls_of_variant > item_calls_for(int(p.n_calls))).sum()) * G
        options = POOL_SIZE * (POOL_SIZE + 1) // 2
        row = dict(step=step, min_pair_posterior=threshold, iterations=ITERATIONS, options_per_barcode=options, barcodes=B,
                   calls=int(p.n_calls), mstep_form=ctx.mstep_form(), sums_of_several_items=several, sums_redone_last_mstep=ctx.redo_count(),
                   call_ms_median=statistics.median(call_ms), call_ms=call_ms, repeats=repeats, warm_up=WARM_UP)
        for name in PHASES:
            row[f'{name}_ms_median'] = statistics.median(phase_ms[name])
            row[f'{name}_ms'] = phase_ms[name]
        if threshold is not None:  # the M-step on its own, behind the E-step of the table the fused call left: the list build alone
            out = ctx.estep_pools(pools, pool_of, True, penalty, fetch_logits=False, resident=True)
            pairs = out['probs'].reshape(B, options)[:, POOL_SIZE:]
            row['list_entries'] = int((pairs >= np.float32(threshold)).sum())
            row['list_entries_bound'] = int(pairs.size)
            row['barcodes_with_live_pairs'] = int((pairs >= np.float32(threshold)).any(axis=1).sum())
            single = {'list_ms': [], 'step_mstep_ms': [], 'step_mcombine_ms': [], 'step_call_ms': []}
            for i in range(WARM_UP + repeats):
                ctx.reset_timings()
                t0 = time.perf_counter()
                ctx.mstep_doublets(pools, pool_of, True, penalty, out['probs'], threshold, fetch=False)
                ctx.synchronize()
                host = (time.perf_counter() - t0) * 1e3
                timings = ctx.timings()
                assert timings['estep']['launches'] == 1 and timings['mstep']['launches'] == 1, timings
                if i >= WARM_UP:
                    single['list_ms'].append(timings['estep']['ms'])
                    single['step_mstep_ms'].append(timings['mstep']['ms'])
                    single['step_mcombine_ms'].append(timings['mcombine']['ms'])
                    single['step_call_ms'].append(host)  # (with the upload of the rows and the layout)
            for name, values in single.items():
                row[f'{name}_median'] = statistics.median(values)
                row[name] = values
        return row
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--step-timeout', type=float, default=300.0, help='seconds a step may take')
    parser.add_argument('--step', default='', help='(internal) run this step and print its JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'doublet_learning.json'))
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
        alone = (f'  list build alone {row["list_ms_median"]:7.3f}  ({row["list_entries"]} entries of at most {row["list_entries_bound"]})'
                 if 'list_ms_median' in row else '')
        print(f'{step:<14} call {row["call_ms_median"]:9.3f} ms  E-step slot {row["estep_ms_median"]:9.3f}  M-step {row["mstep_ms_median"]:8.3f}  combine '
              f'{row["mcombine_ms_median"]:7.3f}  P-step {row["pstep_ms_median"]:7.3f}  redone {row["sums_redone_last_mstep"]} of '
              f'{row["sums_of_several_items"]} sums of several items{alone}', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G}, doublets=True)', pools=f'{POOLS} pools of {POOL_SIZE} consecutive donors, round-robin',
                  iterations=ITERATIONS,
                  clock='dmx_get_timings, summed over the iterations of a call (*_ms); host clock around the call and a synchronise (call_ms); '
                        'list_ms, step_*: one dmx_mstep_doublets call behind a resident E-step',
                  steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
