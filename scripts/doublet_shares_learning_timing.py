"""Times learning from doublets of unequal shares (DeviceContext.em_doublet_shares; include/demux_hip_debug.h: dmx_em_doublet_shares;
DESIGN.md 4.17) next to its yardstick, learning from doublet posteriors (DeviceContext.em_doublets: code the new loop does not touch), on
the same resident problem.  Writes profiles/doublet_shares_learning.json.

    python scripts/doublet_shares_learning_timing.py [--repeats 12] [--step-timeout 300] [--out profiles/doublet_shares_learning.json]

Input, pools and protocol: those of scripts/doublet_learning_timing.py - synth.generate(20_000, 20_000, 64, doublets=True); 8 pools of 8
consecutive donors, barcodes assigned round-robin; 5 iterations, doublets on, threshold 1e-3.  Steps, each in a process of its own under
its own `timeout -k 10` (this process never opens the GPU; a step that fails or runs out of time ends the measurement, nothing is retried):
    doublets_1e-3      dmx_em_doublets: the yardstick
    shares_1           dmx_em_doublet_shares at the grid {0.5}, weight {0}: the same posteriors and additions, bit for bit
    shares_9           dmx_em_doublet_shares at 0.1 .. 0.9 under the uniform prior
Nothing of size rows x options is downloaded in a timed call; the read-outs of the last iteration are.
Per step: two warm-up calls, then --repeats calls; of each call the library's phase timers (dmx_get_timings: E-step, M-step, combine,
P-step - events around the launches, summed over the call's iterations) and the host clock around the whole call; medians of each.  The
E-step slot of a fused call holds the spans of its E-steps (under shares: the grid kernels and, in a span of its own, the rebuild of the
bitmap and codes) AND of its list builds; the parts are therefore timed alone as well: after the fused calls, one resident E-step
(estep_alone_ms) and then two warm-up and --repeats calls of the stateless M-step, whose E-step slot holds the list build alone
(list_ms), next to its walk (step_mstep_ms) and its combine + redo (step_mcombine_ms).  No hardware counters are collected."""
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
B, S, G, POOLS, POOL_SIZE, ITERATIONS, THRESHOLD = 20_000, 20_000, 64, 8, 8, 5, 1e-3
STEPS = ('doublets_1e-3', 'shares_1', 'shares_9')
PHASES = ('pstep', 'estep', 'mstep', 'mcombine')


def grid_of(step):
    """(shares, log_weights) of a step under shares; None for the yardstick."""
    import numpy as np
    from demuxalot_amd.doublet_shares import resolve_shares
    if step == 'shares_1':
        return np.array([0.5], np.float32), np.array([0.0], np.float32)
    return resolve_shares(None, None) if step == 'shares_9' else None


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
        layout = (pools, pool_of, True, penalty)
        grid = grid_of(step)
        quiet = dict(fetch_logits=False, fetch_probs=False, fetch_addition=False)
        if grid is None:
            def call():
                ctx.em_doublets(ITERATIONS, 0.01, *layout, THRESHOLD, **quiet)
        else:
            def call():
                ctx.em_doublet_shares(ITERATIONS, 0.01, *layout, *grid, THRESHOLD, fetch_share_index=False, fetch_share_mean=False, **quiet)
        ctx.set_phase_timers(True)
        phase_ms, call_ms, spans = {name: [] for name in PHASES}, [], None
        for i in range(WARM_UP + repeats):
            ctx.reset_timings()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            timings = ctx.timings()
            assert timings['mstep']['launches'] == ITERATIONS - 1, timings
            spans = timings['estep']['launches']
            if i >= WARM_UP:
                for name in PHASES:
                    phase_ms[name].append(timings[name]['ms'] if timings[name]['launches'] else 0.0)
                call_ms.append(host)
        options = POOL_SIZE * (POOL_SIZE + 1) // 2
        row = dict(step=step, n_shares=None if grid is None else len(grid[0]), min_pair_posterior=THRESHOLD, iterations=ITERATIONS,
                   options_per_barcode=options, barcodes=B, calls=int(p.n_calls), estep_slot_spans=spans, sums_redone_last_mstep=ctx.redo_count(),
                   call_ms_median=statistics.median(call_ms), call_ms=call_ms, repeats=repeats, warm_up=WARM_UP)
        for name in PHASES:
            row[f'{name}_ms_median'] = statistics.median(phase_ms[name])
            row[f'{name}_ms'] = phase_ms[name]
        # the parts alone, behind the E-step of the table the fused call left
        alone = {'estep_alone_ms': [], 'list_ms': [], 'step_mstep_ms': [], 'step_mcombine_ms': [], 'step_call_ms': []}
        for i in range(WARM_UP + repeats):
            ctx.reset_timings()
            if grid is None:
                out = ctx.estep_pools(*layout, fetch_logits=False, resident=True)
            else:
                out = ctx.estep_pair_shares(*layout, *grid, fetch_logits=False, fetch_share_index=False, resident=True)
            ctx.synchronize()
            if i >= WARM_UP:
                alone['estep_alone_ms'].append(ctx.timings()['estep']['ms'])
        pairs = out['probs'].reshape(B, options)[:, POOL_SIZE:]
        row['list_entries'] = int((pairs >= np.float32(THRESHOLD)).sum())
        row['list_entries_bound'] = int(pairs.size)
        row['barcodes_with_live_pairs'] = int((pairs >= np.float32(THRESHOLD)).any(axis=1).sum())
        for i in range(WARM_UP + repeats):
            ctx.reset_timings()
            t0 = time.perf_counter()
            if grid is None:
                ctx.mstep_doublets(*layout, out['probs'], THRESHOLD, fetch=False)
            else:
                ctx.mstep_doublet_shares(*layout, out['probs'], out['share_mean'], THRESHOLD, fetch=False)
            ctx.synchronize()
            host = (time.perf_counter() - t0) * 1e3
            timings = ctx.timings()
            assert timings['estep']['launches'] == 1 and timings['mstep']['launches'] == 1, timings
            if i >= WARM_UP:
                alone['list_ms'].append(timings['estep']['ms'])
                alone['step_mstep_ms'].append(timings['mstep']['ms'])
                alone['step_mcombine_ms'].append(timings['mcombine']['ms'])
                alone['step_call_ms'].append(host)  # (with the upload of the rows and the layout)
        for name, values in alone.items():
            row[f'{name}_median'] = statistics.median(values)
            row[name] = values
        return row
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--step-timeout', type=int, default=300, help='seconds a step may take')
    parser.add_argument('--step', default='', help='(internal) run this step and print its JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'doublet_shares_learning.json'))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(run_step(args.step, args.repeats), default=str), flush=True)
        return
    results = []
    for step in STEPS:  # a step that fails or runs out of time ends the measurement: nothing more is started on the GPU
        done = subprocess.run(['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--step', step,
                               '--repeats', str(args.repeats)], capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            raise SystemExit(f'step {step} ended with status {done.returncode}')
        row = json.loads(next(line for line in done.stdout.splitlines() if line.startswith('RESULT '))[len('RESULT '):])
        results.append(row)
        print(f'{step:<14} call {row["call_ms_median"]:9.3f} ms  E-step slot {row["estep_ms_median"]:9.3f}  M-step {row["mstep_ms_median"]:8.3f}  combine '
              f'{row["mcombine_ms_median"]:7.3f}  P-step {row["pstep_ms_median"]:7.3f}  alone: E-step {row["estep_alone_ms_median"]:7.3f}  list build '
              f'{row["list_ms_median"]:7.3f}  walk {row["step_mstep_ms_median"]:7.3f}  combine {row["step_mcombine_ms_median"]:7.3f}  '
              f'({row["list_entries"]} entries of at most {row["list_entries_bound"]})', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G}, doublets=True)', pools=f'{POOLS} pools of {POOL_SIZE} consecutive donors, round-robin',
                  iterations=ITERATIONS,
                  clock='dmx_get_timings, summed over the iterations of a call (*_ms); host clock around the call and a synchronise (call_ms); '
                        'estep_alone_ms: one resident E-step; list_ms, step_*: one stateless M-step call behind it',
                  steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
