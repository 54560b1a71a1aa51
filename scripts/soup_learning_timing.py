"""Times learning the soup's profile along with the genotypes (DeviceContext.em_ambient_soup; include/demux_hip_debug.h:
dmx_em_ambient_soup) next to its yardstick, learning under the fractions with a fixed profile (DeviceContext.em_ambient: code the new
loop calls and does not change) on the same resident problem, and the soup walk next to the weighted genotype walk on the same
posteriors.  Writes profiles/soup_learning.json.

    python scripts/soup_learning_timing.py [--repeats 12] [--step-timeout 300] [--out profiles/soup_learning.json]

Input, pools and protocol: those of scripts/ambient_learning_timing.py - synth.generate(20_000, 20_000, 64, doublets=True); 8 pools of 8
consecutive donors, barcodes assigned round-robin; 5 iterations, doublets on; fractions cycling 0 / 0.2 / 0.4 over the barcodes, the soup
derived.  Steps, each in a process of its own under its own time limit (this process never opens the GPU):
    ambient_mixed    dmx_em_ambient: the yardstick
    soup_mixed       dmx_em_ambient_soup
    walks            one P-step and one resident ambient E-step, then dmx_mstep_ambient (codes at the floor of its squares), dmx_mstep_soup
                     (the codes rebuilt at floor 0 in its first call) and dmx_mstep_ambient again (codes at floor 0, as the fused loop
                     runs it), each call timed
Per step: two warm-up calls, then --repeats calls; of each call the library's phase timers (dmx_get_timings) and the host clock around
the whole call; medians of each.  Also the sums the last M-step redid in call order (dmx_get_redo_count)."""
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
STEPS = ('ambient_mixed', 'soup_mixed', 'walks')
PHASES = ('pstep', 'estep', 'mstep', 'mcombine')
CYCLE = [0.0, 0.2, 0.4]


def timed(ctx, call, repeats, expect=None):
    """Medians and samples of the phase timers and the host clock over `repeats` calls behind the warm-up calls."""
    phase_ms, call_ms = {name: [] for name in PHASES}, []
    for i in range(WARM_UP + repeats):
        ctx.reset_timings()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        host = (time.perf_counter() - t0) * 1e3
        timings = ctx.timings()
        if expect is not None:
            assert tuple(timings[name]['launches'] for name in ('estep', 'mstep')) == expect, timings
        if i >= WARM_UP:
            for name in PHASES:
                phase_ms[name].append(timings[name]['ms'] if timings[name]['launches'] else 0.0)
            call_ms.append(host)
    row = dict(call_ms_median=statistics.median(call_ms), call_ms=call_ms, repeats=repeats, warm_up=WARM_UP)
    for name in PHASES:
        row[f'{name}_ms_median'] = statistics.median(phase_ms[name])
        row[f'{name}_ms'] = phase_ms[name]
    return row


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
        alpha = np.asarray(CYCLE, dtype=np.float32)[np.arange(B) % len(CYCLE)]
        ctx.set_phase_timers(True)
        head = dict(step=step, fractions=CYCLE, iterations=ITERATIONS, barcodes=B, calls=int(p.n_calls))
        kw = dict(fetch_logits=False, fetch_probs=False, fetch_addition=False)
        if step == 'ambient_mixed':
            row = timed(ctx, lambda: ctx.em_ambient(ITERATIONS, 0.01, pools, pool_of, True, penalty, alpha, **kw), repeats, (ITERATIONS, ITERATIONS - 1))
            return dict(head, sums_redone_last_mstep=ctx.redo_count(), live_posteriors=int(np.count_nonzero(ctx.get_probs())), **row)
        if step == 'soup_mixed':
            row = timed(ctx, lambda: ctx.em_ambient_soup(ITERATIONS, 0.01, pools, pool_of, True, penalty, alpha, **kw), repeats,
                        (ITERATIONS, 2 * (ITERATIONS - 1)))
            return dict(head, sums_redone_last_mstep=ctx.redo_count(), live_posteriors=int(np.count_nonzero(ctx.get_probs())), **row)
        ctx.set_addition(None)
        ctx.probs_from_betas(0.01, fetch=False)
        ctx.estep_ambient(pools, pool_of, True, penalty, alpha, fetch_logits=False, fetch_probs=False, resident=True)
        dense = ctx.get_probs()
        rows = dict(head, live_posteriors=int(np.count_nonzero(dense)), live_above_the_square_floor=int((dense > 2.0 ** -80).sum()))
        for name, call in (('ambient_walk_square_floor', lambda: ctx.mstep_ambient(alpha, fetch=False)),
                           ('soup_walk', lambda: ctx.mstep_soup(alpha)),
                           ('ambient_walk_floor_0', lambda: ctx.mstep_ambient(alpha, fetch=False))):
            rows[name] = dict(timed(ctx, call, repeats), sums_redone=ctx.redo_count())
        return rows
    finally:
        ctx.close()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--step-timeout', type=float, default=300.0, help='seconds a step may take')
    parser.add_argument('--step', default='', help='(internal) run this step and print its JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'soup_learning.json'))
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
        for name, r in ([(step, row)] if step != 'walks' else [(k, v) for k, v in row.items() if isinstance(v, dict)]):
            print(f'{name:<26} call {r["call_ms_median"]:9.3f} ms  E-step {r["estep_ms_median"]:9.3f}  M-step {r["mstep_ms_median"]:8.3f}  combine '
                  f'{r["mcombine_ms_median"]:7.3f}  P-step {r["pstep_ms_median"]:7.3f}', flush=True)
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
