"""Times the pooled E-step (DeviceContext.estep_pools; include/demux_hip_debug.h: dmx_estep_pools) next to its yardstick, the
full-table doublet E-step (dmx_estep) on the same resident problem.  Writes profiles/pooled_posteriors.json.

    python scripts/pooled_posteriors_timing.py [--repeats 12] [--step-timeout 240] [--out profiles/pooled_posteriors.json]

Input: synth.generate(20_000, 20_000, 64, doublets=True); 8 pools of 8 consecutive donors, barcodes assigned round-robin, so a
pooled row has 36 options where the full table's has 2080.  Steps, each in a process of its own under its own time limit (this
process never opens the GPU):
    pools           dmx_estep_pools, results left on the device side of the call (fetch_logits / fetch_probs off: the read-outs
                    are downloaded, the rows are not)
    pools_fetched   the same with the compact rows downloaded (host clock only differs)
    full_exact      dmx_estep, K = 2080, DMX_ESTEP_EXACT, nothing downloaded
    full_default    the same in the library's default mode
Per step: two warm-up calls, then --repeats calls; of each call the library's own phase timer of the E-step (dmx_get_timings, slot
DMX_T_ESTEP: events around the launches, uploads and downloads outside) and the host clock around the whole call; medians of both.
Beside them what a call forms and moves: VALU terms (options x padded calls) and the bytes of its result rows."""
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
B, S, G, POOLS, POOL_SIZE = 20_000, 20_000, 64, 8, 8
STEPS = ('pools', 'pools_fetched', 'full_exact', 'full_default')


def run_step(step, repeats):
    import numpy as np
    from demuxalot_amd import Demultiplexer, synth
    from demuxalot_amd.device import DEFAULT_ESTEP_MODE, DeviceContext
    p = synth.generate(B, S, G, doublets=True)
    ctx = DeviceContext(0)
    try:
        ctx.set_estep_mode('exact' if step == 'full_exact' else DEFAULT_ESTEP_MODE)
        ctx.set_problem(p.n_barcodes, p.n_variants, G, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
        ctx.set_betas(p.prior_betas(add_data_prior=False))
        ctx.set_addition(None)
        ctx.probs_from_betas(0.01, fetch=False)
        calls_per_barcode = np.bincount(p.compressed_cb, minlength=B)
        padded_calls = int(((calls_per_barcode + 7) // 8 * 8).sum())
        if step.startswith('pools'):
            pools = [list(range(POOL_SIZE * i, POOL_SIZE * (i + 1))) for i in range(POOLS)]
            pool_of = (np.arange(B) % POOLS).astype(np.int32)
            penalty = np.full(POOLS, Demultiplexer._doublet_penalties(POOL_SIZE, 0.35)[-1], dtype=np.float32)
            fetch = step == 'pools_fetched'
            options = POOL_SIZE * (POOL_SIZE + 1) // 2

            def call():
                ctx.estep_pools(pools, pool_of, True, penalty, fetch_logits=fetch, fetch_probs=fetch)
        else:
            penalties = Demultiplexer._doublet_penalties(G, 0.35)
            options = G * (G + 1) // 2

            def call():
                ctx.estep(penalties, with_doublets=True, fetch_logits=False, fetch_probs=False)
        ctx.set_phase_timers(True)
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
        return dict(step=step, mode=ctx_mode(step, DEFAULT_ESTEP_MODE), options_per_barcode=options, barcodes=B, calls=int(p.n_calls),
                    padded_calls=padded_calls, valu_terms=options * padded_calls, result_bytes=2 * 4 * options * B,
                    estep_ms_median=statistics.median(phase_ms), estep_ms_min=min(phase_ms), estep_ms_max=max(phase_ms), estep_ms=phase_ms,
                    call_ms_median=statistics.median(call_ms), call_ms=call_ms, repeats=repeats, warm_up=WARM_UP)
    finally:
        ctx.close()


def ctx_mode(step, default):
    return 'exact arithmetic (no modes)' if step.startswith('pools') else 'exact' if step == 'full_exact' else default


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--step-timeout', type=float, default=240.0, help='seconds a step may take')
    parser.add_argument('--step', default='', help='(internal) run this step and print its JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pooled_posteriors.json'))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(run_step(args.step, args.repeats)), flush=True)
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
        print(f'{step:<14} {row["options_per_barcode"]:5d} options  E-step median {row["estep_ms_median"]:8.3f} ms '
              f'(min {row["estep_ms_min"]:.3f}, max {row["estep_ms_max"]:.3f})  call {row["call_ms_median"]:8.3f} ms  '
              f'{row["valu_terms"] / 1e9:7.3f} G terms  {row["result_bytes"] / 1e6:7.1f} MB of rows', flush=True)
    result = dict(input=f'synth.generate({B}, {S}, {G}, doublets=True)', pools=f'{POOLS} pools of {POOL_SIZE} consecutive donors, round-robin',
                  clock='dmx_get_timings, DMX_T_ESTEP (estep_ms); host clock around the call and a synchronise (call_ms)', steps=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
