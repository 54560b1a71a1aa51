"""Times the read-outs over a resident pooled result (DeviceContext.pooled_readout / pooled_top_options / pooled_option_sums;
include/demux_hip_debug.h "Pooled results kept resident") next to two yardsticks, both existing code: the dense
donor read-out (dmx_get_donor_readout) on a resident [B, K] matrix of the same bytes, and the host route - predict_posteriors_in_pools
and the same tables in pandas per pool.  Writes profiles/pooled_readout.json.

    python scripts/pooled_readout_timing.py [--repeats 12] [--step-timeout 300] [--no-kernel-trace] [--out profiles/pooled_readout.json]

Variants, each in a process of its own under its own time limit (this process never opens the GPU):
    kept_a      synth.generate(20_000, 20_000, 64, doublets=True), 8 pools of 8 donors, through dmx_estep_pools with the keep switch on
                and nothing of the rows downloaded; the pass itself is timed with the switch on and off
    upload_b    uploaded rows of 200 000 barcodes at 136 options (one pool of 16 donors with doublets)
    upload_c    uploaded rows of 200 000 barcodes at 990 options (one pool of 44 donors with doublets)
    dense_b / dense_c   dmx_get_donor_readout, with and without marginals, and dmx_get_top_options(1) on dense resident posteriors
                200 000 x 136 / 200 000 x 990: the same bytes
    host_a      Demultiplexer.predict_posteriors_in_pools on kept_a's input, then per pool droplet calls, donor marginals and the
                donor summary in pandas
    device_a    the same call with on_device=True, then droplet_calls(), donor_summary() and donor_marginals(pool) of every pool
Per variant and read-out: two warm-up calls, then --repeats calls; the host clock around each call (it ends in a stream synchronise
and includes the download of the outputs); medians.  `masses` says what the sequential float64 masses cost: the read-out with and
without them requested.  Kernel times: unless --no-kernel-trace, every variant runs once more, alone, under
`rocprofv3 --kernel-trace`, and the median duration of every dispatch of the read-outs' kernels is taken from the trace (the warm-up
dispatches left out); matrix bytes over kernel time is the rate."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM_UP = 2
VARIANTS = ('kept_a', 'upload_b', 'upload_c', 'dense_b', 'dense_c', 'host_a', 'device_a')
B_A, S_A, G_A, POOLS_A, POOL_SIZE_A = 20_000, 20_000, 64, 8, 8
B_UPLOAD = 200_000
UPLOAD_DONORS = {'b': 16, 'c': 44}
KERNELS = ('k_pooled_readout', 'k_pooled_top_options', 'k_pooled_option_partial', 'k_pooled_option_final', 'k_pooled_gather_pool',
           'k_donor_readout', 'k_top_options', 'k_option_partial', 'k_option_final', 'k_estep_pools')


def timed(call, repeats):
    for _ in range(WARM_UP):
        call()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t0) * 1e3)
    return dict(call_ms_median=statistics.median(runs), call_ms_min=min(runs), call_ms_max=max(runs), call_ms=runs)


def pools_a():
    import numpy as np
    from demuxalot_amd import Demultiplexer
    pools = [list(range(POOL_SIZE_A * i, POOL_SIZE_A * (i + 1))) for i in range(POOLS_A)]
    pool_of = (np.arange(B_A) % POOLS_A).astype(np.int32)
    penalty = np.full(POOLS_A, Demultiplexer._doublet_penalties(POOL_SIZE_A, 0.35)[-1], dtype=np.float32)
    return pools, pool_of, penalty


def pooled_passes(ctx, n_options_total):
    return (('readout', lambda: ctx.pooled_readout()),
            ('readout_without_masses', lambda: ctx.pooled_readout(masses=False)),
            ('readout_with_marginals', lambda: ctx.pooled_readout(marginals=True)),
            ('top_options_k1', lambda: ctx.pooled_top_options(1)),
            ('option_sums', lambda: ctx.pooled_option_sums(n_options_total)))


def measure_pooled(ctx, n_options_total, repeats, row):
    info = ctx.pooled_info()
    row.update(barcodes=info['B'], matrix_bytes=4 * info['n_values'], passes={})
    for name, call in pooled_passes(ctx, n_options_total):
        row['passes'][name] = timed(call, repeats)
        row['passes'][name]['matrix_gbytes_per_s_of_call'] = row['matrix_bytes'] / row['passes'][name]['call_ms_median'] / 1e6
    row['masses_cost_call_ms'] = row['passes']['readout']['call_ms_median'] - row['passes']['readout_without_masses']['call_ms_median']
    return row


def run_variant(variant, repeats):
    import numpy as np
    from demuxalot_amd import Demultiplexer, synth
    from demuxalot_amd.device import DeviceContext
    row = dict(variant=variant, repeats=repeats, warm_up=WARM_UP)
    if variant == 'kept_a':
        p = synth.generate(B_A, S_A, G_A, doublets=True)
        pools, pool_of, penalty = pools_a()
        with DeviceContext(0) as ctx:
            ctx.set_problem(p.n_barcodes, p.n_variants, G_A, p.variant_id, p.compressed_cb, p.p_base_wrong, p.v2snp)
            ctx.set_betas(p.prior_betas(add_data_prior=False))
            ctx.set_addition(None)
            ctx.probs_from_betas(0.01, fetch=False)

            def the_pass():
                ctx.estep_pools(pools, pool_of, True, penalty, fetch_logits=False, fetch_probs=False)
            row['pass_keep_off'] = timed(the_pass, repeats)
            ctx.set_keep_pooled(True)
            row['pass_keep_on'] = timed(the_pass, repeats)
            return measure_pooled(ctx, POOLS_A * POOL_SIZE_A * (POOL_SIZE_A + 1) // 2, repeats, row)
    if variant.startswith('upload_'):
        g = UPLOAD_DONORS[variant[-1]]
        K = g * (g + 1) // 2
        rng = np.random.default_rng(0)
        probs = rng.random((B_UPLOAD, K), dtype=np.float32)
        probs /= probs.sum(axis=1, keepdims=True, dtype=np.float32)
        with DeviceContext(0) as ctx:
            ctx.pooled_upload(g, [list(range(g))], np.zeros(B_UPLOAD, np.int32), True, probs.reshape(-1))
            row.update(options=K)
            return measure_pooled(ctx, K, repeats, row)
    if variant.startswith('dense_'):
        from scripts.donor_readout_timing import resident_posteriors
        g = UPLOAD_DONORS[variant[-1]]
        ctx = resident_posteriors(B_UPLOAD, g, True)
        try:
            row.update(barcodes=ctx.B, options=ctx.K, matrix_bytes=ctx.B * ctx.K * 4, passes={})
            for name, call in (('donor_readout', lambda: ctx.get_donor_readout()),
                               ('donor_readout_with_marginals', lambda: ctx.get_donor_readout(marginals=True)),
                               ('top_options_k1', lambda: ctx.get_top_options(1)), ('option_sums', lambda: ctx.get_option_sums())):
                row['passes'][name] = timed(call, repeats)
                row['passes'][name]['matrix_gbytes_per_s_of_call'] = row['matrix_bytes'] / row['passes'][name]['call_ms_median'] / 1e6
            return row
        finally:
            ctx.close()
    # the front door on kept_a's input
    import pandas as pd
    from demuxalot_amd import donor_readout
    p = synth.generate(B_A, S_A, G_A, doublets=True)
    calls, genotypes, handler = synth.as_objects(p)
    names = list(genotypes.genotype_names)
    pool2donors = {f'lane{i}': names[POOL_SIZE_A * i:POOL_SIZE_A * (i + 1)] for i in range(POOLS_A)}
    barcode2pool = {barcode: f'lane{b % POOLS_A}' for b, barcode in enumerate(handler.ordered_barcodes)}

    def host_route():
        t0 = time.perf_counter()
        pooled = Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, barcode2pool, pool2donors)
        t1 = time.perf_counter()
        tables = []
        for pool in pooled.pools:
            _logits, probs = pooled.to_dataframes(pool)
            donors = pool2donors[pool]
            g = len(donors)
            columns = list(probs.columns)
            doublet_mass = probs.iloc[:, g:].sum(axis=1).astype('float64')
            best_singlet = probs.iloc[:, :g].values.argmax(axis=1)
            best_pair = g + probs.iloc[:, g:].values.argmax(axis=1)
            frame = donor_readout.compose_calls(donors, 0.9, best_singlet, probs.values[range(len(probs)), best_singlet], best_pair, doublet_mass.values,
                                                index=probs.index)
            marginals = pd.DataFrame({d: probs[[c for c in columns if d in c.split('+')]].sum(axis=1) for d in donors})
            summary = donor_readout.compose_summary(donors, frame, probs.sum(axis=0).values.astype('float64'))
            tables.append((frame, marginals, summary))
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def device_route():
        t0 = time.perf_counter()
        with Demultiplexer.predict_posteriors_in_pools(calls, genotypes, handler, barcode2pool, pool2donors, on_device=True) as pooled:
            t1 = time.perf_counter()
            pooled.droplet_calls(0.9)
            pooled.donor_summary(0.9)
            for pool in pooled.pools:
                pooled.donor_marginals(pool)
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    route = host_route if variant == 'host_a' else device_route
    runs = [route() for _ in range(WARM_UP + min(repeats, 5))][WARM_UP:]
    row.update(predict_ms_median=statistics.median(r[0] for r in runs), tables_ms_median=statistics.median(r[1] for r in runs),
               predict_ms=[r[0] for r in runs], tables_ms=[r[1] for r in runs], barcodes=B_A)
    return row


def kernels_from(trace_dir):
    """Median durations (microseconds) of the read-outs' kernels in the kernel-trace CSVs under trace_dir, by instantiation."""
    durations = {}
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(path, newline='') as f:
            for record in csv.DictReader(f):
                name = record['Kernel_Name']
                for kernel in KERNELS:
                    at = name.find(kernel)
                    if at >= 0 and (at == 0 or not (name[at - 1].isalnum() or name[at - 1] == '_')):
                        key = name[at:].split('(')[0]
                        durations.setdefault(key, []).append((int(record['End_Timestamp']) - int(record['Start_Timestamp'])) / 1e3)
                        break
    out = {}
    for key, runs in sorted(durations.items()):
        kept = runs[WARM_UP:] if len(runs) > WARM_UP else runs
        out[key] = dict(dispatches=len(runs), kernel_us_median=statistics.median(kept), kernel_us_min=min(kept), kernel_us_max=max(kept))
    return out


def run_child(args, variant, traced):
    command = [sys.executable, os.path.abspath(__file__), '--variant', variant, '--repeats', str(args.repeats)]
    with tempfile.TemporaryDirectory() as trace_dir:
        if traced:
            command = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', trace_dir, '--'] + command
        done = subprocess.run(command, capture_output=True, text=True, timeout=args.step_timeout)
        if done.returncode != 0:  # a variant that fails or runs out of time ends the measurement: nothing more is started on the GPU
            sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
            raise SystemExit(f'variant {variant}{" (traced)" if traced else ""} ended with status {done.returncode}')
        if traced:
            return kernels_from(trace_dir)
    return json.loads(next(line for line in done.stdout.splitlines() if line.startswith('RESULT '))[len('RESULT '):])


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--step-timeout', type=float, default=300.0, help='seconds a variant may take')
    parser.add_argument('--variants', default=','.join(VARIANTS))
    parser.add_argument('--no-kernel-trace', action='store_true')
    parser.add_argument('--variant', default='', help='(internal) run this variant and print its JSON line')
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pooled_readout.json'))
    args = parser.parse_args()
    if args.variant:
        print('RESULT ' + json.dumps(run_variant(args.variant, args.repeats)), flush=True)
        return
    results = []
    for variant in [v for v in args.variants.split(',') if v]:
        row = run_child(args, variant, False)
        if not args.no_kernel_trace and variant not in ('host_a', 'device_a'):
            row['kernels'] = run_child(args, variant, True)
            for key, kernel in row['kernels'].items():
                if key.startswith(('k_pooled_readout', 'k_pooled_top_options', 'k_donor_readout', 'k_top_options')):
                    kernel['matrix_tbytes_per_s'] = row['matrix_bytes'] / kernel['kernel_us_median'] / 1e6
        results.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in ('passes', 'kernels', 'predict_ms', 'tables_ms')}), flush=True)
        for name, numbers in row.get('passes', {}).items():
            print(f'  {variant:<9} {name:<30} call median {numbers["call_ms_median"]:9.3f} ms (min {numbers["call_ms_min"]:.3f}, max {numbers["call_ms_max"]:.3f})', flush=True)
        for key, kernel in row.get('kernels', {}).items():
            rate = f'  {kernel["matrix_tbytes_per_s"]:.2f} TB/s of matrix' if 'matrix_tbytes_per_s' in kernel else ''
            print(f'  {variant:<9} {key:<60} {kernel["dispatches"]:3d} dispatches  median {kernel["kernel_us_median"]:9.1f} us{rate}', flush=True)
    result = dict(input_a=f'synth.generate({B_A}, {S_A}, {G_A}, doublets=True), {POOLS_A} pools of {POOL_SIZE_A} consecutive donors, round-robin',
                  input_b_c=f'{B_UPLOAD} uploaded rows at 136 / 990 options (one pool of 16 / 44 donors with doublets)',
                  clock='host clock around the call and its stream synchronise (call_ms); rocprofv3 --kernel-trace in a run of its own (kernels)',
                  variants=results)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
