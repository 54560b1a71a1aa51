"""Times the donor read-out (DeviceContext.get_donor_readout, with and without the marginals) on resident posteriors of the sizes
users run with doublets, next to the yardstick: dmx_get_top_options(k = 1) on the same resident matrix in the same process - the
existing one-pass reduction, which reads the same bytes.  Writes profiles/donor_readout.json.

    python scripts/donor_readout_timing.py [--repeats 12] [--sizes 200000x64d,130000x128d,200000x64] [--pandas 200000x64d]

A size is <barcodes>x<donors>, `d` for doublets.  The posteriors come from one E-step of a problem with two random calls per
barcode and a random table: the passes read every byte of the matrix whatever it holds.  Per size and pass: the median over
`--repeats` calls (after two warm-up calls) of the host clock around the call, which ends in a stream synchronise and includes the
download of the outputs - B values per output, and [B, G] floats for the marginals -, the bytes of the matrix over that time, and
its share of the 8 TB/s the HBM is specified with.  `--pandas`: what the read-out replaces at that size, to_dataframes() and
the same reductions in pandas, once.

The kernels' own times come from a run of this script under a kernel trace, one size per run:
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/donor_readout_timing.py --sizes 130000x128d --pandas '' --out ''
    python scripts/donor_readout_timing.py --kernels-from <dir> [--out profiles/donor_readout_kernels_130000x128d.json]
which prints the median duration of every dispatch of k_donor_readout (by instantiation: <team, marginals, staged>) and of
k_top_options<1> in the trace, the warm-up dispatches left out."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes per second, specified
WARM_UP = 2


def parse_size(text):
    barcodes, donors = text.lower().split('x')
    with_doublets = donors.endswith('d')
    return int(barcodes), int(donors.rstrip('d')), with_doublets


def resident_posteriors(B, G, with_doublets, seed=0):
    import numpy as np
    from demuxalot_amd.device import DeviceContext
    rng = np.random.default_rng(seed)
    V = 64
    ctx = DeviceContext(0)
    cb = np.repeat(np.arange(B, dtype=np.int32), 2)
    ctx.set_problem(B, V, G, rng.integers(0, V, 2 * B), cb, rng.uniform(0.001, 0.3, 2 * B).astype(np.float32), np.arange(V, dtype=np.int32))
    ctx.set_probs(rng.random((V, G), dtype=np.float32))
    K = G * (G + 1) // 2 if with_doublets else G
    ctx.estep(np.zeros(K, dtype=np.float32), with_doublets=with_doublets, fetch_logits=False, fetch_probs=False)
    return ctx


def timed(call, repeats):
    for _ in range(WARM_UP):
        call()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t0) * 1e3)
    return runs


def measure(size, repeats):
    B, G, with_doublets = parse_size(size)
    ctx = resident_posteriors(B, G, with_doublets)
    try:
        matrix_bytes = ctx.B * ctx.K * 4
        row = dict(size=size, barcodes=B, donors=G, options=ctx.K, matrix_bytes=matrix_bytes, repeats=repeats, passes={})
        passes = (('top_options_k1', lambda: ctx.get_top_options(1)),
                  ('donor_readout', lambda: ctx.get_donor_readout()),
                  ('donor_readout_with_marginals', lambda: ctx.get_donor_readout(marginals=True)))
        for name, call in passes:
            runs = timed(call, repeats)
            median = statistics.median(runs)
            row['passes'][name] = dict(call_ms_median=median, call_ms_min=min(runs), call_ms_max=max(runs), call_ms=runs,
                                       matrix_gbytes_per_s=matrix_bytes / median / 1e6,
                                       share_of_hbm_peak=matrix_bytes / (median * 1e-3) / HBM_PEAK)
            print(f'{size:>14}  {name:<30} median {median:9.3f} ms  (min {min(runs):.3f}, max {max(runs):.3f})  '
                  f'{matrix_bytes / median / 1e6:8.1f} GB/s of matrix', flush=True)
        return row
    finally:
        ctx.close()


def pandas_equivalent(size):
    """to_dataframes() and the reductions of the read-out in pandas: what a user of a doublet run did before."""
    import pandas as pd
    from demuxalot_amd.demux import DevicePosteriors, _option_names
    B, G, with_doublets = parse_size(size)
    ctx = resident_posteriors(B, G, with_doublets)
    donors = [f'd{g}' for g in range(G)]
    columns = _option_names(donors, 0.35 if with_doublets else 0.0)
    dev = DevicePosteriors(ctx, [f'b{i}' for i in range(B)], columns, pooled=False, n_donors=G)
    try:
        t0 = time.perf_counter()
        _logits_df, probs = dev.to_dataframes()
        t1 = time.perf_counter()
        doublet_probability = probs.iloc[:, G:].sum(axis=1)
        best_singlet, best_singlet_prob = probs.iloc[:, :G].idxmax(axis=1), probs.iloc[:, :G].max(axis=1)
        best_pair = probs.iloc[:, G:].idxmax(axis=1)
        t2 = time.perf_counter()
        marginals = pd.DataFrame({d: probs[[c for c in columns if d in c.split('+')]].sum(axis=1) for d in donors})
        t3 = time.perf_counter()
        assert len(doublet_probability) == len(best_singlet) == len(best_singlet_prob) == len(best_pair) == len(marginals) == B
        row = dict(size=size, to_dataframes_ms=(t1 - t0) * 1e3, pandas_masses_and_best_ms=(t2 - t1) * 1e3, pandas_marginals_ms=(t3 - t2) * 1e3)
        print(f'{size:>14}  to_dataframes {row["to_dataframes_ms"]:.0f} ms, pandas masses and arg-maxes {row["pandas_masses_and_best_ms"]:.0f} ms, '
              f'pandas marginals {row["pandas_marginals_ms"]:.0f} ms', flush=True)
        return row
    finally:
        dev.close()


def kernels_from(trace_dir):
    """Median durations (microseconds) of the read-out's and the yardstick's kernels in the kernel-trace CSVs under trace_dir."""
    durations = {}
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(path, newline='') as f:
            for record in csv.DictReader(f):
                name = record['Kernel_Name']
                if 'k_donor_readout' in name:
                    key = 'k_donor_readout' + name[name.index('k_donor_readout') + len('k_donor_readout'):].split('(')[0]
                elif 'k_top_options' in name:
                    key = 'k_top_options' + name[name.index('k_top_options') + len('k_top_options'):].split('(')[0]
                else:
                    continue
                durations.setdefault(key, []).append((int(record['End_Timestamp']) - int(record['Start_Timestamp'])) / 1e3)
    out = {}
    for key, runs in sorted(durations.items()):
        kept = runs[WARM_UP:] if len(runs) > WARM_UP else runs
        out[key] = dict(dispatches=len(runs), kernel_us_median=statistics.median(kept), kernel_us_min=min(kept), kernel_us_max=max(kept))
        print(f'{key:<44} {len(runs):3d} dispatches  median {out[key]["kernel_us_median"]:10.1f} us  (min {min(kept):.1f}, max {max(kept):.1f})')
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--repeats', type=int, default=12)
    parser.add_argument('--sizes', default='200000x64d,130000x128d,200000x64')
    parser.add_argument('--pandas', default='200000x64d')
    parser.add_argument('--kernels-from', default='')
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if args.kernels_from:
        result = dict(trace=args.kernels_from, kernels=kernels_from(args.kernels_from))
        assert result['kernels'], f'no kernel trace of the read-out under {args.kernels_from}'
        out = args.out
    else:
        from demuxalot_amd import _lib
        assert _lib.device_count() > 0, 'this measurement needs the GPU'
        result = dict(hbm_peak_bytes_per_s=HBM_PEAK, warm_up=WARM_UP, sizes=[measure(s, args.repeats) for s in args.sizes.split(',') if s])
        if args.pandas:
            result['pandas_equivalent'] = pandas_equivalent(args.pandas)
        out = os.path.join(ROOT, 'profiles', 'donor_readout.json') if args.out is None else args.out
    if out:
        with open(out, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', out)


if __name__ == '__main__':
    main()
