"""Times the streamed read counting (include/demux_hip_debug.h: dmx_count_reads_begin / _push / _end) on the workload of
scripts/count_reads_timing.py and writes profiles/count_reads_stream_1e7.json: for 1, 16 and 64 chunks the wall time of the whole
stream (slicing on the host excluded: the chunks are cut beforehand), the stages' milliseconds summed over the pushes, the peak
device bytes of the largest push and the largest carry; beside them, from the same process, the one-shot dmx_count_reads on the
same reads as the baseline.  Every figure is the median run of `--repeats`.

    python scripts/count_reads_stream_timing.py [--reads 10000000] [--positions 100000]

The measurement runs in one child process under `timeout -k 10`; if it fails the script ends: nothing is retried."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_run(runs):
    return sorted(runs, key=lambda r: r['wall_ms'])[len(runs) // 2]


def device_step(args):
    import numpy as np
    from demuxalot_amd import _lib, synth
    from demuxalot_amd.device import get_context
    from demuxalot_amd.snp_counter import quality_table
    reads, positions = synth.generate_reads(args.reads, args.positions, seed=1)
    ctx, table = get_context(), quality_table()
    small, small_positions = synth.generate_reads(10_000, 1_000, seed=2)
    ctx.count_reads(small, small_positions, table)  # code objects loaded, the allocator warm
    ctx.count_reads_begin(small_positions, table)
    ctx.count_reads_push(small.slice(0, 5000))
    ctx.count_reads_push(small.slice(5000, 10_000), final=True)
    ctx.count_reads_end()

    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        molecules, snp_calls = ctx.count_reads(reads, positions, table)
        runs.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, stage_ms=ctx.count_reads_timings(), peak_bytes=ctx.count_reads_peak_bytes()))
    best = median_run(runs)
    checksum = int(np.bitwise_xor.reduce(snp_calls['snp_position'].astype(np.int64)))
    result = dict(n_reads=args.reads, n_positions=args.positions, n_molecules=len(molecules), n_snp_calls=len(snp_calls), run_reported='median of all_wall_ms',
                  one_shot=dict(wall_ms=best['wall_ms'], stages_ms=best['stage_ms'], peak_bytes=best['peak_bytes'],
                                stages_without_upload_ms=sum(best['stage_ms'].values()) - best['stage_ms']['upload'],
                                all_wall_ms=[r['wall_ms'] for r in runs]),
                  streams={})
    for n_chunks in args.chunks:
        chunks = [reads.slice(args.reads * k // n_chunks, args.reads * (k + 1) // n_chunks) for k in range(n_chunks)]
        runs = []
        for _ in range(args.repeats):
            stage_ms = dict.fromkeys(_lib.COUNT_READS_STAGES, 0.0)
            peak = carry = n_molecules = n_calls = 0
            folded = 0
            t0 = time.perf_counter()
            ctx.count_reads_begin(positions, table)
            for k, chunk in enumerate(chunks):
                part = ctx.count_reads_push(chunk, final=k == n_chunks - 1)
                t1 = time.perf_counter()  # (the read-outs below are not part of a stream: their time is taken out)
                for stage, ms in ctx.count_reads_timings().items():
                    stage_ms[stage] += ms
                peak, carry = max(peak, ctx.count_reads_peak_bytes()), max(carry, ctx.count_reads_carry())
                n_molecules, n_calls = n_molecules + len(part[0]), n_calls + len(part[1])
                folded ^= int(np.bitwise_xor.reduce(part[1]['snp_position'].astype(np.int64))) if len(part[1]) else 0
                t0 += time.perf_counter() - t1
            ctx.count_reads_end()
            runs.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, stage_ms=stage_ms, peak_bytes=peak, largest_carry=carry))
            assert (n_molecules, n_calls, folded) == (len(molecules), len(snp_calls), checksum), 'the stream counted something else'
        best = median_run(runs)
        result['streams'][str(n_chunks)] = dict(
            wall_ms=best['wall_ms'], stages_ms=best['stage_ms'], stages_without_upload_ms=sum(best['stage_ms'].values()) - best['stage_ms']['upload'],
            peak_bytes=best['peak_bytes'], largest_carry=best['largest_carry'], all_wall_ms=[r['wall_ms'] for r in runs],
            wall_over_one_shot=best['wall_ms'] / result['one_shot']['wall_ms'])
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reads', type=int, default=10_000_000)
    parser.add_argument('--positions', type=int, default=100_000)
    parser.add_argument('--chunks', type=int, nargs='+', default=[1, 16, 64])
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'count_reads_stream_1e7.json'))
    parser.add_argument('--step', choices=('device',))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(device_step(args)))
        return
    command = ['timeout', '-k', '10', '540', sys.executable, os.path.abspath(__file__), '--step', 'device', '--reads', str(args.reads),
               '--positions', str(args.positions), '--repeats', str(args.repeats), '--chunks'] + [str(c) for c in args.chunks]
    done = subprocess.run(command, capture_output=True, text=True, cwd=ROOT)
    if done.returncode != 0:
        sys.stderr.write(done.stdout + done.stderr)
        sys.exit(f'the measurement ended with status {done.returncode}: stopping here')
    result = json.loads([line for line in done.stdout.splitlines() if line.startswith('RESULT ')][-1][7:])
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
