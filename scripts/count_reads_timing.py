"""Times count_snps_from_reads' device call on synthetic reads (demuxalot_amd/synth.py: generate_reads) and writes
profiles/count_reads_1e7.json: reads per second, the stages' milliseconds from hipEvents (include/demux_hip_debug.h:
dmx_get_count_reads_timings) of the median of `--repeats` calls, and beside them the wall time of the tests' Python restatement on a subsample, for scale.

    python scripts/count_reads_timing.py [--reads 10000000] [--positions 100000] [--subsample 100000]

Every step runs in a child process under its own `timeout -k 10`; a step that fails ends the script: nothing is retried."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_step(args):
    import numpy as np
    from demuxalot_amd import synth
    from demuxalot_amd.device import get_context
    from demuxalot_amd.snp_counter import quality_table
    reads, positions = synth.generate_reads(args.reads, args.positions, seed=1)
    ctx, table = get_context(), quality_table()
    small, small_positions = synth.generate_reads(10_000, 1_000, seed=2)
    ctx.count_reads(small, small_positions, table)  # code objects loaded, the allocator warm
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        molecules, snp_calls = ctx.count_reads(reads, positions, table)
        wall = time.perf_counter() - t0
        runs.append(dict(wall_ms=wall * 1e3, stage_ms=ctx.count_reads_timings()))
    best = sorted(runs, key=lambda r: r['wall_ms'])[len(runs) // 2]  # the median run
    device_ms = sum(best['stage_ms'].values())
    upload_bytes = sum(a.nbytes for a in reads.arrays().values()) + positions.nbytes + table.nbytes
    return dict(n_reads=args.reads, n_positions=args.positions, read_length=100, n_molecules=len(molecules), n_snp_calls=len(snp_calls),
                upload_bytes=upload_bytes, run_reported='median of all_wall_ms', wall_ms=best['wall_ms'], stages_ms=best['stage_ms'], stages_total_ms=device_ms,
                reads_per_second=args.reads / (best['wall_ms'] * 1e-3), reads_per_second_without_upload=args.reads / ((device_ms - best['stage_ms']['upload']) * 1e-3),
                all_wall_ms=[r['wall_ms'] for r in runs], checksum=int(np.bitwise_xor.reduce(snp_calls['snp_position'].astype(np.int64))))


def restatement_step(args):
    from demuxalot_amd import synth
    from tests.count_reads_restatement import count_reads
    reads, positions = synth.generate_reads(args.subsample, max(1, args.positions * args.subsample // args.reads), seed=1)
    t0 = time.perf_counter()
    molecules, snp_calls = count_reads(reads.arrays(), positions)
    wall = time.perf_counter() - t0
    return dict(n_reads=args.subsample, n_positions=len(positions), n_molecules=len(molecules), n_snp_calls=len(snp_calls), wall_ms=wall * 1e3,
                reads_per_second=args.subsample / wall)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reads', type=int, default=10_000_000)
    parser.add_argument('--positions', type=int, default=100_000)
    parser.add_argument('--subsample', type=int, default=100_000)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'count_reads_1e7.json'))
    parser.add_argument('--step', choices=('device', 'restatement'))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps({'device': device_step, 'restatement': restatement_step}[args.step](args)))
        return
    result = {}
    for step, limit in (('device', 420), ('restatement', 300)):
        command = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--reads', str(args.reads),
                   '--positions', str(args.positions), '--subsample', str(args.subsample), '--repeats', str(args.repeats)]
        done = subprocess.run(command, capture_output=True, text=True, cwd=ROOT)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(f'step {step} ended with status {done.returncode}: stopping here')
        result[step] = json.loads([line for line in done.stdout.splitlines() if line.startswith('RESULT ')][-1][7:])
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
