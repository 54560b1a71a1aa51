"""Times the three read passes of a detection - count at the known positions, find_candidate_positions over 10 fragments, count
again - with host arrays and with one resident set (include/demux_hip_debug.h "Resident reads"), on the workload of
scripts/count_reads_timing.py, and writes profiles/resident_reads_1e7.json: the wall time of the three passes in both variants
(the median run of `--repeats`), the bytes of decoded-read arrays each variant copied to the device (dmx_get_reads_upload_bytes),
and, once, the wall time of the upload that makes the set resident.

    python scripts/resident_reads_timing.py [--reads 10000000] [--positions 100000]

The measurement runs in one child process under `timeout -k 10`; if it fails the script ends: nothing is retried."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = dict(minimum_coverage=20, minimum_alternative_fraction=0.01, minimum_alternative_coverage=5, minimum_fraction_of_ref_and_alt=0.98)


def median_run(runs):
    return sorted(runs, key=lambda r: r['wall_ms'])[len(runs) // 2]


def device_step(args):
    import numpy as np
    from demuxalot_amd import ResidentReads, count_snps_from_reads, find_candidate_positions, synth
    from demuxalot_amd.device import get_context
    reads, positions = synth.generate_reads(args.reads, args.positions, seed=1)
    ctx = get_context()
    small, small_positions = synth.generate_reads(10_000, 1_000, seed=2)
    with ResidentReads(small) as warm:  # code objects loaded, the allocator warm
        for these in (small, warm):
            count_snps_from_reads({'c': these}, {'c': small_positions})
            find_candidate_positions({'c': these}, max_fragment_step=1000, **THRESHOLDS)

    def three_passes(these, length, step):
        before, t0 = ctx.reads_upload_bytes(), time.perf_counter()
        known = count_snps_from_reads({'c': these}, {'c': positions})['c']
        t1 = time.perf_counter()
        candidates = find_candidate_positions({'c': these}, max_fragment_step=step, chromosome2length={'c': length}, **THRESHOLDS)['c']
        t2 = time.perf_counter()
        again = count_snps_from_reads({'c': these}, {'c': positions})['c']
        t3 = time.perf_counter()
        assert again.n_snp_calls == known.n_snp_calls
        return dict(wall_ms=(t3 - t0) * 1e3, count_ms=(t1 - t0) * 1e3, candidates_ms=(t2 - t1) * 1e3, count_again_ms=(t3 - t2) * 1e3,
                    upload_bytes=ctx.reads_upload_bytes() - before, n_snp_calls=int(known.n_snp_calls), n_candidates=len(candidates),
                    checksum=int(np.bitwise_xor.reduce(known.snp_calls['snp_position'].astype(np.int64))))

    t0 = time.perf_counter()
    resident = ResidentReads(reads)
    upload_ms = (time.perf_counter() - t0) * 1e3
    try:
        length = resident.reference_length
        step = (length + 9) // 10
        assert len(range(0, length, step)) == 10
        result = dict(n_reads=args.reads, n_positions=args.positions, reference_length=length, fragments=10, run_reported='median of all_wall_ms',
                      resident_upload=dict(wall_ms=upload_ms, device_bytes=resident.nbytes))
        for name, these in (('host_arrays', reads), ('resident', resident)):
            runs = [three_passes(these, length, step) for _ in range(args.repeats)]
            result[name] = dict(median_run(runs), all_wall_ms=[r['wall_ms'] for r in runs])
    finally:
        resident.close()
    for key in ('n_snp_calls', 'n_candidates', 'checksum'):
        assert result['host_arrays'][key] == result['resident'][key], f'the two variants differ in {key}'
    result['wall_resident_over_host'] = result['resident']['wall_ms'] / result['host_arrays']['wall_ms']
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reads', type=int, default=10_000_000)
    parser.add_argument('--positions', type=int, default=100_000)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resident_reads_1e7.json'))
    parser.add_argument('--step', choices=('device',))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(device_step(args)))
        return
    command = ['timeout', '-k', '10', '540', sys.executable, os.path.abspath(__file__), '--step', 'device', '--reads', str(args.reads),
               '--positions', str(args.positions), '--repeats', str(args.repeats)]
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
