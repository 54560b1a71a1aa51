"""Times the coverage pass (DeviceContext.coverage_count + coverage_candidates) on synthetic reads and writes
profiles/coverage_1e7.json, in the manner of scripts/count_reads_timing.py.

Two workloads of the same size: demuxalot_amd/synth.py: generate_reads (uniform starts), and a piled-up variant of it in which
half of the reads sit on `--hot-starts` starts (1 % of the SNP positions' number by default: thousands of reads on one start, as
RNA-seq piles them on an exon).  Both accumulation forms (include/demux_hip_debug.h: dmx_set_coverage_form) on both; per
combination the stages' milliseconds from hipEvents (dmx_get_coverage_timings) of the median of `--repeats` calls, reads and
aligned bases per second.  The window is the whole chromosome in ONE call, so that every read and base is accumulated once
(find_candidate_positions would cut it into max_fragment_step windows and upload the reads for each).  Beside them: the
yardstick, dmx_count_reads on the same reads in the same process, the share of the three passes of a detection that is upload,
and the wall time of the tests' Python restatement on a subsample, for scale.

    python scripts/coverage_timing.py [--reads 10000000] [--positions 100000] [--subsample 100000]

Every step runs in a child process under its own `timeout -k 10`; a step that fails ends the script: nothing is retried."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = (20, 0.01, 5, 0.98, 10000)  # minimum_coverage, alternative fraction, alternative coverage, fraction of both, cap


def piled_up(reads, hot_starts, seed=3):
    """The same reads with every second one moved onto one of `hot_starts` starts, sorted by start again."""
    import numpy as np
    from demuxalot_amd.snp_counter import DecodedReads
    rng = np.random.default_rng(seed)
    arrays = dict(reads.arrays())
    start = arrays['reference_start'].copy()
    hot = np.sort(rng.choice(int(start.max()), size=hot_starts, replace=False)).astype(np.int32)
    moved = np.arange(len(start)) % 2 == 1
    start[moved] = hot[rng.integers(0, hot_starts, int(moved.sum()))]
    order = np.argsort(start, kind='stable')
    arrays['reference_start'] = start
    for name, _dtype in DecodedReads.PER_READ:
        arrays[name] = arrays[name][order]
    return DecodedReads(**arrays)


def time_coverage(ctx, reads, length, form, repeats, aligned_bases):
    ctx.set_coverage_form(form)
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ctx.coverage_count(reads, 0, length, 15, fetch=False)
        found = ctx.coverage_candidates(*THRESHOLDS)
        wall = time.perf_counter() - t0
        runs.append(dict(wall_ms=wall * 1e3, stage_ms=ctx.coverage_timings()))
    best = sorted(runs, key=lambda r: r['wall_ms'])[len(runs) // 2]  # the median run
    stages = best['stage_ms']
    device_ms = sum(stages.values())
    return dict(run_reported='median of all_wall_ms', wall_ms=best['wall_ms'], stages_ms=stages, stages_total_ms=device_ms,
                stages_without_upload_ms=device_ms - stages['upload'], n_candidates=len(found),
                reads_per_second=reads.n_reads / (best['wall_ms'] * 1e-3),
                reads_per_second_without_upload=reads.n_reads / ((device_ms - stages['upload']) * 1e-3),
                bases_per_second_accumulate=aligned_bases / (stages['accumulate'] * 1e-3), all_wall_ms=[r['wall_ms'] for r in runs])


def device_step(args):
    import numpy as np
    from demuxalot_amd import _lib, synth
    from demuxalot_amd.device import get_context
    from demuxalot_amd.snp_counter import quality_table
    from demuxalot_amd.snp_detection import reference_ends
    reads, positions = synth.generate_reads(args.reads, args.positions, seed=1)
    ctx, table = get_context(), quality_table()
    small, small_positions = synth.generate_reads(10_000, 1_000, seed=2)
    ctx.count_reads(small, small_positions, table)  # code objects loaded, the allocator warm
    for form in (_lib.COVERAGE_ATOMIC, _lib.COVERAGE_TILED):
        ctx.set_coverage_form(form)
        ctx.coverage_count(small, 0, 1_000_000, 15, fetch=False)
        ctx.coverage_candidates(*THRESHOLDS)
    aligned_bases = args.reads * 100
    result = dict(n_reads=args.reads, read_length=100, aligned_bases=aligned_bases, quality_threshold=15, thresholds=list(THRESHOLDS),
                  upload_bytes=sum(reads.arrays()[name].nbytes for name in ('reference_start', 'n_cigar', 'l_seq', 'cigar_begin', 'seq_begin',
                                                                            'cigar', 'seq', 'qual')))
    workloads = {'uniform': reads, 'piled_up': piled_up(reads, args.hot_starts)}
    checksums = {}
    for name, workload in workloads.items():
        length = int(reference_ends(workload).max())
        result[name] = dict(window=[0, length], hot_starts=args.hot_starts if name == 'piled_up' else 0)
        for form_name, form in (('atomic', _lib.COVERAGE_ATOMIC), ('tiled', _lib.COVERAGE_TILED)):
            result[name][form_name] = time_coverage(ctx, workload, length, form, args.repeats, aligned_bases)
            checksums[name, form_name] = int(ctx.coverage_count(workload, 0, min(length, 2_000_000), 15).astype(np.int64).sum())
        assert checksums[name, 'atomic'] == checksums[name, 'tiled']
        result[name]['checksum_first_2e6_positions'] = checksums[name, 'tiled']
    # the yardstick: read counting on the same reads, here and now
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        ctx.count_reads(reads, positions, table)
        runs.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, stage_ms=ctx.count_reads_timings()))
    best = sorted(runs, key=lambda r: r['wall_ms'])[len(runs) // 2]
    counting = dict(wall_ms=best['wall_ms'], stages_ms=best['stage_ms'], stages_total_ms=sum(best['stage_ms'].values()),
                    stages_without_upload_ms=sum(best['stage_ms'].values()) - best['stage_ms']['upload'])
    result['count_reads_yardstick'] = counting
    # a detection uploads the reads three times: count at the known positions, coverage, count at the candidates
    for name in workloads:
        for form_name in ('atomic', 'tiled'):
            coverage = result[name][form_name]
            uploads = 2 * counting['stages_ms']['upload'] + coverage['stages_ms']['upload']
            total = 2 * counting['stages_total_ms'] + coverage['stages_total_ms']
            coverage['coverage_stages_over_count_reads_stages'] = coverage['stages_without_upload_ms'] / counting['stages_without_upload_ms']
            coverage['upload_share_of_three_passes'] = uploads / total
    return result


def restatement_step(args):
    from demuxalot_amd import synth
    from demuxalot_amd.snp_detection import reference_ends
    from tests import coverage_restatement as cr
    reads, _positions = synth.generate_reads(args.subsample, max(1, args.positions * args.subsample // args.reads), seed=1)
    length = int(reference_ends(reads).max())
    t0 = time.perf_counter()
    counts = cr.coverage(reads.arrays(), 0, length, 15)
    found = cr.candidates(counts, 0, minimum_coverage=THRESHOLDS[0], minimum_alternative_fraction=THRESHOLDS[1],
                          minimum_alternative_coverage=THRESHOLDS[2], minimum_fraction_of_ref_and_alt=THRESHOLDS[3], max_snp_candidates=THRESHOLDS[4])
    wall = time.perf_counter() - t0
    return dict(n_reads=args.subsample, window=[0, length], n_candidates=len(found), wall_ms=wall * 1e3, reads_per_second=args.subsample / wall)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reads', type=int, default=10_000_000)
    parser.add_argument('--positions', type=int, default=100_000)
    parser.add_argument('--hot-starts', type=int, default=None)
    parser.add_argument('--subsample', type=int, default=100_000)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coverage_1e7.json'))
    parser.add_argument('--step', choices=('device', 'restatement'))
    args = parser.parse_args()
    if args.hot_starts is None:
        args.hot_starts = max(1, args.positions // 100)
    if args.step:
        print('RESULT ' + json.dumps({'device': device_step, 'restatement': restatement_step}[args.step](args)))
        return
    result = {}
    for step, limit in (('device', 540), ('restatement', 300)):
        command = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--reads', str(args.reads),
                   '--positions', str(args.positions), '--hot-starts', str(args.hot_starts), '--subsample', str(args.subsample),
                   '--repeats', str(args.repeats)]
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
