"""Times what keeping the call records on the device saves (DESIGN.md "Resident calls") and writes profiles/resident_calls.json.
Both variants of a measurement run in the same process, host containers first; every figure is the median of `--repeats` runs.

  (a) synthetic 200k x 100k x 64 containers: a FIRST predict_posteriors (nothing resident: invalidate_resident() before every
      run) from host containers against the same from ResidentCalls uploaded beforehand; the upload is timed on its own.
  (b) synth.generate_reads(10**7, 10**5) as a ResidentReads: count_snps_from_reads -> predict_posteriors, with host containers in
      between (the parent's behaviour) and with resident_calls=True; wall time and both byte counters of the call records.

    python scripts/resident_calls_timing.py [--only a|b]

The measurement runs in one child process under `timeout -k 10`; if it fails the script ends: nothing is retried."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(values):
    return sorted(values)[len(values) // 2]


def timed(run, repeats, ctx):
    """Median wall time of run() and what one run moved of the call records (host to device, device to host)."""
    walls, moved = [], None
    for _ in range(repeats):
        before = ctx.calls_transfer_bytes()
        t0 = time.perf_counter()
        run()
        walls.append((time.perf_counter() - t0) * 1e3)
        after = ctx.calls_transfer_bytes()
        moved = (after[0] - before[0], after[1] - before[1])
    return dict(wall_ms=median(walls), all_wall_ms=walls, host_to_device_bytes=moved[0], device_to_host_bytes=moved[1])


def measure_predict(args):
    from demuxalot_amd import Demultiplexer, ResidentCalls, invalidate_resident, synth
    from demuxalot_amd.device import get_context
    problem = synth.generate(args.barcodes, args.snps, args.genotypes, seed=7)
    calls, genotypes, handler = synth.as_objects(problem)
    ctx = get_context()
    Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.0)  # context, code objects, the variant keys

    def first_predict(inputs):
        invalidate_resident()
        Demultiplexer.predict_posteriors(inputs, genotypes, handler, doublet_prior=0.0)

    result = dict(barcodes=args.barcodes, snps=args.snps, genotypes=args.genotypes, n_snp_calls=sum(c.n_snp_calls for c in calls.values()),
                  record_bytes=sum(12 * c.n_molecules + 13 * c.n_snp_calls for c in calls.values()))
    result['host_containers'] = timed(lambda: first_predict(calls), args.repeats, ctx)
    uploads, resident = [], None
    for _ in range(args.repeats):
        for calls_set in (resident or {}).values():
            calls_set.close()
        t0 = time.perf_counter()
        resident = {chromosome: ResidentCalls(container) for chromosome, container in calls.items()}
        uploads.append((time.perf_counter() - t0) * 1e3)
    result['upload'] = dict(wall_ms=median(uploads), all_wall_ms=uploads)
    first_predict(resident)
    result['resident_calls'] = timed(lambda: first_predict(resident), args.repeats, ctx)
    for calls_set in resident.values():
        calls_set.close()
    result['saved_ms'] = result['host_containers']['wall_ms'] - result['resident_calls']['wall_ms']
    return result


def measure_count_to_posteriors(args):
    import numpy as np
    from demuxalot_amd import (BarcodeHandler, Demultiplexer, ProbabilisticGenotypes, ResidentReads, count_snps_from_reads, invalidate_resident,
                               synth)
    from demuxalot_amd.device import get_context
    n_barcodes, n_genotypes = 10_000, 8
    reads, positions = synth.generate_reads(args.reads, args.positions, n_barcodes=n_barcodes, seed=1)
    rng = np.random.default_rng(5)
    genotypes = ProbabilisticGenotypes([f'Donor{g + 1}' for g in range(n_genotypes)], default_prior=1.0)
    genotypes.var2varid = {('chr1', int(p), base): 2 * k + b for k, p in enumerate(positions) for b, base in enumerate('AC')}
    genotypes.variant_betas = rng.integers(0, 3, size=(2 * len(positions), n_genotypes)).astype(np.float32)
    handler = BarcodeHandler([f'BC{b:05d}-1' for b in range(n_barcodes)])
    ctx = get_context()
    chromosome2positions = {'chr1': positions}
    with ResidentReads(reads) as resident_reads:
        chromosome2reads = {'chr1': resident_reads}

        def through_the_host():
            invalidate_resident()
            counted = count_snps_from_reads(chromosome2reads, chromosome2positions)
            Demultiplexer.predict_posteriors(counted, genotypes, handler, doublet_prior=0.0)
            return counted

        def on_the_device():
            invalidate_resident()
            counted = count_snps_from_reads(chromosome2reads, chromosome2positions, resident_calls=True)
            try:
                Demultiplexer.predict_posteriors(counted, genotypes, handler, doublet_prior=0.0)
                return counted['chr1'].n_molecules, counted['chr1'].n_snp_calls
            finally:
                counted['chr1'].close()

        counted = through_the_host()  # (warm)
        result = dict(n_reads=args.reads, n_positions=args.positions, n_molecules=int(counted['chr1'].n_molecules),
                      n_snp_calls=int(counted['chr1'].n_snp_calls))
        assert on_the_device() == (result['n_molecules'], result['n_snp_calls'])
        result['host_containers'] = timed(through_the_host, args.repeats, ctx)
        result['resident_calls'] = timed(on_the_device, args.repeats, ctx)
    result['saved_ms'] = result['host_containers']['wall_ms'] - result['resident_calls']['wall_ms']
    return result


def device_step(args):
    result = dict(run_reported='median of all_wall_ms', repeats=args.repeats)
    if args.only in (None, 'a'):
        result['first_predict_posteriors'] = measure_predict(args)
    if args.only in (None, 'b'):
        result['count_to_posteriors'] = measure_count_to_posteriors(args)
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--barcodes', type=int, default=200_000)
    parser.add_argument('--snps', type=int, default=100_000)
    parser.add_argument('--genotypes', type=int, default=64)
    parser.add_argument('--reads', type=int, default=10_000_000)
    parser.add_argument('--positions', type=int, default=100_000)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--only', choices=('a', 'b'))
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resident_calls.json'))
    parser.add_argument('--step', choices=('device',))
    args = parser.parse_args()
    if args.step:
        print('RESULT ' + json.dumps(device_step(args)))
        return
    command = ['timeout', '-k', '10', '560', sys.executable, os.path.abspath(__file__), '--step', 'device', '--repeats', str(args.repeats)]
    for name in ('barcodes', 'snps', 'genotypes', 'reads', 'positions'):
        command += [f'--{name}', str(getattr(args, name))]
    if args.only:
        command += ['--only', args.only]
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
