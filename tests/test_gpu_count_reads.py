"""Read counting on the GPU (include/demux_hip.h "Read counting"): the device's records against the reference's recorded
output on the f9 fixtures and against the Python restatement of the contract on random and skewed problems, bit for bit;
the invalid inputs; coexistence with a resident problem; count_snps_from_reads feeding predict_posteriors."""
import numpy as np
import pytest

from demuxalot_amd import CompressedSNPCalls, DecodedReads, Demultiplexer, _lib, count_snps_from_reads
from demuxalot_amd.device import get_context, shared_context_lock
from demuxalot_amd.snp_counter import quality_table
from tests import fixture_io as fio
from tests.count_reads_restatement import count_reads
from tests.test_count_reads_cpu import FIXTURES, assert_records_equal, fixture_chromosomes, invalid_problems, small_problem

pytestmark = pytest.mark.gpu


def device_count(reads, positions):
    with shared_context_lock:
        return get_context().count_reads(DecodedReads(**reads), positions, quality_table())


def random_problem(seed, n_reads, n_positions, length, n_cb, n_ub, step, min_step=0):
    """Sorted reads with mixed CIGARs (M I D N S H P = X), letters ACGTN, qualities 0 .. 60, few (cb, ub) keys (many reads per key,
    keys that come back after their molecule was flushed), repeated (start, CIGAR, score) triples (duplicates).  Consecutive
    starts differ by min_step .. step: with min_step >= 1000 every read enters another 1000-base segment, so every read is an
    event (EVERY_READ_AN_EVENT); with min_step = 0 and step above 1000 most are."""
    rng = np.random.default_rng(seed)
    positions = np.sort(rng.choice(length, size=n_positions, replace=False)).astype(np.int32)
    start = np.cumsum(rng.integers(min_step, step + 1, size=n_reads)).astype(np.int64)
    start = (start % max(1, length - 400)) if step <= 1000 else start
    start = np.sort(start).astype(np.int32)
    columns = dict(reference_start=start, compressed_cb=rng.integers(0, n_cb, n_reads).astype(np.int32),
                   compressed_ub=rng.integers(-n_ub, n_ub, n_reads).astype(np.int32),
                   p_misaligned=rng.choice([0.01, 0.5, 0.123456789, 1e-3], n_reads), alignment_score=rng.integers(90, 93, n_reads).astype(np.int32))
    cigars, seqs, quals = [], [], []
    shapes = {}
    for r in range(n_reads):
        shape = int(rng.integers(0, 4))
        if (int(start[r]), shape) not in shapes:  # one CIGAR per (start, shape): equal triples (start, end, score) are frequent
            ops = [(4, int(rng.integers(1, 6)))] if rng.random() < 0.3 else []
            for _ in range(int(rng.integers(1, 5))):
                ops.append((int(rng.choice([0, 7, 8])), int(rng.integers(1, 60))))
                if rng.random() < 0.6:
                    ops.append((int(rng.choice([1, 2, 3, 6])), int(rng.integers(1, 40))))
            ops.append((0, int(rng.integers(1, 30))))
            if rng.random() < 0.3:
                ops.append((4, int(rng.integers(1, 6))))
            if rng.random() < 0.2:
                ops.append((5, int(rng.integers(1, 6))))
            shapes[(int(start[r]), shape)] = ops
        ops = shapes[(int(start[r]), shape)]
        l_seq = sum(n for op, n in ops if op in (0, 1, 4, 6, 7, 8))  # room for the cursor's quirks: P advances it too
        cigars.append(np.array([n << 4 | op for op, n in ops], dtype=np.uint32))
        seqs.append(rng.choice(np.frombuffer(b'ACGTN', dtype=np.uint8), size=l_seq, p=[0.3, 0.3, 0.19, 0.19, 0.02]))
        quals.append(rng.integers(0, 61, l_seq).astype(np.uint8))
    n_cigar = np.array([len(c) for c in cigars], dtype=np.int32)
    l_seq = np.array([len(s) for s in seqs], dtype=np.int32)
    columns.update(n_cigar=n_cigar, cigar_begin=(np.cumsum(n_cigar) - n_cigar).astype(np.int64), l_seq=l_seq,
                   seq_begin=(np.cumsum(l_seq, dtype=np.int64) - l_seq).astype(np.int64), cigar=np.concatenate(cigars),
                   seq=np.concatenate(seqs).astype(np.uint8), qual=np.concatenate(quals))
    return columns, positions


def skewed_problem():
    """One UMI of 6000 complete duplicates (plus a few reads that count), and one position covered by 6000 molecules of one read."""
    n_dup, n_pile = 6000, 6000
    n = n_dup + 3 + n_pile
    start = np.concatenate([np.full(n_dup + 3, 100), np.full(n_pile, 5000)]).astype(np.int32)
    rng = np.random.default_rng(5)
    score = np.concatenate([np.full(n_dup, 98), [97, 96, 98], np.full(n_pile, 98)]).astype(np.int32)
    reads = dict(reference_start=start, compressed_cb=np.concatenate([np.zeros(n_dup + 3), rng.integers(0, 50, n_pile)]).astype(np.int32),
                 compressed_ub=np.concatenate([np.full(n_dup + 3, 77), np.arange(1000, 1000 + n_pile)]).astype(np.int32),
                 p_misaligned=np.full(n, 0.01), alignment_score=score, cigar_begin=np.arange(n, dtype=np.int64),
                 n_cigar=np.ones(n, np.int32), seq_begin=np.arange(n, dtype=np.int64) * 100, l_seq=np.full(n, 100, np.int32),
                 cigar=np.full(n, 100 << 4, np.uint32), seq=rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), size=n * 100),
                 qual=rng.integers(0, 61, n * 100).astype(np.uint8))
    return reads, np.array([120, 150, 5050], dtype=np.int32)


# Starts 1000 .. 1150 apart: every read is an event, and a read of 100 .. 300 reference bases often reaches beyond the next
# event's threshold (its start - 1000), so molecules both survive events and are flushed by them; two (cb, ub) keys.
EVERY_READ_AN_EVENT = dict(seed=6, n_reads=2500, n_positions=30000, length=3000000, n_cb=1, n_ub=1, step=1150, min_step=1000)


@pytest.mark.parametrize('name', FIXTURES)
def test_device_equals_the_reference_on_the_fixtures(name):
    for chromosome, reads, positions, molecules, snp_calls in fixture_chromosomes(name):
        got_molecules, got_calls = device_count(reads, positions)
        print(name, chromosome, len(got_molecules), 'molecules', len(got_calls), 'calls; expected', len(molecules), len(snp_calls))
        assert_records_equal(got_molecules, molecules, f'{name} {chromosome} molecules')
        assert_records_equal(got_calls, snp_calls, f'{name} {chromosome} snp_calls')


@pytest.mark.parametrize('kwargs', [
    dict(seed=1, n_reads=3000, n_positions=400, length=6000, n_cb=4, n_ub=3, step=1),       # deep: many reads per key and position
    dict(seed=2, n_reads=3000, n_positions=3000, length=400000, n_cb=3, n_ub=2, step=260),  # keys that come back after a flush
    dict(seed=3, n_reads=1500, n_positions=20000, length=2400000, n_cb=2, n_ub=2, step=1600),  # most reads are events
    EVERY_READ_AN_EVENT,
    dict(seed=4, n_reads=2000, n_positions=1, length=700, n_cb=50, n_ub=50, step=1),
    dict(seed=5, n_reads=1, n_positions=50, length=300, n_cb=1, n_ub=1, step=1),
], ids=lambda k: f'seed{k["seed"]}')
def test_device_equals_the_restatement_on_random_problems(kwargs):
    reads, positions = random_problem(**kwargs)
    trace = {}
    molecules, snp_calls = count_reads(reads, positions, trace=trace)
    got_molecules, got_calls = device_count(reads, positions)
    print(kwargs, len(molecules), 'molecules', len(snp_calls), 'calls', trace)
    assert_records_equal(got_molecules, molecules, 'molecules')
    assert_records_equal(got_calls, snp_calls, 'snp_calls')


def test_random_problems_exercise_the_contract():
    """The generator's problems must hold the cases they are there for (checked on the restatement's trace)."""
    trace = {}
    for seed, step in ((1, 1), (2, 260)):
        reads, positions = random_problem(seed=seed, n_reads=3000, n_positions=400 if seed == 1 else 3000,
                                          length=6000 if seed == 1 else 400000, n_cb=4 if seed == 1 else 3, n_ub=3 if seed == 1 else 2, step=step)
        count_reads(reads, positions, trace=trace)
        assert reads['qual'].max() == 60 and reads['qual'].min() == 0
    for case in ('key split into molecules', 'event inside a molecule', 'complete duplicate', 'same span, other alignment score',
                 'conflict resolved', 'conflict drops the position', 'N call', 'quality above 40', 'position seen by two reads'):
        assert trace.get(case, 0) > 0, case
    reads, _ = random_problem(seed=3, n_reads=1500, n_positions=20000, length=2400000, n_cb=2, n_ub=2, step=1600)
    start = reads['reference_start'].astype(np.int64)
    assert np.mean(start[1:] // 1000 != start[:-1] // 1000) > 0.4
    reads, positions = random_problem(**EVERY_READ_AN_EVENT)
    start = reads['reference_start'].astype(np.int64)
    assert np.all(start[1:] // 1000 != start[:-1] // 1000), 'every read must be an event'
    trace = {}
    molecules, _calls = count_reads(reads, positions, trace=trace)
    assert len(np.unique(np.stack([reads['compressed_cb'], reads['compressed_ub']]), axis=1)[0]) == 2
    for case in ('key split into molecules', 'event inside a molecule'):  # molecules flushed by an event, and molecules that outlive one
        assert trace.get(case, 0) >= 50, (case, trace)


def test_device_equals_the_restatement_on_the_skewed_problem():
    reads, positions = skewed_problem()
    trace = {}
    molecules, snp_calls = count_reads(reads, positions, trace=trace)
    assert trace['complete duplicate'] >= 5000
    assert np.sum(snp_calls['snp_position'] == 5050) >= 5000 and len(molecules) >= 5000
    got_molecules, got_calls = device_count(reads, positions)
    assert_records_equal(got_molecules, molecules, 'molecules')
    assert_records_equal(got_calls, snp_calls, 'snp_calls')


def test_invalid_inputs_return_the_invalid_argument_status_and_the_context_stays_usable():
    want = count_reads(*small_problem())
    for name, (reads, positions) in invalid_problems().items():
        with pytest.raises(_lib.DemuxHipError, match=r'status -1\)') as error:
            device_count(reads, positions)
        print(name, '->', error.value)
        got = device_count(*small_problem())
        assert_records_equal(got[0], want[0], f'molecules after {name}')
        assert_records_equal(got[1], want[1], f'snp_calls after {name}')
    reads, positions = small_problem()
    with pytest.raises(_lib.DemuxHipError, match=r'status -1\)'):
        device_count(reads, positions[::-1].copy())
    reads['seq_begin'][1] = 15  # the second read's bases would end beyond seq
    with pytest.raises(_lib.DemuxHipError, match=r'status -1\)'):
        device_count(reads, positions)
    reads, positions = small_problem()
    empty = device_count(reads, np.zeros(0, np.int32))
    assert len(empty[0]) == 0 and len(empty[1]) == 0


def test_counting_leaves_a_resident_problem_and_open_posteriors_unchanged():
    fx = fio.load('f3_small_2.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    posteriors = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.35, on_device=True)
    try:
        ctx = posteriors._ctx
        before = (ctx.get_logits().copy(), ctx.get_probs().copy(), posteriors.assignments(0.8).to_dict())
        reads, positions = skewed_problem()
        molecules, snp_calls = ctx.count_reads(DecodedReads(**reads), positions, quality_table())
        assert len(molecules) > 5000
        after = (ctx.get_logits(), ctx.get_probs(), posteriors.assignments(0.8).to_dict())
        fio.assert_bitwise(after[0], before[0], 'logits of the resident problem')
        fio.assert_bitwise(after[1], before[1], 'posteriors of the resident problem')
        assert after[2] == before[2]
        fio.assert_bitwise(after[0], fx['predict1_logits'], 'logits against the fixture')
        # ... and the problem still runs: an E-step on it gives the same posteriors
        again = ctx.estep(with_doublets=True, penalties=Demultiplexer._doublet_penalties(genotypes.n_genotypes, 0.35))
        fio.assert_bitwise(np.asarray(again[1]), before[1], 'posteriors of a new E-step')
    finally:
        posteriors.close()


def test_count_snps_from_reads_feeds_predict_posteriors():
    f1 = fio.load('f1_synthetic_default.npz')
    _calls, genotypes, handler = fio.product_inputs(f1)
    chromosomes = fixture_chromosomes('f9_count_synthetic.npz')
    assert [str(b) for b in fio.load('f9_count_synthetic.npz')['barcodes']] == handler.ordered_barcodes
    chromosome2reads = {c: DecodedReads(**reads) for c, reads, _p, _m, _s in chromosomes}
    chromosome2reads['unlisted'] = chromosome2reads[chromosomes[0][0]]  # reads of a chromosome without positions: skipped
    chromosome2positions = {c: positions for c, _r, positions, _m, _s in chromosomes}
    chromosome2positions['no_reads'] = np.array([5, 6], dtype=np.int32)
    counted = count_snps_from_reads(chromosome2reads, chromosome2positions)
    assert list(counted) == [c for c, *_ in chromosomes] + ['no_reads']
    assert counted['no_reads'].n_molecules == 0 and counted['no_reads'].n_snp_calls == 0
    expected = {}
    for c, _reads, _positions, molecules, snp_calls in chromosomes:
        assert_records_equal(counted[c].molecules, molecules, c)
        assert_records_equal(counted[c].snp_calls, snp_calls, c)
        expected[c] = CompressedSNPCalls()
        expected[c].molecules, expected[c].snp_calls = molecules, snp_calls
        expected[c].n_molecules, expected[c].n_snp_calls = len(molecules), len(snp_calls)
    del counted['no_reads']
    got = Demultiplexer.predict_posteriors(counted, genotypes, handler, doublet_prior=0.25)
    want = Demultiplexer.predict_posteriors(expected, genotypes, handler, doublet_prior=0.25)
    fio.assert_bitwise(got[0].values, want[0].values, 'logits')
    fio.assert_bitwise(got[1].values, want[1].values, 'posteriors')
    assert np.isfinite(got[1].values).all() and got[1].values.shape == (handler.n_barcodes, len(want[1].columns))
