"""Streamed read counting on the GPU (include/demux_hip_debug.h "Streamed read counting"): the records of a stream of chunks
against the reference's recorded output on the f9 fixtures, against the device's own one-shot call and the Python
restatement on synthetic and hand-made reads, record for record and bit for bit; the status codes; the Python front; that the
device memory of a push is bounded by the chunk and the carry."""
import ctypes
import gc
import weakref

import numpy as np
import pytest

from demuxalot_amd import (DecodedReads, Demultiplexer, ReadCounter, _lib, count_snps_from_read_chunks,
                           count_snps_from_reads)
from demuxalot_amd.device import get_context, shared_context_lock
from demuxalot_amd.snp_counter import quality_table
from demuxalot_amd.synth import generate_reads
from tests import fixture_io as fio
from tests.count_reads_restatement import REQUIRED_CASES, count_reads, special_cases
from tests.count_reads_stream_restatement import even_cuts
from tests.test_count_reads_cpu import FIXTURES, assert_records_equal, fixture_chromosomes, small_problem
from tests.test_count_reads_stream_cpu import chunkings

pytestmark = pytest.mark.gpu

INVALID = r'status -1\)'  # DMX_ERR_INVALID
DMX_ERR_UNSUPPORTED = -5


def as_reads(reads):
    return reads if isinstance(reads, DecodedReads) else DecodedReads(**reads)


def stream(reads, positions, cuts, final_is_empty=False, log=None):
    """(molecules, snp_calls) of the reads pushed through a ReadCounter as the chunks the cuts give; log receives
    (molecules emitted, carried reads, peak bytes) per push."""
    reads = as_reads(reads)
    bounds = [0] + [int(c) for c in cuts] + [reads.n_reads]
    parts = []
    with ReadCounter(positions) as counter:
        for k, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            last = k == len(bounds) - 2
            chunk = reads.slice(lo, hi)
            parts.append(counter.finish(chunk) if last and not final_is_empty else counter.push(chunk))
            if log is not None:
                log.append((len(parts[-1][0]), counter.carried_reads, counter._ctx.count_reads_peak_bytes()))
        if final_is_empty:
            parts.append(counter.finish())
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def one_shot(reads, positions):
    with shared_context_lock:
        return get_context().count_reads(as_reads(reads), positions, quality_table())


def assert_same(got, want, what):
    assert_records_equal(got[0], want[0], f'{what}: molecules')
    assert_records_equal(got[1], want[1], f'{what}: snp_calls')


@pytest.mark.parametrize('name', FIXTURES)
def test_streamed_fixtures_equal_the_reference(name):
    for chromosome, reads, positions, molecules, snp_calls in fixture_chromosomes(name):
        if name == 'f9_count_adversarial.npz':
            found = special_cases(reads, positions)
            assert all(found.get(case, 0) >= 1 for case in REQUIRED_CASES) and len(REQUIRED_CASES) == 16
        for what, cuts in chunkings(len(reads['reference_start'])).items():
            assert_same(stream(reads, positions, cuts), (molecules, snp_calls), f'{name} {chromosome} {what}')


@pytest.fixture(scope='module')
def synthetic():
    reads, positions = generate_reads(200_000, 2_000)
    return reads, positions, one_shot(reads, positions)


def cuts_on_events(reads, how_many=12):
    start = reads.reference_start.astype(np.int64)
    events = np.flatnonzero(start[1:] // 1000 != start[:-1] // 1000) + 1
    return [int(e) for e in events[np.linspace(0, len(events) - 1, how_many).astype(int)]]


def cuts_inside_duplicates(reads, how_many=12):
    """Cuts right in front of a read that is a complete duplicate of an earlier one (same key, start, CIGAR, score)."""
    seen, cuts = {}, []
    for r in range(reads.n_reads):
        identity = (int(reads.compressed_cb[r]), int(reads.compressed_ub[r]), int(reads.reference_start[r]), int(reads.n_cigar[r]))
        if identity in seen and r - seen[identity] <= 50:
            cuts.append(r)
        seen[identity] = r
    assert len(cuts) >= how_many
    return [cuts[i] for i in np.linspace(0, len(cuts) - 1, how_many).astype(int)]


SYNTHETIC_CHUNKINGS = {
    '3 chunks': lambda reads: (even_cuts(reads.n_reads, 3), False),
    '16 chunks': lambda reads: (even_cuts(reads.n_reads, 16), False),
    '257 chunks': lambda reads: (even_cuts(reads.n_reads, 257), False),
    'cuts on events': lambda reads: (cuts_on_events(reads), False),
    'cuts inside duplicates': lambda reads: (cuts_inside_duplicates(reads), False),
    'single reads': lambda reads: (list(range(1, 201)), False),
    'empty chunks in the middle': lambda reads: ([reads.n_reads // 4] * 2 + [reads.n_reads // 2] * 3 + [3 * reads.n_reads // 4], False),
    'empty final push': lambda reads: (even_cuts(reads.n_reads, 5), True),
}


@pytest.mark.parametrize('chunking', list(SYNTHETIC_CHUNKINGS))
def test_streamed_synthetic_reads_equal_the_one_shot_call(synthetic, chunking):
    reads, positions, want = synthetic
    cuts, final_is_empty = SYNTHETIC_CHUNKINGS[chunking](reads)
    log = []
    got = stream(reads, positions, cuts, final_is_empty=final_is_empty, log=log)
    print(chunking, len(log), 'pushes; largest carry', max(carry for _m, carry, _b in log), 'molecules', len(got[0]), 'calls', len(got[1]))
    assert len(want[0]) > 5_000 and len(want[1]) > 5_000
    assert_same(got, want, chunking)
    if chunking != 'single reads':
        assert sum(1 for emitted, _c, _b in log[:-1] if emitted) >= 2, 'pushes before the last must emit molecules'


def test_streamed_subsample_equals_the_restatement(synthetic):
    reads, positions, _ = synthetic
    sub = reads.slice(0, 8000)
    want = count_reads(sub.arrays(), positions)
    assert len(want[0]) > 100
    assert_same(stream(sub, positions, even_cuts(8000, 16)), want, 'subsample, 16 chunks')
    assert_same(one_shot(sub, positions), want, 'subsample, one call')


def hand_made(rows, positions):
    """rows: (reference_start, cb, ub, [(op, length)], letter, alignment_score); every base of a read is `letter`, quality 30."""
    cigars = [np.array([length << 4 | op for op, length in ops], dtype=np.uint32) for _s, _c, _u, ops, _l, _a in rows]
    l_seq = np.array([sum(length for op, length in ops if op in (0, 1, 4, 7, 8)) for _s, _c, _u, ops, _l, _a in rows], dtype=np.int32)
    n_cigar = np.array([len(c) for c in cigars], dtype=np.int32)
    reads = dict(reference_start=np.array([r[0] for r in rows], np.int32), compressed_cb=np.array([r[1] for r in rows], np.int32),
                 compressed_ub=np.array([r[2] for r in rows], np.int32), p_misaligned=np.full(len(rows), 0.01),
                 alignment_score=np.array([r[5] for r in rows], np.int32), n_cigar=n_cigar,
                 cigar_begin=(np.cumsum(n_cigar) - n_cigar).astype(np.int64), l_seq=l_seq,
                 seq_begin=(np.cumsum(l_seq, dtype=np.int64) - l_seq).astype(np.int64), cigar=np.concatenate(cigars),
                 seq=np.concatenate([np.full(n, ord(r[4]), np.uint8) for n, r in zip(l_seq, rows)]), qual=np.full(int(l_seq.sum()), 30, np.uint8))
    assert np.all(np.diff(reads['reference_start']) >= 0)
    return reads, np.asarray(positions, dtype=np.int32)


M100 = [(0, 100)]


def test_hand_made_molecules_across_chunks():
    """Key (7, 7) splits into three molecules that lie in three different chunks (another key's read is the event between
    them: a read joins its molecule before it flushes); the duplicate of (3, 3)'s read arrives a chunk later than its
    original; the two reads of (5, 5) disagree at their only position with equal qualities, so that molecule is dropped whole."""
    rows = [(100, 7, 7, M100, 'A', 90), (150, 3, 3, M100, 'C', 90), (150, 5, 5, M100, 'A', 90),    # chunk 0
            (150, 3, 3, M100, 'C', 90), (150, 5, 5, M100, 'G', 91), (190, 1, 1, M100, 'T', 90),    # chunk 1: the duplicate, the conflict
            (3100, 2, 2, M100, 'G', 90), (3150, 7, 7, M100, 'C', 90),                              # chunk 2
            (7100, 4, 4, M100, 'T', 90), (7150, 7, 7, M100, 'G', 90)]                              # chunk 3, the final push
    reads, positions = hand_made(rows, [199, 3199, 7199])
    trace = {}
    want = count_reads(reads, positions, trace=trace)
    assert trace['key split into molecules'] == 2 and trace['complete duplicate'] == 1 and trace['molecule with every position dropped'] == 1
    log = []
    got = stream(reads, positions, [3, 6, 8], log=log)
    print(log, got[0])
    assert_same(got, want, 'hand-made')
    keys = [m[:2] for m in got[0].tolist()]
    assert keys.count((7, 7)) == 3 and (5, 5) not in keys
    assert got[0][keys.index((3, 3))]['p_group_misaligned'] == np.float32(0.01), 'the duplicate must not count'
    assert [carry for _m, carry, _b in log] == [3, 6, 2, 0]
    assert [emitted for emitted, _c, _b in log] == [0, 0, 3, 4]  # read 6 flushes four molecules; (5, 5) leaves no record
    assert_same(stream(reads, positions, list(range(1, len(rows)))), want, 'hand-made, single reads')


def test_a_long_skip_holds_a_molecule_open_while_its_neighbours_flush():
    skip = [(0, 50), (3, 50_000), (0, 50)]
    rows = [(1000, 9, 9, skip, 'A', 90)] + [(1200 + 700 * k, 1, k, M100, 'C', 90) for k in range(72)] + [(50_950, 9, 9, M100, 'G', 90)]
    rows = sorted(rows, key=lambda r: r[0])
    positions = [1010, 51_060, 51_070] + [1200 + 700 * k + 5 for k in range(72)]
    reads, positions = hand_made(rows, sorted(positions))
    want = count_reads(reads, positions)
    cuts = list(range(6, len(rows), 6))
    assert len(cuts) + 1 >= 12
    log = []
    got = stream(reads, positions, cuts, log=log)
    print(log)
    assert_same(got, want, 'long skip')
    late = [k for k, row in enumerate(rows) if row[0] == 50_950][0] // 6
    assert late >= 10 and all(carry >= 1 for _m, carry, _b in log[:-1]), 'the molecule is carried over at least 10 pushes'
    assert sum(1 for emitted, _c, _b in log[1:late] if emitted >= 4) >= 9, 'its neighbours flush meanwhile'
    assert max(carry for _m, carry, _b in log) <= 8
    held = got[0][[m[:2] for m in got[0].tolist()].index((9, 9))]
    assert held['p_group_misaligned'] == np.float32(0.01 * 0.01), 'both reads, 50 000 bases apart, are one molecule'
    assert sorted(got[1]['snp_position'][got[1]['molecule_index'] == [m[:2] for m in got[0].tolist()].index((9, 9))].tolist()) == [1010, 51_060, 51_070]


def test_count_snps_from_read_chunks_consumes_a_generator_one_chunk_at_a_time(synthetic):
    reads, positions, want = synthetic
    alive = []

    def chunks(step=40_000):
        for lo in range(0, reads.n_reads, step):
            gc.collect()
            assert not any(ref() is not None for ref in alive), 'the previous chunk is still alive'
            chunk = reads.slice(lo, lo + step)
            alive.append(weakref.ref(chunk))
            yield chunk
            del chunk

    skipped = []

    def unlisted():
        skipped.append(1)
        yield reads.slice(0, 10)

    got = count_snps_from_read_chunks({'chr1': chunks(), 'unlisted': unlisted()}, {'chr1': positions, 'no_chunks': positions[:5]})
    assert list(got) == ['chr1', 'no_chunks'] and len(alive) == 5 and skipped == [1]
    assert got['no_chunks'].n_molecules == 0 and got['no_chunks'].n_snp_calls == 0
    assert got['chr1'].n_molecules == len(want[0]) and got['chr1'].n_snp_calls == len(want[1])
    assert_same((got['chr1'].molecules, got['chr1'].snp_calls), want, 'chunks from a generator')


def test_max_reads_per_call_gives_the_default_result():
    chromosomes = fixture_chromosomes('f9_count_synthetic.npz')
    chromosome2reads = {c: DecodedReads(**reads) for c, reads, _p, _m, _s in chromosomes}
    chromosome2positions = {c: positions for c, _r, positions, _m, _s in chromosomes}
    chromosome2positions['no_reads'] = np.array([5, 6], dtype=np.int32)
    default = count_snps_from_reads(chromosome2reads, chromosome2positions)
    for step in (1000, 7):
        sliced = count_snps_from_reads(chromosome2reads, chromosome2positions, max_reads_per_call=step)
        assert list(sliced) == list(default)
        for c in default:
            assert_same((sliced[c].molecules, sliced[c].snp_calls), (default[c].molecules, default[c].snp_calls), f'{c}, {step} reads per call')
            assert sliced[c].n_molecules == default[c].n_molecules and sliced[c].n_snp_calls == default[c].n_snp_calls


def far_apart_problem(duplicate_ops=M100):
    """Three molecules, 5000 bases apart: every read flushes the one before it.  The last read is a complete duplicate."""
    rows = [(100, 0, 1, M100, 'A', 90), (5100, 0, 2, M100, 'C', 90), (10_100, 0, 3, M100, 'G', 90), (10_100, 0, 3, duplicate_ops, 'G', 90)]
    return hand_made(rows, [150, 5150, 10_150])


def test_status_codes_of_the_stream():
    """(The status for more than 2^31 - 1 molecules in one stream cannot be reached by a test: it needs that many molecules.)"""
    reads, positions = far_apart_problem()
    decoded, table = DecodedReads(**reads), quality_table()
    want = count_reads(reads, positions)
    with shared_context_lock:
        ctx = get_context()
        with pytest.raises(_lib.DemuxHipError, match=INVALID):  # push without begin
            ctx.count_reads_push(decoded)
        ctx.count_reads_begin(positions, table)
        try:
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # second begin
                ctx.count_reads_begin(positions, table)
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # one-shot call on a context with an open stream
                ctx.count_reads(decoded, positions, table)
            first = ctx.count_reads_push(decoded.slice(0, 2))
            assert len(first[0]) == 1 and ctx.count_reads_carry() == 1
            # carry + chunk above 2^31 - 1 reads: refused before any array is looked at; it ends the stream
            arrays = decoded.slice(2, 4).arrays()
            desc = _lib.DecodedReadsStruct(n_reads=2 ** 31 - 1, n_cigar_ops=2, n_bases=200, **{name: _lib.ptr(a) for name, a in arrays.items()})
            n = ctypes.c_int64(0)
            status = ctx._lib.dmx_count_reads_push(ctx._h, ctypes.cast(ctypes.byref(desc), ctypes.c_void_p), 0, ctypes.byref(n), ctypes.byref(n))
            assert status == DMX_ERR_UNSUPPORTED, status
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # the stream is dead
                ctx.count_reads_push(None, final=True)
        finally:
            ctx.count_reads_end()
        assert ctx.count_reads_carry() == 0
        ctx.count_reads_begin(positions, table)
        try:
            ctx.count_reads_push(decoded.slice(1, 3))
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # a chunk that starts below the previous chunk's last start
                ctx.count_reads_push(decoded.slice(0, 1))
        finally:
            ctx.count_reads_end()
        ctx.count_reads_begin(positions, table)
        try:
            parts = [ctx.count_reads_push(decoded.slice(0, 3)), ctx.count_reads_push(None), ctx.count_reads_push(decoded.slice(3, 4), final=True)]
            assert [len(p[0]) for p in parts] == [2, 0, 1] and parts[2][1]['molecule_index'].tolist() == [2]
            assert_same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want, 'three pushes')
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # push after the final push
                ctx.count_reads_push(None)
        finally:
            ctx.count_reads_end()
        with pytest.raises(_lib.DemuxHipError, match=INVALID):  # positions are checked once, at begin
            ctx.count_reads_begin(positions[::-1].copy(), table)
        # the context is usable for a one-shot call after end
        assert_same(ctx.count_reads(decoded, positions, table), want, 'one call after the streams')
    assert_same(one_shot(*small_problem()), count_reads(*small_problem()), 'small problem')


def test_a_bad_operation_fails_the_push_that_emits_its_molecule_and_not_a_duplicate():
    reads, positions = far_apart_problem()
    want = count_reads(reads, positions)
    # operation 9 moves no cursor: the last read is still a complete duplicate of read 2 (same start, end and score), and does not count
    bad_duplicate, _ = far_apart_problem(duplicate_ops=[(0, 100), (9, 5)])
    bad_duplicate['seq'][300:400] = ord('R')   # ... nor do its letters
    assert_same(stream(bad_duplicate, positions, [1, 2, 3]), want, 'a bad operation in a duplicate of a later chunk')
    bad = {name: value.copy() for name, value in reads.items()}
    bad['cigar'][1] = 100 << 4 | 9  # read 1 counts
    decoded, table = DecodedReads(**bad), quality_table()
    with shared_context_lock:
        ctx = get_context()
        ctx.count_reads_begin(positions, table)
        try:
            assert len(ctx.count_reads_push(decoded.slice(0, 1))[0]) == 0
            # read 1 arrives and flushes read 0's molecule; its own stays open: its operation is not judged yet
            assert len(ctx.count_reads_push(decoded.slice(1, 2))[0]) == 1
            with pytest.raises(_lib.DemuxHipError, match=INVALID):  # read 2 flushes read 1's molecule: this push fails
                ctx.count_reads_push(decoded.slice(2, 3))
            with pytest.raises(_lib.DemuxHipError, match=INVALID):
                ctx.count_reads_push(None, final=True)
        finally:
            ctx.count_reads_end()
        assert_same(ctx.count_reads(DecodedReads(**reads), positions, table), want, 'one call after the failed stream')


def test_a_stream_leaves_a_resident_problem_unchanged():
    fx = fio.load('f3_small_2.npz')
    calls, genotypes, handler = fio.product_inputs(fx)
    posteriors = Demultiplexer.predict_posteriors(calls, genotypes, handler, doublet_prior=0.35, on_device=True)
    try:
        ctx = posteriors._ctx
        before = (ctx.get_logits().copy(), ctx.get_probs().copy())
        (_chromosome, reads, positions, molecules, snp_calls), = fixture_chromosomes('f9_count_adversarial.npz')
        decoded = DecodedReads(**reads)
        parts = []
        with ReadCounter(positions, on_context=ctx) as counter:
            for lo in range(0, decoded.n_reads, 3):
                parts.append(counter.push(decoded.slice(lo, lo + 3)))
            parts.append(counter.finish())
        assert_same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), (molecules, snp_calls), 'adversarial')
        fio.assert_bitwise(ctx.get_logits(), before[0], 'logits of the resident problem')
        fio.assert_bitwise(ctx.get_probs(), before[1], 'posteriors of the resident problem')
        again = ctx.estep(with_doublets=True, penalties=Demultiplexer._doublet_penalties(genotypes.n_genotypes, 0.35))
        fio.assert_bitwise(np.asarray(again[1]), before[1], 'posteriors of a new E-step')
    finally:
        posteriors.close()


def test_a_push_holds_a_fraction_of_what_the_one_shot_call_holds():
    """Every per-read, per-observation and per-molecule cost is linear in the reads of a call, so a sixteenth of the reads plus
    a carry of a few hundred reads holds about a sixteenth of the bytes; the bound leaves room for rocPRIM's fixed temporaries."""
    n = 2_000_000
    reads, positions = generate_reads(n, 20_000)
    with shared_context_lock:
        ctx = get_context()
        want = ctx.count_reads(reads, positions, quality_table())
        one_shot_bytes = ctx.count_reads_peak_bytes()
    log = []
    got = stream(reads, positions, even_cuts(n, 16), log=log)
    print('one call', one_shot_bytes, 'bytes; pushes', [b for _m, _c, b in log], 'carries', [c for _m, c, _b in log])
    assert_same(got, want, '2e6 reads, 16 chunks')
    assert one_shot_bytes > 150 * n
    assert max(b for _m, _c, b in log) < one_shot_bytes / 4
    assert all(0 < carry < 0.01 * n for _m, carry, _b in log[:-1]) and log[-1][1] == 0
