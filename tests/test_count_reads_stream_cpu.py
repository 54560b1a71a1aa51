"""Streamed read counting without a GPU: the Python restatement of the streaming rule (tests/count_reads_stream_restatement.py)
against the reference's recorded output on the three f9 fixtures for several chunkings, byte for byte, and against the
one-shot restatement on synthetic reads; that the carry stays small; DecodedReads.slice; the argument checks of the Python
front; the new C entry points' null checks."""
import numpy as np
import pytest

from demuxalot_amd import DecodedReads, ReadCounter, count_snps_from_read_chunks, count_snps_from_reads
from demuxalot_amd.synth import generate_reads
from tests.count_reads_restatement import InvalidReads, count_reads
from tests.count_reads_stream_restatement import StreamRestatement, chunk_of, count_reads_streamed, even_cuts
from tests.test_count_reads_cpu import FIXTURES, assert_records_equal, fixture_chromosomes, small_problem


def chunkings(n, seed=0):
    """{name: cuts} for n reads: 2 chunks, 16 chunks, 7 random cuts, cuts that leave empty chunks (at the front, in the middle,
    at the end), and single-read chunks over the first 39 reads."""
    rng = np.random.default_rng(seed)
    return {'2 chunks': even_cuts(n, 2), '16 chunks': even_cuts(n, 16),
            '7 random cuts': sorted(int(c) for c in rng.integers(0, n + 1, 7)),
            'empty chunks': [0, 0, n // 3, n // 3, n // 3, n, n],
            '39 single reads': list(range(1, min(n, 39) + 1))}


@pytest.mark.parametrize('name', FIXTURES)
def test_streamed_restatement_equals_the_reference_byte_for_byte(name):
    for chromosome, reads, positions, molecules, snp_calls in fixture_chromosomes(name):
        for what, cuts in chunkings(len(reads['reference_start'])).items():
            got_molecules, got_calls = count_reads_streamed(reads, positions, cuts)
            assert_records_equal(got_molecules, molecules, f'{name} {chromosome} {what} molecules')
            assert_records_equal(got_calls, snp_calls, f'{name} {chromosome} {what} snp_calls')


@pytest.fixture(scope='module')
def synthetic():
    reads, positions = generate_reads(20000, 400, seed=3)
    return reads.arrays(), positions, count_reads(reads.arrays(), positions)


def test_streamed_restatement_equals_the_one_shot_restatement_and_its_carry_stays_small(synthetic):
    reads, positions, (molecules, snp_calls) = synthetic
    carries = []
    got_molecules, got_calls = count_reads_streamed(reads, positions, even_cuts(20000, 16), carries=carries)
    assert_records_equal(got_molecules, molecules, 'molecules')
    assert_records_equal(got_calls, snp_calls, 'snp_calls')
    print('carry after every push', carries)
    assert len(carries) == 16 and carries[-1] == 0 and min(carries[:-1]) > 0
    assert max(carries) < 0.05 * 20000, 'the carry is the reads of about two segments (50 reads per segment here)'


def test_a_push_emits_what_its_events_flush_and_keeps_the_rest():
    reads, positions = small_problem()  # two molecules of one read: starts 10 and 20
    stream = StreamRestatement(positions)
    first = stream.push(chunk_of(reads, 0, 1))
    assert len(first[0]) == 0 and stream.carried_reads == 1
    middle = stream.push(None)
    assert len(middle[0]) == 0 and stream.carried_reads == 1
    last = stream.push(chunk_of(reads, 1, 2), final=True)
    assert stream.carried_reads == 0 and last[1]['molecule_index'].tolist() == [0, 1]
    want = count_reads(reads, positions)
    assert_records_equal(last[0], want[0], 'molecules')
    assert_records_equal(last[1], want[1], 'snp_calls')
    with pytest.raises(InvalidReads):
        stream.push(None)
    stream = StreamRestatement(positions)
    stream.push(chunk_of(reads, 1, 2))
    with pytest.raises(InvalidReads):
        stream.push(chunk_of(reads, 0, 1))  # starts at 10, below 20


def test_slice_gives_the_reads_with_arrays_of_their_own():
    reads = DecodedReads(reference_start=[5, 6, 7, 9], compressed_cb=[0, 1, 2, 3], compressed_ub=[4, 5, 6, 7],
                         p_misaligned=[0.1, 0.2, 0.3, 0.4], alignment_score=[1, 2, 3, 4], cigar_begin=[0, 2, 2, 3], n_cigar=[2, 0, 1, 2],
                         seq_begin=[0, 3, 7, 7], l_seq=[3, 4, 0, 2], cigar=[3 << 4, 1 << 4 | 1, 4 << 4, 2 << 4, 5 << 4 | 4],
                         seq=np.frombuffer(b'ACGTTTTAC', dtype=np.uint8), qual=np.arange(9))
    part = reads.slice(1, 3)
    assert isinstance(part, DecodedReads) and part.n_reads == 2
    assert part.reference_start.tolist() == [6, 7] and part.compressed_cb.tolist() == [1, 2] and part.compressed_ub.tolist() == [5, 6]
    assert part.p_misaligned.tolist() == [0.2, 0.3] and part.alignment_score.tolist() == [2, 3]
    assert part.cigar_begin.tolist() == [0, 0] and part.n_cigar.tolist() == [0, 1] and part.cigar.tolist() == [4 << 4]
    assert part.seq_begin.tolist() == [0, 4] and part.l_seq.tolist() == [4, 0]
    assert part.seq.tobytes() == b'TTTT' and part.qual.tolist() == [3, 4, 5, 6]
    for name, dtype in DecodedReads.PER_READ + DecodedReads.FLAT:
        assert getattr(part, name).dtype == dtype and getattr(part, name).flags.c_contiguous, name
    tail = reads.slice(3, 10)  # clipped as a Python slice
    assert tail.n_reads == 1 and tail.cigar.tolist() == [2 << 4, 5 << 4 | 4] and tail.seq.tobytes() == b'AC' and tail.cigar_begin.tolist() == [0]
    for lo, hi in ((2, 2), (4, 9), (3, 1)):
        empty = reads.slice(lo, hi)
        assert empty.n_reads == 0 and len(empty.cigar) == 0 and len(empty.seq) == 0 and len(empty.qual) == 0
    whole = reads.slice(0, 4)
    for name, _ in DecodedReads.PER_READ + DecodedReads.FLAT:
        assert np.array_equal(getattr(whole, name), getattr(reads, name)), name
    assert reads.cigar_begin.tolist() == [0, 2, 2, 3], 'slice must not change its input'
    # the slices of a fixture, joined again by the restatement's own chunking, are the fixture's reads
    (_chromosome, arrays, _positions, _molecules, _calls), = fixture_chromosomes('f9_count_adversarial.npz')
    decoded = DecodedReads(**arrays)
    n = decoded.n_reads
    assert n >= 6
    for lo, hi in ((0, n // 3), (n // 3, n - 2), (n - 2, n)):
        want = chunk_of(arrays, lo, hi)
        for name, value in decoded.slice(lo, hi).arrays().items():
            assert np.array_equal(value, want[name]), (lo, hi, name)


def test_the_python_front_checks_its_arguments_before_it_counts():
    positions = {'chr1': np.array([1], np.int32)}
    with pytest.raises(TypeError):
        count_snps_from_read_chunks([], positions)
    with pytest.raises(ValueError, match='max_reads_per_call'):
        count_snps_from_reads({}, positions, on_context=object(), max_reads_per_call=0)
    # no chunks at all: empty containers, no device call; chunks of a chromosome without positions are consumed
    consumed = []

    def chunks():
        consumed.append(1)
        yield None

    empty = count_snps_from_read_chunks({'other': chunks()}, positions, on_context=object())
    assert list(empty) == ['chr1'] and empty['chr1'].n_molecules == 0 and empty['chr1'].n_snp_calls == 0 and consumed == [1]
    empty = count_snps_from_reads({}, positions, on_context=object(), max_reads_per_call=5)
    assert empty['chr1'].n_molecules == 0
    counter = ReadCounter(positions['chr1'], on_context=object())
    assert counter.carried_reads == 0
    with pytest.raises(RuntimeError, match='with'):
        counter.push(None)


def test_stream_entry_points_validate_their_arguments_without_a_gpu():
    from demuxalot_amd import _lib
    lib = _lib.load()
    n = _lib.c_int64(0)
    assert lib.dmx_count_reads_begin(None, None, 0, None) != 0
    assert lib.dmx_count_reads_push(None, None, 1, _lib.ctypes.byref(n), _lib.ctypes.byref(n)) != 0
    assert lib.dmx_count_reads_end(None) != 0
    assert lib.dmx_get_count_reads_carry(None, _lib.ctypes.byref(n)) != 0
    assert lib.dmx_get_count_reads_peak_bytes(None, _lib.ctypes.byref(n)) != 0
