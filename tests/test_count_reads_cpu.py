"""Read counting without a GPU: the Python restatement of the contract (tests/count_reads_restatement.py) against the
reference's recorded output on the three f9 fixtures, record for record; the special cases the adversarial fixture must
contain; DecodedReads.from_reads, hash_string, parse_read and BarcodeHandler.get_barcode_index against values recorded
from the reference; the container helpers; the restatement's argument checks."""
import numpy as np
import pytest

from demuxalot_amd import BarcodeHandler, CompressedSNPCalls, DecodedReads
from demuxalot_amd.cellranger_specific import parse_read
from demuxalot_amd.snp_counter import MOLECULE_DTYPE, SNP_CALL_DTYPE, quality_table
from demuxalot_amd.utils import hash_string
from tests import fixture_io as fio
from tests.count_reads_restatement import REQUIRED_CASES, InvalidReads, count_reads, special_cases

FIXTURES = ('f9_count_synthetic.npz', 'f9_count_example.npz', 'f9_count_adversarial.npz')
NAMES = [name for name, _ in DecodedReads.PER_READ + DecodedReads.FLAT]


def fixture_chromosomes(name):
    """[(chromosome, {array name: array}, positions, molecules, snp_calls)] of a f9 fixture."""
    fx = fio.load(name)
    return [(str(chromosome), {n: fx[f'c{i}_{n}'] for n in NAMES}, fx[f'c{i}_positions'], fx[f'c{i}_molecules'], fx[f'c{i}_snp_calls'])
            for i, chromosome in enumerate(fx['chroms'])]


def assert_records_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what
    assert got.tobytes() == want.tobytes(), f'{what}: float fields differ in their bits'


class Read:
    """A pysam-like read: what from_reads, parse_read and the barcode handler look at."""

    def __init__(self, reference_start, cigartuples, seq, query_qualities, tags, mapq=255):
        self.reference_start, self.cigartuples, self.seq, self.query_qualities = reference_start, cigartuples, seq, query_qualities
        self.tags, self.mapq = dict(tags), mapq

    def has_tag(self, name):
        return name in self.tags

    def get_tag(self, name):
        return self.tags[name]


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_equals_the_reference_record_for_record(name):
    for chromosome, reads, positions, molecules, snp_calls in fixture_chromosomes(name):
        assert molecules.dtype == MOLECULE_DTYPE and snp_calls.dtype == SNP_CALL_DTYPE
        got_molecules, got_calls = count_reads(reads, positions)
        assert_records_equal(got_molecules, molecules, f'{name} {chromosome} molecules')
        assert_records_equal(got_calls, snp_calls, f'{name} {chromosome} snp_calls')


def test_adversarial_fixture_holds_every_special_case():
    (_chromosome, reads, positions, _molecules, _calls), = fixture_chromosomes('f9_count_adversarial.npz')
    found = special_cases(reads, positions)
    assert len(REQUIRED_CASES) == 16
    for case in REQUIRED_CASES:
        assert found.get(case, 0) >= 1, f'the adversarial fixture has no case of: {case}'


def test_quality_table_is_the_reference_expression():
    table = quality_table()
    assert table.dtype == np.float64 and table.shape == (41,)
    assert table[0] == 1.0 and table[40] == 0.1 ** 4.0 and table[13] == 0.1 ** (0.1 * 13)


def test_hash_string_parse_read_and_barcode_index_match_the_recorded_values():
    fx = fio.load('f9_count_adversarial.npz')
    for string, value in zip(fx['hash_strings'], fx['hash_values']):
        assert hash_string(str(string)) == int(value)
    assert 0 <= hash_string('T' * 30) < 2 ** 31
    handler = BarcodeHandler([str(b) for b in fx['barcodes']])
    kinds = set()
    for i in range(len(fx['raw_l_seq'])):
        tags = {'AS': int(fx['raw_alignment_score'][i]), 'NH': int(fx['raw_nh'][i]), 'CB': str(fx['raw_cb'][i])}
        if str(fx['raw_ub'][i]):
            tags['UB'] = str(fx['raw_ub'][i])
        read = Read(0, [(0, int(fx['raw_l_seq'][i]))], 'A' * int(fx['raw_l_seq'][i]), [30] * int(fx['raw_l_seq'][i]), tags,
                    mapq=int(fx['raw_mapq'][i]))
        parsed = parse_read(read)
        assert (parsed is not None) == bool(fx['raw_parsed'][i]), i
        if parsed is not None:
            assert parsed == (float(fx['raw_parsed_p'][i]), int(fx['raw_parsed_ub'][i]))
        index = handler.get_barcode_index(read)
        assert (-1 if index is None else index) == int(fx['raw_barcode_index'][i]), i
        kinds.add((parsed is not None, index is not None))
    assert kinds == {(True, True), (False, True), (True, False)}, 'the recorded reads must exercise both filters'
    other = BarcodeHandler(['X'], tag='XC')
    assert other.get_barcode_index(Read(0, [], '', [], {'CB': 'X'})) is None
    assert other.get_barcode_index(Read(0, [], '', [], {'XC': 'X'})) == 0


def test_from_reads_applies_both_filters_and_lays_the_arrays_out():
    handler = BarcodeHandler(['AAA-1', 'CCC-1'])
    tags = {'NH': 1, 'AS': 8, 'CB': 'CCC-1', 'UB': 'ACG'}
    reads = [
        Read(7, [(4, 2), (0, 5), (1, 1), (0, 2)], 'ACGTNACGTA', [1, 2, 3, 4, 5, 6, 7, 8, 9, 50], tags),
        Read(8, [(0, 10)], 'A' * 10, [30] * 10, dict(tags, NH=2)),               # dropped by parse_read
        Read(8, [(0, 10)], 'A' * 10, [30] * 10, dict(tags, CB='GGG-1')),         # dropped by the barcode handler
        Read(9, [(0, 4), (3, 100), (0, 4), (5, 3)], 'TTTTGGGG', [40] * 8, dict(tags, CB='AAA-1', AS=7)),
    ]
    decoded = DecodedReads.from_reads(reads, handler, parse_read)
    assert decoded.n_reads == 2
    for name, dtype in DecodedReads.PER_READ + DecodedReads.FLAT:
        assert getattr(decoded, name).dtype == dtype and getattr(decoded, name).flags.c_contiguous, name
    assert decoded.reference_start.tolist() == [7, 9] and decoded.compressed_cb.tolist() == [1, 0]
    assert decoded.compressed_ub.tolist() == [hash_string('ACG')] * 2 and decoded.p_misaligned.tolist() == [0.01, 0.01]
    assert decoded.alignment_score.tolist() == [8, 7]
    assert decoded.cigar_begin.tolist() == [0, 4] and decoded.n_cigar.tolist() == [4, 4]
    assert decoded.seq_begin.tolist() == [0, 10] and decoded.l_seq.tolist() == [10, 8]
    assert decoded.cigar.tolist() == [2 << 4 | 4, 5 << 4, 1 << 4 | 1, 2 << 4, 4 << 4, 100 << 4 | 3, 4 << 4, 3 << 4 | 5]
    assert decoded.seq.tobytes() == b'ACGTNACGTATTTTGGGG' and decoded.qual.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 50] + [40] * 8
    empty = DecodedReads.from_reads([], handler, parse_read)
    assert empty.n_reads == 0 and empty.cigar.dtype == np.uint32 and len(empty.seq) == 0
    with pytest.raises(TypeError):
        DecodedReads(reference_start=[0])
    with pytest.raises(ValueError):
        DecodedReads(**dict(decoded.arrays(), l_seq=decoded.l_seq[:1]))


def test_from_reads_reproduces_the_fixture_arrays():
    """Read objects rebuilt from the adversarial fixture's arrays go through from_reads unchanged."""
    (_chromosome, arrays, _positions, _molecules, _calls), = fixture_chromosomes('f9_count_adversarial.npz')

    class Handler:
        def get_barcode_index(self, read):
            return read.get_tag('cb')

    reads = []
    for r in range(len(arrays['reference_start'])):
        c0, s0 = int(arrays['cigar_begin'][r]), int(arrays['seq_begin'][r])
        cigar = [(int(c) & 15, int(c) >> 4) for c in arrays['cigar'][c0:c0 + arrays['n_cigar'][r]]]
        seq = arrays['seq'][s0:s0 + arrays['l_seq'][r]].tobytes().decode()
        reads.append(Read(int(arrays['reference_start'][r]), cigar, seq, arrays['qual'][s0:s0 + arrays['l_seq'][r]].astype(np.int64),
                          {'AS': int(arrays['alignment_score'][r]), 'cb': int(arrays['compressed_cb'][r]),
                           'ub': int(arrays['compressed_ub'][r]), 'p': float(arrays['p_misaligned'][r])}))
    decoded = DecodedReads.from_reads(reads, Handler(), lambda read: (read.get_tag('p'), read.get_tag('ub')))
    for name in NAMES:
        assert np.array_equal(getattr(decoded, name), arrays[name]) and getattr(decoded, name).dtype == arrays[name].dtype, name


def test_concatenate_and_minimize_memory_footprint():
    parts = []
    for _chromosome, _reads, _positions, molecules, snp_calls in fixture_chromosomes('f9_count_synthetic.npz')[:2]:
        part = CompressedSNPCalls()
        part.molecules = np.concatenate([molecules, np.full(3, -1, dtype=MOLECULE_DTYPE)])
        part.snp_calls = np.concatenate([snp_calls, np.full(5, 255, dtype=SNP_CALL_DTYPE)])
        part.n_molecules, part.n_snp_calls = len(molecules), len(snp_calls)
        parts.append(part)
    joined = CompressedSNPCalls.concatenate(parts)
    a, b = parts
    assert joined.n_molecules == a.n_molecules + b.n_molecules == len(joined.molecules)
    assert joined.n_snp_calls == a.n_snp_calls + b.n_snp_calls == len(joined.snp_calls)
    assert np.array_equal(joined.molecules[:a.n_molecules], a.molecules[:a.n_molecules])
    assert np.array_equal(joined.molecules[a.n_molecules:], b.molecules[:b.n_molecules])
    assert np.array_equal(joined.snp_calls[:a.n_snp_calls], a.snp_calls[:a.n_snp_calls])
    tail = joined.snp_calls[a.n_snp_calls:]
    assert np.array_equal(tail['molecule_index'], b.snp_calls['molecule_index'][:b.n_snp_calls] + a.n_molecules)
    for field in ('snp_position', 'base_index', 'p_base_wrong'):
        assert np.array_equal(tail[field], b.snp_calls[field][:b.n_snp_calls])
    assert b.snp_calls['molecule_index'][0] == 0, 'concatenate must not change its inputs'
    a.minimize_memory_footprint()
    assert len(a.molecules) == a.n_molecules and len(a.snp_calls) == a.n_snp_calls
    assert np.array_equal(a.molecules, joined.molecules[:a.n_molecules])
    fresh = CompressedSNPCalls()
    fresh.n_molecules = 1  # an unfilled record inside the valid range
    with pytest.raises(AssertionError):
        fresh.minimize_memory_footprint()


def small_problem():
    reads = dict(reference_start=np.array([10, 20], np.int32), compressed_cb=np.array([0, 0], np.int32),
                 compressed_ub=np.array([5, 6], np.int32), p_misaligned=np.array([0.01, 0.02]), alignment_score=np.array([8, 8], np.int32),
                 cigar_begin=np.array([0, 1], np.int64), n_cigar=np.array([1, 1], np.int32), seq_begin=np.array([0, 10], np.int64),
                 l_seq=np.array([10, 10], np.int32), cigar=np.array([10 << 4, 10 << 4], np.uint32),
                 seq=np.frombuffer(b'ACGTACGTAC' * 2, dtype=np.uint8).copy(), qual=np.full(20, 30, np.uint8))
    return reads, np.array([12, 25], np.int32)


def invalid_problems():
    """{name: (reads, positions)}: the four inputs the C entry point answers with its invalid-argument status."""
    out = {}
    reads, positions = small_problem()
    reads['reference_start'] = reads['reference_start'][::-1].copy()
    out['unsorted reads'] = (reads, positions)
    reads, positions = small_problem()
    reads['cigar'][1] = 10 << 4 | 9
    out['unknown operation'] = (reads, positions)
    reads, positions = small_problem()
    reads['cigar'][1] = 20 << 4   # 20M on a read of 10 bases: position 25 is base 5, fine; position 32 is base 12
    out['read index out of range'] = (reads, np.array([12, 25, 32], np.int32))
    reads, positions = small_problem()
    reads['seq'][15] = ord('R')
    out['bad letter'] = (reads, positions)
    return out


def test_restatement_rejects_the_invalid_inputs_and_accepts_their_valid_twin():
    molecules, snp_calls = count_reads(*small_problem())
    assert molecules.tolist() == [(0, 5, np.float32(0.01)), (0, 6, np.float32(0.02))]
    assert snp_calls.tolist() == [(0, 12, 2, np.float32(0.1 ** 3.0)), (1, 25, 1, np.float32(0.1 ** 3.0))]
    problems = invalid_problems()
    assert sorted(problems) == ['bad letter', 'read index out of range', 'unknown operation', 'unsorted reads']
    for name, (reads, positions) in problems.items():
        with pytest.raises(InvalidReads):
            count_reads(reads, positions)
    # an unknown operation or a bad letter in a read that does not count (a duplicate) or off the SNP positions is no error
    reads, positions = small_problem()
    reads['seq'][14] = ord('R')
    count_reads(reads, positions)


def test_c_entry_points_validate_their_arguments_without_a_gpu():
    """dmx_count_reads and dmx_count_reads_fetch refuse a null context before they touch a device."""
    from demuxalot_amd import _lib
    lib = _lib.load()
    n = _lib.c_int64(0)
    assert lib.dmx_count_reads(None, None, None, 0, None, _lib.ctypes.byref(n), _lib.ctypes.byref(n)) != 0
    assert lib.dmx_count_reads_fetch(None, None, None) != 0


def test_count_snps_from_reads_checks_its_arguments_before_it_counts():
    from demuxalot_amd import count_snps_from_reads

    class NotReads:
        n_reads = 0

    for wrong in (NotReads(), 5, {'reference_start': []}):
        with pytest.raises(TypeError, match='DecodedReads'):
            count_snps_from_reads({'chr1': wrong}, {'chr1': np.array([1], np.int32)}, on_context=object())
    with pytest.raises(TypeError):
        count_snps_from_reads([], {})
    # no reads at all: empty containers, no device call
    empty = count_snps_from_reads({}, {'chr1': np.array([1], np.int32)}, on_context=object())
    assert list(empty) == ['chr1'] and empty['chr1'].n_molecules == 0 and empty['chr1'].n_snp_calls == 0
