"""
tests/golden/make_count_fixtures.py -- regenerates the read-counting fixtures tests/golden/f9_count_*.npz.

Runs ONLY where the reference is importable (make_fixtures.py: import_reference and its in-memory pysam stand-in).
Per case and chromosome it captures
  * the reads the reference's scanner kept, as the arrays of demuxalot_amd.DecodedReads, taken from the very read objects
    count_call_variants_for_chromosome scanned (recorded through the parse_read / barcode handler it was given),
  * the SNP positions,
  * the records count_call_variants_for_chromosome returned.
Nothing of the reference's source travels: the fixtures are inputs and recorded outputs.

    python tests/golden/make_count_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_fixtures import REFERENCE, import_reference, save  # noqa: E402

PER_READ = ('reference_start', 'compressed_cb', 'compressed_ub', 'p_misaligned', 'alignment_score', 'cigar_begin', 'n_cigar',
            'seq_begin', 'l_seq')
MAX_BYTES = 1 << 20  # a committed file stays below 1 MiB


class _Reads:
    """What count_call_variants_for_chromosome needs of an open BAM file: fetch()."""

    def __init__(self, reads):
        self.reads = reads

    def fetch(self, chromosome, start=None, stop=None):
        return iter(self.reads)


def scan(ref, reads, chromosome, positions, handler, parse_read):
    """Runs the reference's scanner over `reads`; returns (arrays of the kept reads, molecules, snp_calls)."""
    kept, last = [], {}

    def recording_parse(read):
        last['parsed'] = parse_read(read)
        return last['parsed']

    class RecordingHandler:
        def get_barcode_index(self, read):
            cb = handler.get_barcode_index(read)
            if cb is not None:
                kept.append((read, cb, last['parsed']))
            return cb

    _, calls = ref.snp_counter.count_call_variants_for_chromosome(_Reads(reads), chromosome, np.asarray(positions), RecordingHandler(),
                                                                  parse_read=recording_parse)
    columns = {name: [] for name in PER_READ}
    cigar, seq, qual = [], [], []
    for read, cb, (p_misaligned, ub) in kept:
        columns['reference_start'].append(read.reference_start)
        columns['compressed_cb'].append(cb)
        columns['compressed_ub'].append(ub)
        columns['p_misaligned'].append(p_misaligned)
        columns['alignment_score'].append(read.get_tag('AS'))
        columns['cigar_begin'].append(len(cigar))
        columns['n_cigar'].append(len(read.cigartuples))
        columns['seq_begin'].append(len(seq))
        columns['l_seq'].append(len(read.seq))
        cigar.extend((length << 4) | op for op, length in read.cigartuples)
        seq.extend(read.seq.encode('ascii'))
        qual.extend(int(q) for q in read.query_qualities)
    dtypes = dict(reference_start=np.int32, compressed_cb=np.int32, compressed_ub=np.int32, p_misaligned=np.float64,
                  alignment_score=np.int32, cigar_begin=np.int64, n_cigar=np.int32, seq_begin=np.int64, l_seq=np.int32)
    arrays = {name: np.asarray(values, dtype=dtypes[name]) for name, values in columns.items()}
    arrays.update(cigar=np.asarray(cigar, dtype=np.uint32), seq=np.asarray(seq, dtype=np.uint8), qual=np.asarray(qual, dtype=np.uint8))
    return arrays, calls.molecules[:calls.n_molecules].copy(), calls.snp_calls[:calls.n_snp_calls].copy()


def store(out, i, chromosome, arrays, positions, molecules, snp_calls):
    for name, value in arrays.items():
        out[f'c{i}_{name}'] = value
    out[f'c{i}_positions'] = np.asarray(positions, dtype=np.int32)
    out[f'c{i}_molecules'] = molecules
    out[f'c{i}_snp_calls'] = snp_calls
    print(f'  {chromosome}: {len(arrays["reference_start"])} reads, {len(positions)} positions, {len(molecules)} molecules, '
          f'{len(snp_calls)} calls')


def finish(name, out, chromosomes):
    out['chroms'] = np.asarray(chromosomes, dtype=str)
    save(name, out)
    assert os.path.getsize(os.path.join(HERE, name)) < MAX_BYTES, name


def synthetic_case(ref, ref_tests):
    """(a) the reference's generate_bam_file with seed 42, as F1; the reads of every fifth barcode (the file must stay small)."""
    import pysam
    np.random.seed(42)
    filename, genotypes, _ids, bc2names = ref_tests.generate_bam_file(filename='/tmp/golden_count_fixture.bam')
    handler = ref.BarcodeHandler(list(bc2names))
    subset = set(handler.ordered_barcodes[::5])
    bam = pysam.AlignmentFile(filename)
    out, chromosomes = {}, []
    for i, (chromosome, positions) in enumerate(genotypes.get_chromosome2positions().items()):
        reads = [read for read in bam.fetch(chromosome) if read.get_tag('CB') in subset]
        arrays, molecules, snp_calls = scan(ref, reads, chromosome, positions, handler, ref.cellranger_specific.parse_read)
        store(out, i, chromosome, arrays, positions, molecules, snp_calls)
        chromosomes.append(chromosome)
    out['barcodes'] = np.asarray(handler.ordered_barcodes, dtype=str)
    finish('f9_count_synthetic.npz', out, chromosomes)


def example_case(ref):
    """(b) the reference's shipped example BAM (decoded by the stand-in) at the positions of the example VCF."""
    import pysam
    data = f'{REFERENCE}/examples/example_data'
    genotypes = ref.ProbabilisticGenotypes(genotype_names=['Donor01', 'Donor02', 'Donor03', 'Donor04'])
    genotypes.add_vcf(f'{data}/test_genotypes.vcf')
    handler = ref.BarcodeHandler.from_file(f'{data}/test_barcodes.csv')
    bam = pysam.AlignmentFile(f'{data}/test_bamfile.bam')
    out, chromosomes = {}, []
    stride = 1
    while True:
        out, chromosomes = {}, []
        for i, (chromosome, positions) in enumerate(genotypes.get_chromosome2positions().items()):
            reads = list(bam.fetch(chromosome))[::stride]
            arrays, molecules, snp_calls = scan(ref, reads, chromosome, positions, handler, ref.cellranger_specific.parse_read)
            store(out, i, chromosome, arrays, positions, molecules, snp_calls)
            chromosomes.append(chromosome)
        out['chroms'] = np.asarray(chromosomes, dtype=str)
        save('f9_count_example.npz', out)
        if os.path.getsize(os.path.join(HERE, 'f9_count_example.npz')) < MAX_BYTES:
            break
        stride += 1  # every stride-th read of the file: still sorted, still the reference's output for exactly these reads
    print('  example: every', stride, 'th read')


def adversarial_case(ref):
    """(c) a hand-built chromosome with every special case of the contract (tests/count_reads_restatement.py: REQUIRED_CASES)."""
    import pysam
    positions = [10, 20, 30, 45, 60, 75, 1200, 1210, 2500, 2510, 4000, 4010, 4020]
    ops = {'M': 0, 'I': 1, 'D': 2, 'N': 3, 'S': 4, 'H': 5, 'P': 6, '=': 7, 'X': 8}

    def read(start, cigar, cb, ub, letters=(), score=-2, quals=(), nh=1, mapq=255):
        """letters / quals: {index in the read: letter / quality}; everything else 'A' and 30."""
        a = pysam.AlignedSegment()
        a.reference_start = start
        a.cigar = tuple((ops[c[-1]], int(c[:-1])) for c in cigar.split())
        length = sum(n for op, n in a.cigar if op in (0, 1, 4, 7, 8))
        seq, qual = ['A'] * length, [30] * length
        for index, letter in dict(letters).items():
            seq[index] = letter
        for index, q in dict(quals).items():
            qual[index] = q
        a.query_sequence = ''.join(seq)
        a.query_qualities = np.asarray(qual, dtype=np.int64)
        a.mapping_quality = mapq
        a.tags = tuple(t for t in (('NH', nh), ('AS', length + score), ('CB', cb), ('UB', ub)) if t[1] is not None)
        return a

    one, two, three = 'AAAC-1', 'CCGT-1', 'GGTA-1'
    reads = [
        # molecule (one, ACGTA): soft clips, an insertion; then a deletion and a hard clip over the same positions
        read(0, '5S 30M 2I 20M 3S', one, 'ACGTA', letters={15: 'A', 25: 'G', 37: 'C', 52: 'N'}, quals={25: 45, 52: 20}),
        read(5, '20M 10D 20M 4H', one, 'ACGTA', letters={5: 'C', 15: 'T', 30: 'N'}, quals={15: 0, 30: 20}),
        read(5, '20M 10D 20M 4H', one, 'ACGTA', letters={5: 'T', 15: 'T', 30: 'G'}),            # a complete duplicate: skipped
        read(5, '20M 10D 20M 4H', one, 'ACGTA', letters={5: 'G', 15: 'G', 30: 'N'}, score=-3, quals={5: 2}),  # other AS: counted
        read(7, '30M', one, 'ACGTA', nh=2),                      # dropped: several hits
        read(8, '30M', one, None),                               # dropped: no molecule barcode
        read(9, '30M', 'TTTT-1', 'ACGTA'),                       # dropped: barcode not listed
        read(9, '30M', one, 'ACGTA', mapq=10),                   # dropped: mapping quality
        read(9, '30M', one, 'ACGTA', score=-8),                  # dropped: too many edits
        # molecule (two, CCCCC): both positions conflict at equal quality -> no call, no molecule
        read(50, '30M', two, 'CCCCC', letters={10: 'A', 25: 'G'}),
        read(52, '30M', two, 'CCCCC', letters={8: 'C', 23: 'T'}),
        # (three, GGGGG): this molecule is flushed by the event at 1190 ...
        read(55, '20= 10X', three, 'GGGGG', letters={5: 'T', 20: 'C'}),
        # (one, TTTTT): an event (the read at 2005) falls between its reads without flushing it
        read(1190, '30M', one, 'TTTTT', letters={10: 'G', 20: 'C'}, quals={10: 41, 20: 60}),
        read(2005, '10M 490N 20M 2P', two, 'AAAAA', letters={15: 'T'}),
        read(2100, '30M', one, 'TTTTT'),
        # ... and (three, GGGGG) comes back as a second molecule
        read(2480, '50M', three, 'GGGGG', letters={20: 'A', 30: 'C'}, quals={20: 40, 30: 39}),
        read(2485, '50M', three, 'GGGGG', letters={15: 'G', 25: 'C'}, quals={15: 3}),  # 2500: A at 40 against G at 3: resolved
        # (two, AAAAA) again beyond the 1000-base rule: another molecule
        read(4000, '25M', two, 'AAAAA', letters={0: 'N', 10: 'T', 20: 'G'}, quals={0: 7}),
    ]
    handler = ref.BarcodeHandler([one, two, three])
    parse_read = ref.cellranger_specific.parse_read
    arrays, molecules, snp_calls = scan(ref, reads, 'chrA', positions, handler, parse_read)

    from tests.count_reads_restatement import REQUIRED_CASES, special_cases
    found = special_cases(arrays, positions)
    print('  cases:', found)
    missing = [case for case in REQUIRED_CASES if not found.get(case)]
    assert not missing, missing
    out = {}
    store(out, 0, 'chrA', arrays, positions, molecules, snp_calls)
    # every read of the list, kept or not, as the columns parse_read and the barcode handler look at, with their answers
    parsed = [parse_read(r) for r in reads]
    out['raw_l_seq'] = np.asarray([len(r.seq) for r in reads], dtype=np.int32)
    out['raw_alignment_score'] = np.asarray([r.get_tag('AS') for r in reads], dtype=np.int32)
    out['raw_nh'] = np.asarray([r.get_tag('NH') for r in reads], dtype=np.int32)
    out['raw_mapq'] = np.asarray([r.mapq for r in reads], dtype=np.int32)
    out['raw_ub'] = np.asarray([r.get_tag('UB') if r.has_tag('UB') else '' for r in reads], dtype=str)
    out['raw_cb'] = np.asarray([r.get_tag('CB') for r in reads], dtype=str)
    out['raw_parsed'] = np.asarray([p is not None for p in parsed], dtype=bool)
    out['raw_parsed_p'] = np.asarray([p[0] if p else -1.0 for p in parsed], dtype=np.float64)
    out['raw_parsed_ub'] = np.asarray([p[1] if p else -1 for p in parsed], dtype=np.int64)
    cb = [handler.get_barcode_index(r) for r in reads]
    out['raw_barcode_index'] = np.asarray([-1 if c is None else c for c in cb], dtype=np.int64)
    out['barcodes'] = np.asarray(handler.ordered_barcodes, dtype=str)
    strings = ['', 'A', 'ACGT', 'TTTTTTTTTT', 'ACGTACGTACGTACGTACGTACGTACGT', 'N' * 40, 'acgt-1']
    out['hash_strings'] = np.asarray(strings, dtype=str)
    out['hash_values'] = np.asarray([ref.utils.hash_string(s) for s in strings], dtype=np.int64)
    finish('f9_count_adversarial.npz', out, ['chrA'])


def main():
    ref, ref_tests = import_reference()
    import demuxalot.cellranger_specific  # noqa: F401  (ref.cellranger_specific)
    adversarial_case(ref)
    synthetic_case(ref, ref_tests)
    example_case(ref)


if __name__ == '__main__':
    main()
