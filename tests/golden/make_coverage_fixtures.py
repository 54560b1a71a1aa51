"""
tests/golden/make_coverage_fixtures.py -- regenerates the coverage / candidate vectors tests/golden/f10_coverage_*.npz.

Runs ONLY where the reference package can be imported (make_fixtures.py: import_reference, with its in-memory pysam
stand-in).  The stand-in has no count_coverage, and pysam itself is not available where this runs: snp_detection's own
`pysam` name gets an AlignmentFile whose count_coverage is written here to the contract of DESIGN.md "Coverage and
candidates" (the pattern of make_snp_fixtures.py: patch_bam_side).  So the recorded coverage COUNTS pin the contract, not
pysam; what the reference itself contributes is everything behind them: the candidate positions its
detect_snps_for_chromosome handed to count_snps (captured there), and the result of its detect_snps_positions with its real
count_snps.  Only data is stored: the reads that pass parse_read as DecodedReads arrays (compressed_cb -1 where the barcode is
not whitelisted), the coverage, the candidates, the end-to-end results.

    python tests/golden/make_coverage_fixtures.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402
from make_snp_fixtures import canonical, no_tie_decides  # noqa: E402

MAX_BYTES = 1 << 20
CHROMS = ('chr1', 'chr2', 'chr3')
LENGTH = 1000
# (minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage, minimum_fraction_of_ref_and_alt)
THRESHOLDS = ((10, 0.01, 2, 0.98), (5, 0.01, 1, 0.98), (20, 0.01, 4, 0.98), (10, 0.25, 2, 0.9))
WINDOWS = (('chr1', 300, 700), ('chr2', 650, 1000))  # start > 0: the reference returns window-relative indices
# (threshold set, n_best_snps_per_donor, n_additional_best_snps, ignore_known_snps)
END_TO_END = ((0, 20, 50, True), (1, 5, 10, False))
PER_READ = ('reference_start', 'compressed_cb', 'compressed_ub', 'p_misaligned', 'alignment_score', 'cigar_begin', 'n_cigar',
            'seq_begin', 'l_seq')


def count_coverage(reads, start, stop, quality_threshold=15, read_callback=None):
    """The contract's coverage over pysam-like reads: rows A, C, G, T; aligned pairs as pysam forms them (operations 0, 7, 8
    advance both cursors, 1 and 4 the read, 2 and 3 the reference, 5 and 6 neither)."""
    counts = np.zeros((4, stop - start), dtype=np.int64)
    for read in reads:
        if read_callback is not None and not read_callback(read):
            continue
        q, r = 0, read.reference_start
        for op, length in read.cigartuples:
            if op in (0, 7, 8):
                for k in range(length):
                    if start <= r + k < stop and (quality_threshold == 0 or read.query_qualities[q + k] >= quality_threshold):
                        row = 'ACGT'.find(read.seq[q + k])
                        if row >= 0:
                            counts[row, r + k - start] += 1
                q, r = q + length, r + length
            elif op in (1, 4):
                q += length
            elif op in (2, 3):
                r += length
            else:
                assert op in (5, 6), op
    return tuple(counts)


def patch_coverage(sd, standin):
    """snp_detection's own `pysam` name only: the stand-in's AlignmentFile with the count_coverage above."""
    class AlignmentFile(standin.AlignmentFile):
        def count_coverage(self, contig, start=None, stop=None, quality_threshold=15, read_callback=None):
            return count_coverage(self.fetch(contig), start, stop, quality_threshold, read_callback)

    sd.pysam = types.SimpleNamespace(AlignmentFile=AlignmentFile)


def decoded_arrays(reads, handler, parse_read):
    """DecodedReads arrays of the reads parse_read accepts, in fetch order; compressed_cb -1: barcode not whitelisted."""
    columns = {name: [] for name in PER_READ}
    cigar, seq, qual = [], [], []
    for read in reads:
        parsed = parse_read(read)
        if parsed is None:
            continue
        cb = handler.get_barcode_index(read)
        p_misaligned, ub = parsed
        for name, value in (('reference_start', read.reference_start), ('compressed_cb', -1 if cb is None else cb),
                            ('compressed_ub', ub), ('p_misaligned', p_misaligned), ('alignment_score', read.get_tag('AS')),
                            ('cigar_begin', len(cigar)), ('n_cigar', len(read.cigartuples)), ('seq_begin', len(seq)),
                            ('l_seq', len(read.seq))):
            columns[name].append(value)
        cigar.extend((length << 4) | op for op, length in read.cigartuples)
        seq.extend(read.seq.encode('ascii'))
        qual.extend(int(q) for q in read.query_qualities)
    dtypes = dict(reference_start=np.int32, compressed_cb=np.int32, compressed_ub=np.int32, p_misaligned=np.float64,
                  alignment_score=np.int32, cigar_begin=np.int64, n_cigar=np.int32, seq_begin=np.int64, l_seq=np.int32)
    arrays = {name: np.asarray(values, dtype=dtypes[name]) for name, values in columns.items()}
    arrays.update(cigar=np.asarray(cigar, dtype=np.uint32), seq=np.asarray(seq, dtype=np.uint8), qual=np.asarray(qual, dtype=np.uint8))
    return arrays


def captured_candidates(sd, filename, chrom, start, stop, handler, parse_read, thresholds, **extra):
    """The positions the reference's detect_snps_for_chromosome handed to count_snps, as it handed them."""
    seen = {}

    def count_snps(bamfile_location, chromosome2positions, **_kw):
        (seen['positions'],) = chromosome2positions.values()
        return {}  # "no calls": detect_snps_for_chromosome returns []

    original = sd.count_snps
    sd.count_snps = count_snps
    try:
        minimum_coverage, alternative_fraction, alternative_coverage, fraction_of_both = thresholds
        result = sd.detect_snps_for_chromosome(filename, chrom, start, stop, sorted_donors=[], barcode2donor={}, parse_read=parse_read,
                                               barcode_handler=handler, regularization=3., minimum_coverage=minimum_coverage,
                                               minimum_alternative_fraction=alternative_fraction,
                                               minimum_alternative_coverage=alternative_coverage,
                                               minimum_fraction_of_ref_and_alt=fraction_of_both, **extra)
    finally:
        sd.count_snps = original
    assert result == []
    return np.asarray(seen['positions'], dtype=np.int64)


def alt_counts(coverage):
    return np.sort(np.asarray(coverage, dtype=np.int64), axis=0)[-2]


def synthetic_case(ref, ref_tests, sd, seed):
    import pysam
    np.random.seed(seed)
    filename, truth, _ids, bc2names = ref_tests.generate_bam_file(filename='/tmp/coverage_fixture.bam', n_genotypes=4, n_barcodes=60,
                                                                  mutation_prob=0.04, n_reads_per_barcode=20, read_length=40)
    barcodes = list(bc2names)
    handler = ref.BarcodeHandler(barcodes[:52])  # the reads of eight barcodes pass parse_read but are not whitelisted
    parse_read = ref.cellranger_specific.parse_read
    bam = pysam.AlignmentFile(filename)
    out = {'chroms': np.asarray(CHROMS, dtype=str), 'length': np.int64(LENGTH), 'barcodes': np.asarray(handler.ordered_barcodes, dtype=str)}

    # ---- reads and coverage
    from tests import coverage_restatement as restatement
    coverage = {}
    for i, chrom in enumerate(CHROMS):
        arrays = decoded_arrays(bam.fetch(chrom), handler, parse_read)
        assert (arrays['compressed_cb'] < 0).any() and (arrays['compressed_cb'] >= 0).any()
        for name, value in arrays.items():
            out[f'r{i}_{name}'] = value
        coverage[chrom] = np.asarray(count_coverage(bam.fetch(chrom), 0, LENGTH, 15, lambda read: parse_read(read) is not None), dtype=np.int32)
        assert np.array_equal(coverage[chrom], restatement.coverage(arrays, 0, LENGTH, 15))  # two writings of one contract
        out[f'cov{i}'] = coverage[chrom]

    # ---- candidates: what the reference handed to count_snps
    out['thresholds'] = np.asarray(THRESHOLDS, dtype=np.float64)
    sizes = []
    for s, thresholds in enumerate(THRESHOLDS):
        for i, chrom in enumerate(CHROMS):
            out[f'cand{s}_c{i}'] = captured_candidates(sd, filename, chrom, 0, LENGTH, handler, parse_read, thresholds)
            sizes.append(len(out[f'cand{s}_c{i}']))
    if min(sizes) == 0 or max(sizes) >= LENGTH:  # both outcomes of the filter, everywhere
        return None
    # a small cap on a boundary between distinct alt values: no tie sits on the cut
    alt = alt_counts(coverage[CHROMS[0]])[out['cand0_c0']]
    distinct = np.unique(alt)
    if len(distinct) < 3:
        return None
    cap = int((alt >= distinct[len(distinct) // 2]).sum())
    assert 0 < cap < len(alt)
    assert np.sort(alt)[-cap] > np.sort(alt)[-cap - 1], 'a tie on the cut'
    out['cap'] = np.int64(cap)
    out['capped_c0'] = captured_candidates(sd, filename, CHROMS[0], 0, LENGTH, handler, parse_read, THRESHOLDS[0], max_snp_candidates=cap)
    assert len(out['capped_c0']) == cap
    out['windows'] = np.asarray([(CHROMS.index(chrom), start, stop) for chrom, start, stop in WINDOWS], dtype=np.int64)
    for w, (chrom, start, stop) in enumerate(WINDOWS):
        out[f'window{w}'] = captured_candidates(sd, filename, chrom, start, stop, handler, parse_read, THRESHOLDS[0])  # as returned: relative
        assert len(out[f'window{w}']) and out[f'window{w}'].max() < stop - start

    # ---- end to end: the reference's detect_snps_positions with its real count_snps; part of the true SNPs is hidden
    rng = np.random.default_rng(seed)
    true_positions = sorted(truth.get_snp_positions_set())
    hidden = rng.random(len(true_positions)) < 0.4
    known = {k for k, h in zip(true_positions, hidden) if not h}
    genotypes = ref.ProbabilisticGenotypes(truth.genotype_names)
    rows = [(key, row) for key, row in truth.var2varid.items() if key[:2] in known]
    genotypes.var2varid = {key: i for i, (key, _row) in enumerate(rows)}
    genotypes.variant_betas = np.array(truth.variant_betas[[row for _key, row in rows]], dtype=np.float32)
    keys = list(genotypes.var2varid.items())
    out['var_chrom'] = np.asarray([k[0] for k, _ in keys], dtype=str)
    out['var_pos'] = np.asarray([k[1] for k, _ in keys], dtype=np.int64)
    out['var_base'] = np.asarray([mf.BASES[k[2]] for k, _ in keys], dtype=np.uint8)
    out['var_row'] = np.asarray([row for _, row in keys], dtype=np.int32)
    out['betas'] = np.array(genotypes.variant_betas[:genotypes.n_variants], dtype=np.float32)
    out['genotype_names'] = np.asarray(genotypes.genotype_names, dtype=str)
    out['default_prior'] = np.float64(genotypes.default_prior)
    out['end_to_end'] = np.asarray(END_TO_END, dtype=np.int64)
    seen = []
    select_top_snps = sd._select_top_snps

    def recording_select(chrom_pos_importances, n_additional, n_best):
        seen.append(chrom_pos_importances)
        return select_top_snps(chrom_pos_importances, n_additional, n_best)

    sd._select_top_snps = recording_select
    try:
        for e, (s, n_best, n_add, ignore) in enumerate(END_TO_END):
            minimum_coverage, alternative_fraction, alternative_coverage, _default = THRESHOLDS[s]
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, 'prior.parquet')
                result = sd.detect_snps_positions(filename, genotypes, handler, minimum_coverage=minimum_coverage,
                                                  minimum_alternative_fraction=alternative_fraction,
                                                  minimum_alternative_coverage=alternative_coverage, n_best_snps_per_donor=n_best,
                                                  n_additional_best_snps=n_add, joblib_n_jobs=1, joblib_verbosity=0,
                                                  result_beta_prior_filename=path, ignore_known_snps=bool(ignore))
                index = pd.read_parquet(path).index.to_frame()
            importances = np.stack([imp for _, _, imp, _ in seen[-1]])
            if not no_tie_decides(importances, n_best, n_add) or len(result) == 0:
                return None
            result = canonical(result, list(CHROMS))
            out[f'detect{e}_n_scored'] = np.int64(len(seen[-1]))
            out[f'detect{e}_chrom'] = np.asarray([CHROMS.index(c) for c, *_ in result], dtype=np.int32)
            out[f'detect{e}_pos'] = np.asarray([int(p) for _, p, *_ in result], dtype=np.int32)
            out[f'detect{e}_importances'] = np.stack([imp for _, _, imp, _ in result]).astype(np.float64)
            out[f'detect{e}_bases'] = np.asarray([''.join(bc) for *_, bc in result], dtype=str)
            out[f'detect{e}_totals'] = np.asarray([list(bc.values()) for *_, bc in result], dtype=np.int64)
            out[f'detect{e}_parquet_chrom'] = np.asarray(index['CHROM'], dtype=str)
            out[f'detect{e}_parquet_pos'] = np.asarray(index['POS'], dtype=np.int64)
            out[f'detect{e}_parquet_base'] = np.asarray(index['BASE'], dtype=str)
    finally:
        sd._select_top_snps = select_top_snps
    print('seed', seed, 'candidates', sizes, 'cap', cap, 'windows', [len(out[f'window{w}']) for w in range(len(WINDOWS))],
          'scored / selected', [(int(out[f'detect{e}_n_scored']), len(out[f'detect{e}_pos'])) for e in range(len(END_TO_END))])
    return out


def main():
    ref, ref_tests = mf.import_reference()
    import demuxalot.cellranger_specific  # noqa: F401  (ref.cellranger_specific)
    import demuxalot.snp_detection as sd
    import pysam
    patch_coverage(sd, pysam)
    for seed in range(7, 57):
        out = synthetic_case(ref, ref_tests, sd, seed)
        if out is not None:
            mf.save('f10_coverage_synthetic.npz', out)
            assert os.path.getsize(os.path.join(HERE, 'f10_coverage_synthetic.npz')) < MAX_BYTES
            break
    else:
        raise SystemExit('no seed meets the conditions (a tie on a cut, or a filter with one outcome only)')


if __name__ == '__main__':
    main()
