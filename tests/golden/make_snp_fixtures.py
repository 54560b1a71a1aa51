"""
tests/golden/make_snp_fixtures.py -- regenerates the SNP detection vectors tests/golden/f8_snp_*.npz.

Runs ONLY where the reference package can be imported (make_fixtures.py: import_reference, with its in-memory pysam
stand-in).  It captures the reference's own detect_snps_for_chromosome / _select_top_snps / detect_snps_positions on
the calls at every covered position of a reduced synthetic experiment, with the BAM side patched to serve those calls:
count_snps returns the prepared containers, pysam.AlignmentFile reports a coverage that makes every position a
candidate.  Part of the true SNPs is hidden from the genotypes.  Only data is stored: calls, genotypes, the assignment,
the counts, the importances, the base totals, the selections and the parquet index.

    python tests/golden/make_snp_fixtures.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402

CHROMS = ('chr1', 'chr2', 'chr3')
SETTINGS = ((20, 50, True), (5, 10, False), (100, 1000, True))  # (n_best_snps_per_donor, n_additional_best_snps, ignore_known_snps)


def filtered_calls(ref, calls, keep_positions):
    """The containers restricted to the calls at keep_positions[chrom] (molecule tables unchanged)."""
    from demuxalot.snp_counter import CompressedSNPCalls
    out = {}
    for chrom, c in calls.items():
        sc = c.snp_calls[:c.n_snp_calls]
        sc = sc[np.isin(sc['snp_position'], np.asarray(sorted(keep_positions.get(chrom, ())), dtype=np.int64))]
        cc = CompressedSNPCalls()
        cc.molecules = c.molecules[:c.n_molecules].copy()
        cc.n_molecules = c.n_molecules
        cc.snp_calls = sc.copy()
        cc.n_snp_calls = len(sc)
        out[chrom] = cc
    return out


class _Stat:
    def __init__(self, contig):
        self.contig = contig


def patch_bam_side(sd, known_calls, candidate_calls):
    """count_snps serves the prepared calls; the coverage makes every position a candidate (stage 1 passes all)."""
    def count_snps(bamfile_location, chromosome2positions, barcode_handler, joblib_n_jobs=-1, **_kw):
        if joblib_n_jobs is None:  # stage 2 (detect_snps_for_chromosome)
            (chrom,) = chromosome2positions
            return {chrom: candidate_calls[chrom]}
        return known_calls

    class AlignmentFile:
        def __init__(self, *_a, **_kw):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def count_coverage(self, chrom, start, stop, read_callback=None):
            cov = np.zeros((4, stop - start), dtype=np.int64)
            cov[:2] = 1000
            return cov

        def get_index_statistics(self):
            return [_Stat(c) for c in candidate_calls]

        def get_reference_length(self, chrom):
            return 1000

    sd.count_snps = count_snps
    sd.pysam = types.SimpleNamespace(AlignmentFile=AlignmentFile)  # snp_detection's own name only: the stand-in stays as it is


def canonical(chrom_pos_importances, chroms):
    order = sorted(range(len(chrom_pos_importances)),
                   key=lambda i: (chroms.index(chrom_pos_importances[i][0]), int(chrom_pos_importances[i][1])))
    return [chrom_pos_importances[i] for i in order]


def no_tie_decides(importances, n_best, n_add):
    """True when no tie in the reference's rankings sits on a membership cut (so any tie order selects the same set)."""
    P = len(importances)
    for col in importances.T:
        s = np.sort(col)[::-1]
        if n_best < P and n_best > 0 and s[n_best - 1] == s[n_best]:
            return False
    best_for_donors = np.argsort(-importances, axis=0, kind='stable')[:n_best]
    total = importances.sum(axis=1)
    overall = np.argsort(-total, kind='stable')
    is_new = ~np.isin(overall, best_for_donors)
    cut = np.searchsorted(np.cumsum(is_new), n_add, side='right')
    if 0 < cut < P and total[overall[cut - 1]] == total[overall[cut]]:
        return False
    return True


def capture_positions(out, prefix, cpi, chroms, counts_of):
    out[f'{prefix}_chrom'] = np.asarray([chroms.index(c) for c, *_ in cpi], dtype=np.int32)
    out[f'{prefix}_pos'] = np.asarray([int(p) for _, p, *_ in cpi], dtype=np.int32)
    if counts_of is not None:
        out[f'{prefix}_counts'] = np.stack([counts_of[c][p] for c, p, *_ in cpi]).astype(np.int32)
        out[f'{prefix}_importances'] = np.stack([imp for _, _, imp, _ in cpi]).astype(np.float64)
        out[f'{prefix}_bases'] = np.asarray([['ACGT'.index(b) for b in bc] for *_, bc in cpi], dtype=np.uint8)
        out[f'{prefix}_totals'] = np.asarray([list(bc.values()) for *_, bc in cpi], dtype=np.int64)


def synthetic_case(ref, ref_tests, sd, seed):
    np.random.seed(seed)
    filename, truth, _ids, _bc2names = ref_tests.generate_bam_file(filename='/tmp/snp_fixture.bam', n_genotypes=4, n_barcodes=60,
                                                                   mutation_prob=0.04, n_reads_per_barcode=20, read_length=40)
    handler = ref.BarcodeHandler(list(_bc2names))
    candidate_calls = ref.count_snps(filename, chromosome2positions={c: np.arange(1000) for c in CHROMS}, barcode_handler=handler,
                                     joblib_n_jobs=1, joblib_verbosity=0)
    rng = np.random.default_rng(seed)
    true_positions = sorted(truth.get_snp_positions_set())
    hidden = rng.random(len(true_positions)) < 0.4
    known = {k for k, h in zip(true_positions, hidden) if not h}
    genotypes = ref.ProbabilisticGenotypes(truth.genotype_names)
    rows = [(key, row) for key, row in truth.var2varid.items() if key[:2] in known]
    genotypes.var2varid = {key: i for i, (key, _row) in enumerate(rows)}
    genotypes.variant_betas = np.array(truth.variant_betas[[row for _key, row in rows]], dtype=np.float32)
    keep = {}
    for chrom, pos in known:
        keep.setdefault(chrom, set()).add(pos)
    known_calls = filtered_calls(ref, candidate_calls, keep)
    patch_bam_side(sd, known_calls, candidate_calls)
    chroms = list(candidate_calls)

    _lik, post = ref.Demultiplexer.predict_posteriors(known_calls, genotypes, handler, doublet_prior=0.0)
    barcode2donor = post[post.max(axis=1).gt(0.8)].idxmax(axis=1).to_dict()
    sorted_donors = np.unique([d for d in barcode2donor.values()])
    donor2dindex = {d: i for i, d in enumerate(sorted_donors)}
    cpi, counts_of = [], {}
    for chrom in chroms:
        cpi += sd.detect_snps_for_chromosome('unused.bam', chrom, 0, 1000, sorted_donors, barcode2donor, None, handler, 3.,
                                             minimum_coverage=0, minimum_alternative_fraction=0., minimum_alternative_coverage=0)
        counts_of[chrom] = dict(sd._count_snp_stats_for_donors(candidate_calls[chrom], handler, barcode2donor, donor2dindex))
    importances = np.stack([imp for _, _, imp, _ in cpi])
    for n_best, n_add, _ignore in SETTINGS:
        if not no_tie_decides(importances, n_best, n_add):
            return None

    out = mf.inputs_as_arrays(candidate_calls, genotypes, handler)
    out['true_chrom'] = np.asarray([chroms.index(c) for c, _ in true_positions], dtype=np.int32)
    out['true_pos'] = np.asarray([p for _, p in true_positions], dtype=np.int32)
    out['true_hidden'] = hidden
    out['assign_barcodes'] = np.asarray(list(barcode2donor), dtype=str)
    out['assign_donors'] = np.asarray(list(barcode2donor.values()), dtype=str)
    out['sorted_donors'] = np.asarray(sorted_donors, dtype=str)
    capture_positions(out, 'all', canonical(cpi, chroms), chroms, counts_of)
    out['settings'] = np.asarray(SETTINGS, dtype=np.int64)
    for s, (n_best, n_add, ignore) in enumerate(SETTINGS):
        selected = sd._select_top_snps(cpi, n_add, n_best)
        capture_positions(out, f'sel{s}', canonical(selected, chroms), chroms, None)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'prior.parquet')
            result = sd.detect_snps_positions('unused.bam', genotypes, handler, minimum_coverage=0, minimum_alternative_fraction=0.,
                                              minimum_alternative_coverage=0, n_best_snps_per_donor=n_best,
                                              n_additional_best_snps=n_add, joblib_n_jobs=1, joblib_verbosity=0,
                                              result_beta_prior_filename=path, ignore_known_snps=bool(ignore))
            index = pd.read_parquet(path).index.to_frame()
        result = canonical(result, chroms)
        capture_positions(out, f'detect{s}', result, chroms, None)
        out[f'detect{s}_importances'] = np.stack([imp for _, _, imp, _ in result])
        out[f'detect{s}_bases'] = np.asarray([''.join(bc) for *_, bc in result], dtype=str)
        out[f'detect{s}_totals'] = np.asarray([list(bc.values()) for *_, bc in result], dtype=np.int64)
        # the parquet in the reference's own order (its list order, ref base then alt)
        out[f'detect{s}_parquet_chrom'] = np.asarray(index['CHROM'], dtype=str)
        out[f'detect{s}_parquet_pos'] = np.asarray(index['POS'], dtype=np.int64)
        out[f'detect{s}_parquet_base'] = np.asarray(index['BASE'], dtype=str)
        hidden_set = {k for k, h in zip(true_positions, hidden) if h}
        found = {(c, int(p)) for c, p, *_ in result} & hidden_set
        out[f'detect{s}_recovered'] = np.int64(len(found))
    out['n_hidden'] = np.int64(hidden.sum())
    return out


def edge_case(ref, sd):
    """Hand-made: cap exceeded, p == float32(0.01), tied base totals, unassigned barcodes, fewer positions than n_best;
    once with three donors and once with one."""
    handler = ref.BarcodeHandler([f'BC{i:02}' for i in range(8)])
    p_edge = float(np.float32(0.01))
    # (molecule barcode, position, base, p)
    rows = {
        'chrA': [(0, 10, 0, 0.001)] * 5 + [(1, 10, 1, 0.001)] * 2 + [(2, 10, 1, 0.002), (3, 10, 0, 0.001)]  # cap: 5 -> 3
        + [(0, 20, 2, p_edge), (1, 20, 2, 0.001), (4, 20, 3, 0.001), (2, 20, 2, 0.0099)]  # p == float32(0.01) dropped
        + [(0, 30, 0, 0.001), (1, 30, 1, 0.001), (5, 30, 2, 0.001), (6, 30, 3, 0.001)]   # tied totals, barcodes 5/6/7 unassigned
        + [(7, 40, 1, 0.001), (6, 40, 1, 0.001)],                                         # unassigned only: no position
        'chrB': [(3, 5, 3, 0.001)] * 4 + [(0, 5, 0, 0.001), (4, 7, 1, 0.001), (4, 7, 2, 0.001), (1, 7, 2, 0.001)],
    }
    per_chrom = {}
    for chrom, calls in rows.items():
        mol_cb = [cb for cb, *_ in calls]
        per_chrom[chrom] = (mol_cb, [(m, pos, base, p) for m, (_cb, pos, base, p) in enumerate(calls)])
    candidate_calls = mf.build_calls(ref, per_chrom)
    chroms = list(candidate_calls)
    out = {}
    out.update(mf.inputs_as_arrays(candidate_calls, ref.ProbabilisticGenotypes(['D1']), handler))
    for tag, barcode2donor in (('three', {'BC00': 'Dz', 'BC01': 'Da', 'BC02': 'Dm', 'BC03': 'Da', 'BC04': 'Dz'}),
                               ('one', {'BC00': 'Donly', 'BC02': 'Donly', 'BC04': 'Donly'})):
        sorted_donors = np.unique([d for d in barcode2donor.values()])
        donor2dindex = {d: i for i, d in enumerate(sorted_donors)}
        patch_bam_side(sd, None, candidate_calls)
        cpi, counts_of = [], {}
        for chrom in chroms:
            cpi += sd.detect_snps_for_chromosome('unused.bam', chrom, 0, 1000, sorted_donors, barcode2donor, None, handler, 3.,
                                                 minimum_coverage=0, minimum_alternative_fraction=0., minimum_alternative_coverage=0)
            counts_of[chrom] = dict(sd._count_snp_stats_for_donors(candidate_calls[chrom], handler, barcode2donor, donor2dindex))
        out[f'{tag}_assign_barcodes'] = np.asarray(list(barcode2donor), dtype=str)
        out[f'{tag}_assign_donors'] = np.asarray(list(barcode2donor.values()), dtype=str)
        capture_positions(out, f'{tag}_all', canonical(cpi, chroms), chroms, counts_of)
        selected = sd._select_top_snps(cpi, 1000, 100)  # fewer positions than n_best
        capture_positions(out, f'{tag}_sel', canonical(selected, chroms), chroms, None)
    return out


def main():
    ref, ref_tests = mf.import_reference()
    import demuxalot.snp_detection as sd
    for seed in range(1, 50):
        out = synthetic_case(ref, ref_tests, sd, seed)
        if out is not None:
            print('seed', seed, 'P', len(out['all_pos']), 'D', len(out['sorted_donors']), 'hidden', int(out['n_hidden']),
                  'recovered', [int(out[f'detect{s}_recovered']) for s in range(len(SETTINGS))])
            mf.save('f8_snp_synthetic.npz', out)
            break
    else:
        raise SystemExit('every seed has a tie on a membership cut')
    mf.save('f8_snp_edge.npz', edge_case(ref, sd))


if __name__ == '__main__':
    main()
