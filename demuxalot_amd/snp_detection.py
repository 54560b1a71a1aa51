"""Detection of new SNPs from the calls at candidate positions: the compute half of the reference's
detect_snps_positions (demuxalot/snp_detection.py:78-125, 128-242), with counting, scoring and selection on the GPU
(include/demux_hip.h "SNP detection", csrc/snp_detect.hip).  Reading BAM files - the coverage filter of stage 1 and
count_snps - stays with the caller: the calls come as the containers count_snps produces.

Contract (what differs from the reference is marked):
  * a call counts when p_base_wrong < float32(0.01), its barcode has a donor, and (not in the reference, which raises
    IndexError) base_index < 4; every (barcode, position, base) adds min(calls, max_contribution_to_base_count_from_barcode)
  * importances are the reference's float64 formulas in its operation order; ref = the base of the largest total, alt
    the next, the higher base winning a tie (a stable argsort)
  * positions are in the canonical order: chromosome in the dict's order, then position ascending; every ranking of
    _select_top_snps is stable in that order (the reference's argsort leaves ties to chance); the result lists the
    selected positions in that order
  * no position at all gives an empty list (the reference's np.stack fails)
"""
from collections import defaultdict

import numpy as np
import pandas as pd

from .demux import Demultiplexer, DevicePosteriors
from .device import get_context, shared_context_lock

P_BASE_WRONG_BELOW = np.float32(0.01)  # calls['p_base_wrong'] < 0.01 compares in float32 (snp_detection.py:111)
ASSIGNMENT_THRESHOLD = 0.8             # posterior above which a barcode counts for its donor (snp_detection.py:166)
BASES = 'ACGT'


def _containers(candidate_calls):
    parts = []
    for k, calls in enumerate(candidate_calls.values()):
        parts.append((k, calls.snp_calls[:calls.n_snp_calls], calls.molecules[:calls.n_molecules]))
    return parts


def _donor_of_barcode(barcode2donor, barcode_handler):
    """(sorted donor names, int32[B] donor index of every barcode or -1), as snp_detection.py:111-122, 176 index them."""
    if isinstance(barcode2donor, DevicePosteriors):
        barcode2donor = barcode2donor.assignments(ASSIGNMENT_THRESHOLD)
    if isinstance(barcode2donor, pd.Series):
        barcode2donor = barcode2donor.to_dict()
    if not isinstance(barcode2donor, dict):
        raise TypeError('barcode2donor must be a dict, a pandas Series or a DevicePosteriors')
    sorted_donors = np.unique([donor for donor in barcode2donor.values()])
    donor2index = {donor: d for d, donor in enumerate(sorted_donors)}
    donor_of_barcode = np.full(len(barcode_handler.ordered_barcodes), -1, dtype=np.int32)
    for row, barcode in enumerate(barcode_handler.ordered_barcodes):
        donor = barcode2donor.get(barcode, None)
        if donor is not None:
            donor_of_barcode[row] = donor2index[donor]
    return sorted_donors, donor_of_barcode


def _check_arguments(candidate_calls, regularization, n_best_snps_per_donor, n_additional_best_snps, cap):
    if not isinstance(candidate_calls, dict):
        raise TypeError('candidate_calls must be a dict chromosome -> CompressedSNPCalls')
    for name, value in (('n_best_snps_per_donor', n_best_snps_per_donor), ('n_additional_best_snps', n_additional_best_snps)):
        if int(value) != value or value < 0:
            raise ValueError(f'{name} must be a non-negative integer, got {value!r}')
    if float(cap) != int(cap) or cap < 0 or cap >= 2 ** 31:
        raise ValueError(f'max_contribution_to_base_count_from_barcode must be a non-negative integer, got {cap!r}')
    if not np.isfinite(regularization) or regularization < 0:
        raise ValueError(f'regularization must be finite and >= 0, got {regularization!r}')


def _select_on(ctx, candidate_calls, sorted_donors, donor_of_barcode, regularization, n_best_snps_per_donor,
               n_additional_best_snps, cap):
    if len(sorted_donors) == 0:
        return []
    n_positions = ctx.snp_count(_containers(candidate_calls), donor_of_barcode, len(sorted_donors), P_BASE_WRONG_BELOW, int(cap))
    if n_positions == 0:
        return []
    scored = ctx.snp_score(regularization, fetch_counts=False, fetch_importances=True)
    selected = ctx.snp_select(int(n_best_snps_per_donor), int(n_additional_best_snps))
    chromosomes = list(candidate_calls)
    result = []
    for i in selected:
        ref, alt = scored['bases'][i]
        ref_total, alt_total = scored['base_totals'][i]
        result.append((chromosomes[scored['chrom'][i]], int(scored['pos'][i]), scored['importances'][i].copy(),
                       {BASES[ref]: int(ref_total), BASES[alt]: int(alt_total)}))
    return result


def _finish(selected, genotypes, ignore_known_snps, result_beta_prior_filename):
    if ignore_known_snps and genotypes is not None:  # snp_detection.py:204-210
        snp_positions = genotypes.get_snp_positions_set()
        selected = [snp for snp in selected if (snp[0], snp[1]) not in snp_positions]
    if result_beta_prior_filename is not None:
        export_snps_to_beta(selected, result_beta_prior_filename)
    return selected


def select_snps_from_calls(candidate_calls, barcode_handler, barcode2donor, *, regularization=3., n_best_snps_per_donor=100,
                           n_additional_best_snps=1000, max_contribution_to_base_count_from_barcode=3, genotypes=None,
                           ignore_known_snps=True, result_beta_prior_filename=None):
    """Scores every candidate position per donor and selects the best (snp_detection.py:78-125, 204-227).

    :param candidate_calls: dict chromosome -> CompressedSNPCalls at the candidate positions (what the reference's stage-2
        count_snps returns)
    :param barcode2donor: dict or pandas Series barcode -> donor name, or a DevicePosteriors (its assignments(0.8))
    :param genotypes: with ignore_known_snps, positions these genotypes already hold are dropped from the result
    :return: [(chromosome, position, importances float64[D], {ref base: count, alt base: count})] of the selected positions,
        in the canonical order; D = the donors that have at least one barcode, sorted by name
    """
    _check_arguments(candidate_calls, regularization, n_best_snps_per_donor, n_additional_best_snps,
                     max_contribution_to_base_count_from_barcode)
    sorted_donors, donor_of_barcode = _donor_of_barcode(barcode2donor, barcode_handler)
    if len(sorted_donors) == 0:
        return _finish([], genotypes, ignore_known_snps, result_beta_prior_filename)
    with shared_context_lock:
        selected = _select_on(get_context(), candidate_calls, sorted_donors, donor_of_barcode, regularization, n_best_snps_per_donor,
                              n_additional_best_snps, max_contribution_to_base_count_from_barcode)
    return _finish(selected, genotypes, ignore_known_snps, result_beta_prior_filename)


def detect_snps_positions_from_calls(known_calls, candidate_calls, genotypes, barcode_handler, *, regularization=3.,
                                     n_best_snps_per_donor=100, n_additional_best_snps=1000,
                                     max_contribution_to_base_count_from_barcode=3, ignore_known_snps=True,
                                     result_beta_prior_filename=None):
    """detect_snps_positions (snp_detection.py:128-215) with the BAM reading replaced by calls the caller supplies:
    known_calls at the genotypes' positions (step 1), candidate_calls at the candidate positions (step 2).
    Step 1 is predict_posteriors without doublets; its posteriors stay on the GPU, and the detection runs on the same
    device context."""
    _check_arguments(candidate_calls, regularization, n_best_snps_per_donor, n_additional_best_snps,
                     max_contribution_to_base_count_from_barcode)
    posteriors = Demultiplexer.predict_posteriors(known_calls, genotypes, barcode_handler, doublet_prior=0.0, on_device=True)
    try:
        sorted_donors, donor_of_barcode = _donor_of_barcode(posteriors.assignments(ASSIGNMENT_THRESHOLD), barcode_handler)
        selected = _select_on(posteriors._ctx, candidate_calls, sorted_donors, donor_of_barcode, regularization,
                              n_best_snps_per_donor, n_additional_best_snps, max_contribution_to_base_count_from_barcode)
    finally:
        posteriors.close()
    return _finish(selected, genotypes, ignore_known_snps, result_beta_prior_filename)


def export_snps_to_beta(selected_snps, prior_filename):
    """The column-less parquet of the reference's _export_snps_to_beta (snp_detection.py:230-242): index CHROM, POS, BASE,
    the ref base of every position first, then the alt base.  ProbabilisticGenotypes.add_prior_betas registers them."""
    df = defaultdict(list)
    for chromosome, position, _importances, bases_count in selected_snps:
        for base in bases_count:
            df['CHROM'].append(chromosome)
            df['POS'].append(position)
            df['BASE'].append(base)
    df = pd.DataFrame({name: df[name] for name in ('CHROM', 'POS', 'BASE')})
    if len(df) == 0:
        df = df.astype({'CHROM': object, 'POS': np.int64, 'BASE': object})
    df = df.set_index(['CHROM', 'POS', 'BASE'])
    df.to_parquet(prior_filename)
