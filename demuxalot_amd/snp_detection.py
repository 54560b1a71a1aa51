"""Detection of new SNPs: the compute half of the reference's detect_snps_positions (demuxalot/snp_detection.py:32-125,
128-242) on the GPU.  Stage 1 - the per-base coverage of every read, the ref / alt filter and the max_snp_candidates cut
(include/demux_hip.h "Coverage", csrc/coverage.hip) - gives the candidate positions from decoded reads; counting, scoring and
selection (include/demux_hip.h "SNP detection", csrc/snp_detect.hip) work on the calls at those positions.
detect_snps_positions_from_reads runs the whole chain from DecodedReads; reading and decompressing BAM files stays with the
caller.

Contract of the coverage and the candidates (what differs from the reference is marked; DESIGN.md "Coverage and candidates"):
  * the coverage is pysam's count_coverage with a read callback: every read counts, aligned pairs as pysam forms them (H and
    P move neither cursor), a base counts when its quality is >= quality_threshold (or the threshold is 0) and its letter is
    exactly one of A C G T
  * ref / alt are the largest / second largest count of a position; the four comparisons of snp_detection.py:46-50 in float64
  * more candidates than max_snp_candidates: those with the largest alt, a tie at the cut going to the HIGHER position (the
    reference's unstable argsort leaves it to chance)
  * positions are ABSOLUTE, start + index (for a fragment with start > 0 the reference hands window-relative indices to
    count_snps: a bug that is not repeated)
  * negative minimum_coverage / minimum_alternative_coverage, max_snp_candidates < 1 and non-finite thresholds raise
    ValueError (they would let the reference's tail pick positions that are no candidates)
  * DecodedReads by contract hold the reads with a whitelisted barcode only, while the reference's stage 1 filters by
    parse_read alone: pass the larger set as coverage_reads to repeat that

Contract of scoring and selection (what differs from the reference is marked):
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
from .snp_counter import DecodedReads, ResidentCalls, ResidentReads, _on, count_snps_from_reads, split_call_sets

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
    if split_call_sets(candidate_calls, 'candidate_calls'):  # views of the sets (this or another context of the device): no upload
        views = [(k, calls._view(ctx.device)) for k, calls in enumerate(candidate_calls.values())]
        n_positions = ctx.snp_count_device(views, donor_of_barcode, len(sorted_donors), P_BASE_WRONG_BELOW, int(cap))
    else:
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
        count_snps returns), or -> ResidentCalls (all of them: the records are read where they lie)
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
    device context.  known_calls and candidate_calls may (each) be dicts of ResidentCalls."""
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


def _check_candidate_arguments(minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                               minimum_fraction_of_ref_and_alt, max_snp_candidates, max_fragment_step, quality_threshold):
    for name, value in (('minimum_coverage', minimum_coverage), ('minimum_alternative_fraction', minimum_alternative_fraction),
                        ('minimum_alternative_coverage', minimum_alternative_coverage),
                        ('minimum_fraction_of_ref_and_alt', minimum_fraction_of_ref_and_alt)):
        if not np.isfinite(value):
            raise ValueError(f'{name} must be finite, got {value!r}')
    for name, value in (('minimum_coverage', minimum_coverage), ('minimum_alternative_coverage', minimum_alternative_coverage)):
        if value < 0:
            raise ValueError(f'{name} must be >= 0, got {value!r}')
    if int(max_snp_candidates) != max_snp_candidates or max_snp_candidates < 1:
        raise ValueError(f'max_snp_candidates must be a positive integer, got {max_snp_candidates!r}')
    if int(max_fragment_step) != max_fragment_step or max_fragment_step < 1:
        raise ValueError(f'max_fragment_step must be a positive integer, got {max_fragment_step!r}')
    if int(quality_threshold) != quality_threshold or not 0 <= quality_threshold <= 255:
        raise ValueError(f'quality_threshold must be an integer 0 .. 255, got {quality_threshold!r}')


def _check_cigar_ranges(reads):
    first, last = reads.cigar_begin, reads.cigar_begin + reads.n_cigar
    if reads.n_reads and (reads.n_cigar.min() < 0 or first.min() < 0 or last.max() > len(reads.cigar)):
        raise ValueError("a read's cigar range lies outside the cigar array")


def reference_ends(reads):
    """int64 reference_end of every read of a DecodedReads: start + the operations that advance the reference (0, 2, 3, 7, 8).
    On the host; a ResidentReads knows the largest of them from the device (reference_length)."""
    _check_cigar_ranges(reads)
    cigar = reads.cigar
    first, last = reads.cigar_begin, reads.cigar_begin + reads.n_cigar
    advances = np.isin(cigar & 15, (0, 2, 3, 7, 8)) * (cigar >> 4).astype(np.int64)
    consumed = np.concatenate([[0], np.cumsum(advances, dtype=np.int64)])
    return reads.reference_start.astype(np.int64) + consumed[last] - consumed[first]


def coverage_from_reads(reads, start, stop, *, quality_threshold=15, on_context=None):
    """The counterpart of pysam's AlignmentFile.count_coverage(chromosome, start, stop, quality_threshold, read_callback) on
    the reads of one chromosome: int32[4, stop - start], rows A, C, G, T (the contract is in the module docstring).

    :param reads: DecodedReads of the chromosome (reference_start non-decreasing), or a ResidentReads (nothing is uploaded; the
        call runs on its context)
    :param on_context: a DeviceContext to run on (the caller holds it); default: the shared context, under its lock
    """
    if not isinstance(reads, (DecodedReads, ResidentReads)):
        raise TypeError('reads must be a DecodedReads or a ResidentReads')
    if not 0 <= start <= stop:
        raise ValueError(f'the window must satisfy 0 <= start <= stop, got [{start}, {stop})')
    if isinstance(reads, ResidentReads):
        return _on(on_context, lambda ctx: ctx.coverage_count_resident(reads._handle, start, stop, quality_threshold), [reads])
    return _on(on_context, lambda ctx: ctx.coverage_count(reads, start, stop, quality_threshold))


def find_candidate_positions(chromosome2reads, *, minimum_coverage, minimum_alternative_fraction=0.01,
                             minimum_alternative_coverage=100, max_snp_candidates=10000, minimum_fraction_of_ref_and_alt=0.98,
                             max_fragment_step=10_000_000, chromosome2length=None, quality_threshold=15, on_context=None):
    """Stage 1 of detect_snps_for_chromosome (snp_detection.py:32-57) for every fragment of every chromosome: coverage, the
    ref / alt filter, the max_snp_candidates cut, on the device.  The fragments are the reference's (:194-195):
    [k * max_fragment_step, min((k + 1) * max_fragment_step, length)); the cut applies per fragment.

    :param chromosome2reads: dict chromosome -> DecodedReads (reference_start non-decreasing) or ResidentReads.  A DecodedReads
        is uploaded once for all its fragments, as a temporary coverage-only set that is released before the next chromosome
        (the device holds one chromosome and one window at a time); a ResidentReads is counted where it lies.
    :param chromosome2length: dict chromosome -> reference length; default (and for chromosomes it does not list): the largest
        reference_end of the chromosome's reads, found on the device (ResidentReads.reference_length).  For a DecodedReads that
        end is known only once the chromosome is uploaded, so a default length beyond 2^31 - 1 raises its ValueError when the
        run reaches that chromosome, after the ones before it were counted; given lengths, the lengths of ResidentReads and
        cigar ranges outside the array are refused before anything is counted.
    :param on_context: a DeviceContext to run on (the caller holds it); default: the context of the ResidentReads if there are
        any, else the shared context, under its lock
    :return: dict chromosome -> ascending int32 ABSOLUTE positions, in the order of chromosome2reads; a chromosome without
        reads gives an empty array
    """
    if not isinstance(chromosome2reads, dict):
        raise TypeError('chromosome2reads must be a dict chromosome -> DecodedReads')
    _check_candidate_arguments(minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                               minimum_fraction_of_ref_and_alt, max_snp_candidates, max_fragment_step, quality_threshold)

    def checked(chromosome, length):
        if length >= 2 ** 31:
            raise ValueError(f'chromosome {chromosome!r}: length {length} is beyond 2^31 - 1')
        return length

    lengths = {}  # what is known before anything is counted; the others: the temporary set's reference_length
    for chromosome, reads in chromosome2reads.items():
        if not isinstance(reads, (DecodedReads, ResidentReads)):
            raise TypeError(f'chromosome2reads[{chromosome!r}] must be a DecodedReads or a ResidentReads')
        if chromosome2length is not None and chromosome in chromosome2length:
            lengths[chromosome] = checked(chromosome, int(chromosome2length[chromosome]))
        elif isinstance(reads, ResidentReads):
            lengths[chromosome] = checked(chromosome, reads.reference_length)
        elif reads.n_reads == 0:
            lengths[chromosome] = 0
        else:
            _check_cigar_ranges(reads)

    def fragments(ctx, count, length):
        found = [np.zeros(0, dtype=np.int32)]
        for start in range(0, length, int(max_fragment_step)):
            count(start, min(start + int(max_fragment_step), length))
            found.append(ctx.coverage_candidates(minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                                                 minimum_fraction_of_ref_and_alt, int(max_snp_candidates)))
        return np.concatenate(found)

    def run(ctx):
        result = {}
        for chromosome, reads in chromosome2reads.items():
            if reads.n_reads == 0:
                result[chromosome] = np.zeros(0, dtype=np.int32)
            elif isinstance(reads, ResidentReads):
                result[chromosome] = fragments(ctx, lambda start, stop, handle=reads._handle: ctx.coverage_count_resident(
                    handle, start, stop, quality_threshold, fetch=False), lengths[chromosome])
            elif not hasattr(ctx, 'reads_upload'):
                # duck-typed compatibility path: `on_context` may be any object with coverage_count / coverage_candidates (the
                # tests' host restatement is one).  One that keeps no reads is handed the arrays per fragment, and the length
                # comes from the host walk; a DeviceContext never takes this branch.
                length = lengths[chromosome] if chromosome in lengths else checked(chromosome, int(max(0, reference_ends(reads).max())))
                result[chromosome] = fragments(ctx, lambda start, stop, reads=reads: ctx.coverage_count(
                    reads, start, stop, quality_threshold, fetch=False), length)
            else:
                handle = ctx.reads_upload(reads, coverage_only=True)
                try:
                    length = lengths[chromosome] if chromosome in lengths else checked(
                        chromosome, max(0, ctx.reads_info(handle)['reference_length']))
                    result[chromosome] = fragments(ctx, lambda start, stop, handle=handle: ctx.coverage_count_resident(
                        handle, start, stop, quality_threshold, fetch=False), length)
                finally:
                    ctx.reads_release(handle)
        return result

    return _on(on_context, run, list(chromosome2reads.values()))


def detect_snps_positions_from_reads(chromosome2reads, genotypes, barcode_handler, *, minimum_coverage,
                                     minimum_alternative_fraction=0.01, minimum_alternative_coverage=100, max_snp_candidates=10000,
                                     minimum_fraction_of_ref_and_alt=0.98, max_fragment_step=10_000_000, chromosome2length=None,
                                     quality_threshold=15, regularization=3., n_best_snps_per_donor=100,
                                     n_additional_best_snps=1000, max_contribution_to_base_count_from_barcode=3,
                                     ignore_known_snps=True, result_beta_prior_filename=None, coverage_reads=None):
    """detect_snps_positions (snp_detection.py:128-215) from decoded reads:
      1. count_snps_from_reads at the genotypes' positions,
      2. predict_posteriors without doublets, its posteriors left on the GPU, and their assignments(0.8),
      3. find_candidate_positions,
      4. count_snps_from_reads at the candidates,
      5. scoring and selection as in detect_snps_positions_from_calls.
    Steps 2 to 5 run on the posteriors' device context.  Chromosomes are taken in the order of chromosome2reads; a
    chromosome without candidates is left out (the reference's `return []`).
    chromosome2reads and coverage_reads may hold ResidentReads: the three read passes (steps 1, 3 and 4) then run on the sets'
    context and upload nothing, steps 2 and 5 on the posteriors' context.  Both call sets (steps 1 and 4) stay on the device as
    ResidentCalls of the context that counted them, are read from there by steps 2 and 5, and are released before the function
    returns: no call record crosses the link in either direction.

    :param coverage_reads: dict chromosome -> DecodedReads for step 3 when they differ from chromosome2reads.  The reference's
        stage 1 counts every read parse_read accepts, while DecodedReads by contract also drop the reads without a whitelisted
        barcode (INTEGRATION.md "Reads for the coverage pass"); the default counts the coverage over chromosome2reads.
    :return: as select_snps_from_calls
    """
    _check_arguments({}, regularization, n_best_snps_per_donor, n_additional_best_snps, max_contribution_to_base_count_from_barcode)
    _check_candidate_arguments(minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                               minimum_fraction_of_ref_and_alt, max_snp_candidates, max_fragment_step, quality_threshold)
    if coverage_reads is None:
        coverage_reads = chromosome2reads
    # reads that are resident decide where the read passes run; host arrays go to the posteriors' context, as ever
    resident = any(isinstance(reads, ResidentReads) for reads in list(chromosome2reads.values()) + list(coverage_reads.values()))
    call_sets = []  # the ResidentCalls of steps 1 and 4

    def release_call_sets():
        for calls in call_sets:
            calls.close()

    known_calls = count_snps_from_reads(chromosome2reads, genotypes.get_chromosome2positions(), resident_calls=True)
    call_sets.extend(known_calls.values())
    try:
        posteriors = Demultiplexer.predict_posteriors(known_calls, genotypes, barcode_handler, doublet_prior=0.0, on_device=True)
    except BaseException:
        release_call_sets()
        raise
    try:
        ctx = posteriors._ctx
        sorted_donors, donor_of_barcode = _donor_of_barcode(posteriors.assignments(ASSIGNMENT_THRESHOLD), barcode_handler)
        candidates = find_candidate_positions(
            {chromosome: coverage_reads[chromosome] for chromosome in chromosome2reads if chromosome in coverage_reads},
            minimum_coverage=minimum_coverage, minimum_alternative_fraction=minimum_alternative_fraction,
            minimum_alternative_coverage=minimum_alternative_coverage, max_snp_candidates=max_snp_candidates,
            minimum_fraction_of_ref_and_alt=minimum_fraction_of_ref_and_alt, max_fragment_step=max_fragment_step,
            chromosome2length=chromosome2length, quality_threshold=quality_threshold, on_context=None if resident else ctx)
        candidates = {chromosome: positions for chromosome, positions in candidates.items() if len(positions)}
        candidate_calls = count_snps_from_reads(chromosome2reads, candidates, on_context=None if resident else ctx, resident_calls=True)
        call_sets.extend(candidate_calls.values())
        selected = _select_on(ctx, candidate_calls, sorted_donors, donor_of_barcode, regularization, n_best_snps_per_donor,
                              n_additional_best_snps, max_contribution_to_base_count_from_barcode)
    finally:
        release_call_sets()  # (before the posteriors' context goes back to its pool: the candidate sets may live on it)
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
