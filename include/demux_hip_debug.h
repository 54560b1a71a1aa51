/*
 * demux_hip_debug.h -- test, measurement and tuning surface of libdemux_hip.so.
 *
 * Not what a front-end binds (that is demux_hip.h): the switches that pin the choices the library otherwise
 * makes by itself (E-step level, schedule and form, M-step form), the read-outs of the device-side controller, the emulated
 * multi-GPU wire and the device self-tests of the float32 building blocks.  Used by tests/, bench.py and scripts/; every
 * default is what a production call runs.  Same conventions as demux_hip.h (status codes, caller-owned host arrays).
 */
#ifndef DEMUX_HIP_DEBUG_H
#define DEMUX_HIP_DEBUG_H

#include "demux_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of (variant, genotype) sums the last exact-mode M-step redid in the reference's order (instrumentation). */
int dmx_get_redo_count(dmx_ctx *ctx, int64_t *count);

/* Tile-major form of the M-step (kernels.h: MTileArgs).  Possible when the exact additions are off, G <= 64 and
 * contribution_power > 0: the M-step records are kept once more, sorted by (tile of <= 128 variants, barcode), +8 bytes per
 * call, and the sums are formed in 64-bit FIXED POINT (every contribution, a float32 in [0, 1], added as the integer
 * rint(c 2^s), s = 50 for all but the hottest tiles): independent of the order of the additions, so bit-reproducible from run
 * to run like the reference's np.bincount (utils.py:35-36), exact for contributions of 2^-27 and more, and within one float32
 * ulp + n 2^-(s + 1) (n calls of the variant) of the reference's float64 sum in general.  Building the records is a sort of
 * the calls (2.6 ms on 200k x 100k x 64, where an M-step then takes 0.34 instead of 0.70 ms), so
 *   1 (default) builds them at the first M-step that has 8 or more M-steps still to come - in the running dmx_em /
 *     dmx_run_iterations call, or announced with dmx_set_msteps_expected -, or when the resident problem has seen 8; where the
 *     incremental M-step applies (dmx_set_mstep_incremental: its full passes are made by the work items with the same fixed-point
 *     arithmetic, dmx_get_mstep_form = 3) only once the device's count of full passes, read at the 4th / 16th / 64th M-step,
 *     says that they keep coming;
 *   2 at the first M-step;  0 never (the float64 work-item form).
 * dmx_set_msteps_expected: a hint - the caller will run about n more M-steps on the resident problem (a front-end that drives
 * the iterations call by call, a benchmark that warms up first); counted down as M-steps run.
 * dmx_get_mstep_tiles_info: whether the records exist and the host wall time their build took. */
int dmx_set_mstep_tiles(dmx_ctx *ctx, int enable);
int dmx_get_mstep_tiles_info(dmx_ctx *ctx, int32_t *built, double *build_ms);
/* form of the last M-step launch: 0 none yet, 1 work items (float64 partial sums), 2 tiles, 3 work items adding the tile-major form's
 * integers under the incremental M-step (the dense regime's kernel may still have taken any of them) */
int dmx_get_mstep_form(dmx_ctx *ctx, int32_t *form);
/* The live floor of the barcode codes and the bitmap the E-step leaves for the M-step (csrc/kernels.h: live_floor_fixed).  With
 * contribution_power == 2 a float64 M-step form needs every posterior above 2^-80 in them (below it the float32 contribution is +0);
 * the fixed-point forms (dmx_get_mstep_form 2 and 3, the incremental delta pass) add integers rint(c 2^shift), shift <= 50, and a
 * posterior below 2^-26 adds the integer 0 there.  on_grid = 1 (default): an E-step that a fixed-point M-step will follow - as the
 * M-step's plan says ahead - on a context without a communicator calls a posterior live from 2^-26 on; far fewer barcodes then count
 * as dense or carry extra live posteriors, same sums bit for bit.  The M-step's choice between the dense regime's kernel and the others
 * keeps its own count above 2^-80.  An M-step whose form turns out to be a float64 one rebuilds the codes at 2^-80 first.  on_grid = 0:
 * always 2^-80 (tests, measurements).
 * dmx_get_live_floor: the floor of the current codes, and the rebuild launches of M-steps since dmx_reset_timings (0 in steady state).
 * dmx_debug_get_live_counts: [B] live posteriors of every barcode as its code counts them (G <= 64, after an E-step). */
int dmx_set_live_floor_on_grid(dmx_ctx *ctx, int on_grid);
int dmx_get_live_floor(dmx_ctx *ctx, float *floor, int64_t *rebuilds);
int dmx_debug_get_live_counts(dmx_ctx *ctx, int32_t *counts);

/* Worst case of the guarded mode.  With the fast pass taking F, the exact kernel over every barcode E, and a fraction f of the
 * barcodes queued, a guarded E-step costs F + f E: more than the exact mode's E once f > 1 - F / E, and (F + E) / E on a
 * workload where nothing can be proven.  F / E depends on the workload (0.56 at 200k x 100k x 64, 0.34 at 1M x 650k x 128 with
 * doublets, above 1 on small problems), so the two passes are TIMED on the device (wall-clock stamps between the launches)
 * and - adaptive = 1, the default - the E-step that follows one of the same resident problem and option
 * table for which F + f E > E runs DIRECT: the fast kernels stand back and the exact kernel walks every barcode (results then
 * bit-identical to the reference's on all of them), counting what the guard would have queued, so that the fast pass
 * returns when it pays again (3 % of hysteresis).  Decided on the device between two E-steps, no host synchronisation.  E is
 * first estimated from the redo's time over its share of the barcodes (only when that share is at least 5 %), then measured
 * by the first direct E-step.  An iterated run is then never slower than the exact mode by more than one mispredicted
 * E-step plus the fast kernels' launches standing back (~10 us per E-step); a single E-step (predict_posteriors) has no
 * history and runs the fast pass + redo.  adaptive = 0: always the fast pass + redo.
 * dmx_get_guard_direct: whether the last guarded E-step ran direct, how many did since dmx_reset_timings, the number of
 * barcodes the last one queued (direct: would have queued), and the device's own timings: the fast pass over all barcodes
 * and the exact kernel over all barcodes in ms (0: not known yet; negative: the estimate, not yet measured by a direct
 * E-step); any pointer may be NULL. */
int dmx_set_guard_adaptive(dmx_ctx *ctx, int adaptive);
/* The COARSE pass of the guarded mode (csrc/kernels.hip: k_estep_tiled_coarse).  For singlet runs of 33..64 genotypes under the
 * tile-major schedule, an E-step whose logits nobody can read - every E-step of a dmx_em / dmx_run_iterations call but the
 * last - may read the genotype table as binary16 (half the bytes of every row gather; relative error 2^-11 per term, priced
 * per call by the guard): posteriors of the barcodes it keeps are proven within the contract exactly as in the fine pass,
 * the others are redone by the exact kernel; the LOGITS of such an E-step are only within the guard's bound D (0.2 at 400
 * calls per barcode) of the reference's, which is why the last E-step of a call - the one whose logits dmx_get_logits /
 * dmx_get_block / dmx_em return - never takes it.  Coarse pass, fine pass or the direct form: chosen per E-step on the
 * device from the measured times of the passes and the fractions both guards flag (both are evaluated whichever pass runs).
 * coarse = 0: never (the guarded mode of round 4).  Default 1.  coarse = 2: admissible for EVERY E-step, the last one of a call and
 * dmx_estep included - their logits then carry the bound D (tests and measurements).  dmx_get_guard_levels: level of the last guarded E-step
 * (0 coarse, 1 fine, 2 direct; -1: none), E-steps that took the coarse pass since dmx_reset_timings, barcodes the fine / the
 * coarse guard flagged in the last one (-1: not evaluated; the guard of a pass that did not run is shown one barcode in 8: an
 * estimate), and the device's timings of the three passes over all barcodes
 * in ms (0: not run yet; exact: negative while it is an estimate).  Any pointer may be NULL. */
int dmx_set_coarse_pass(dmx_ctx *ctx, int coarse);

/* Incremental M-step (csrc/kernels.h: MIncrArgs).  The tile-major M-step adds integers, so its sums can be updated exactly: once a
 * full pass has left them on the device, an M-step visits only the barcodes whose posteriors changed where it matters (a posterior
 * below 2^-26 contributes exactly 0 on the sums' grid) and adds the differences of their new and old contributions - a fraction of a
 * percent of the calls on converged iterations.  The additions are the full pass's, bit for bit; the device falls back to the full
 * pass whenever the changed barcodes hold more than an eighth of the calls, the kept sums are not valid (a new problem, dmx_set_addition,
 * the first M-step of a dmx_em call, another M-step form in between) or the posteriors are dense.  Taken where the tile-major form is
 * (dmx_set_mstep_tiles) on one context that holds all calls of its barcodes.  incremental = 0: every M-step the full pass.  Default 1.
 * incremental = 2 (tests, measurements): the first sums too are built by the delta pass, every barcode against an all-zero row - the
 * full pass's bits from another kernel and another walk of the calls, at 20 x its time.
 * dmx_get_mstep_incremental: full and delta passes since dmx_reset_timings, barcodes the last M-step found changed (-1: it had no
 * valid sums to compare with). */
int dmx_set_mstep_incremental(dmx_ctx *ctx, int incremental);
int dmx_get_mstep_incremental(dmx_ctx *ctx, int64_t *full_passes, int64_t *delta_passes, int64_t *barcodes_changed_last);
int dmx_get_guard_levels(dmx_ctx *ctx, int32_t *level_last, int64_t *coarse_steps, int64_t *flagged_fine_last, int64_t *flagged_coarse_last,
                         double *coarse_pass_ms, double *fine_pass_ms, double *exact_pass_ms);
/* The device times a pass only when it runs, so the time of a pass that is not chosen goes stale - and a pass timed once under other
 * conditions (the first E-step on a device that had idled runs at a fraction of its clocks) would not be chosen again because of that
 * time.  After 64 E-steps in a row on one level the cheapest other admissible level runs once, if its standing price is below twice the
 * running one's (csrc/kernels.h: GUARD_PROBE_STREAK).  dmx_get_guard_probes: such E-steps since dmx_reset_timings, the current streak.
 * dmx_debug_set_pass_ms (testing aid): overwrite the device's times of the coarse / fine / exact pass (ms over all barcodes; negative:
 * leave; exact 0: back to "not measured"). */
int dmx_get_guard_probes(dmx_ctx *ctx, int64_t *probes, int64_t *streak);
int dmx_debug_set_pass_ms(dmx_ctx *ctx, double coarse_pass_ms, double fine_pass_ms, double exact_pass_ms);
int dmx_get_guard_direct(dmx_ctx *ctx, int32_t *last_ran_direct, int64_t *direct_steps, int64_t *would_queue_last, double *fast_pass_ms,
                         double *exact_pass_ms);

/* E-step work distribution.  For singlet runs of 17..128 genotypes on at least 8 192 barcodes with a genotype table
 * of 1 MB or more, the problem upload also builds a tile-major schedule (bins of 8 barcodes with equal numbers of
 * calls, walked variant tile by variant tile, so that the wavefronts of an XCD gather genotype rows from the same
 * ~2 MB of the table at any time: csrc/kernels.hip, k_estep_tiled).  tiled = 1 (default): used where it pays, i.e.
 * in the tolerance mode (DMX_ESTEP_FAST), whose time is the row gathers; the exact mode is bound by its arithmetic
 * and keeps one barcode per wavefront.  tiled = 2: used whenever built; tiled = 0: never.  Results of a given
 * E-step mode are bit-identical under every schedule. */
int dmx_set_estep_schedule(dmx_ctx *ctx, int tiled);

/* Dictionary form of the exact E-step (csrc/estep_dict.hip).  Before the first M-step - predict_posteriors
 * (demux.py:120-156) and iteration 0 of learn_genotypes (demux.py:86-101) - a row of genotype_prob holds a handful of
 * distinct float32 values (the importers write betas from {0, s/2, s, 0.1 x mean}: genotypes.py:147-164).  When every
 * row has at most 8 distinct values (singlet runs) or 4 (doublet runs: at most 10 values of (p1 + p2) * 0.5,
 * demux.py:190) numpy's float32 log is evaluated once per (call, distinct value) instead of once per (call, option);
 * every option still receives the same float32 addends in the same order, so logits and posteriors are bit-identical
 * to the direct form's.  mode = 1 (default): the form is tried whenever the table was computed without a beta
 * addition or supplied by the caller, and used when every row fits; 0: never; 2: tried for every E-step.
 * dmx_get_estep_form reports what the last E-step ran. */
#define DMX_FORM_NONE 0
#define DMX_FORM_DIRECT 1   /* one numpy log per (call, option): k_estep_direct / k_estep_tiled / k_estep_block */
#define DMX_FORM_DICT 2     /* dictionary form, lane-per-option kernel */
#define DMX_FORM_DICT_BLOCK 3   /* dictionary form, workgroup-per-barcode kernel (wide doublet tables) */
#define DMX_FORM_PACKED 4   /* one numpy log per (call, option), several option slots per lane (narrow doublet tables:
                               csrc/estep_packed.hip) */
int dmx_set_estep_dictionary(dmx_ctx *ctx, int mode);
int dmx_get_estep_form(dmx_ctx *ctx, int32_t *form, int32_t *distinct_values);

/* Narrow doublet tables in the exact mode (K = G (G + 1) / 2 options that fill a power-of-two lane group badly: K = 36
 * takes 36 of 64 lanes): lane groups of 8 / 16 / 32 lanes with 3 or 5 option slots per lane (csrc/estep_packed.hip).
 * A barcode's calls are added in order, so with A slots per lane its walk is A times longer; the barcodes with more
 * calls than a third of what a SIMD gets on average therefore take 64-lane wavefronts inside the same launch.
 * mode = 1 (default): used where the shape wastes fewer slots than the direct form and at most an eighth of the
 * barcodes are such long ones; 0: never; 2: every barcode on packed lane groups; 3: the split wherever the shape exists.
 * Bit-identical results. */
int dmx_set_estep_packing(dmx_ctx *ctx, int mode);

/* M-step loads (G <= 64).  wide = 0 (default): 32-bit buffer offsets wherever the tables allow (posterior table below
 * 4 GiB, fewer than 2^24 barcodes), 64-bit addresses otherwise.  wide = 1: always 64-bit addresses - the form the
 * largest problems run, selectable so that it can be exercised at any size.  Results are bit-identical. */
int dmx_set_mstep_wide_addresses(dmx_ctx *ctx, int wide);

/* Emulated wire, for MEASURING what of the exchange a schedule leaves exposed on a box with one GPU: this context behaves
 * as rank `rank` of `nranks` - variant slices, padded tables, sliced P-step, every kernel and copy of the real exchange -
 * but the three collectives move nothing between processes: this rank's block is copied to where the collective would leave
 * it, and the stream is then held by a one-wavefront kernel for the modelled wire time, latency_us + block bytes /
 * link_gbytes_per_s per collective (a direct exchange on a fully connected xGMI node: one block per peer link and
 * direction, all links at once).  The other ranks contribute nothing - their slices of genotype_prob keep the table
 * without addition - so the numbers such a run produces are not an EM of any experiment; its TIMINGS are those of one
 * rank of an nranks-GPU run whose wire behaves as modelled (scripts/emulated_scaling.py). */
int dmx_comm_init_emulated(dmx_ctx *ctx, int rank, int nranks, double link_gbytes_per_s, double latency_us, int reduce_dtype);

/* Variant-sharded M-step, G <= 64: the all-gather of the singlet posteriors is COMPACT - a barcode with one live posterior is described
 * by its 8-byte code, which travels anyway, and its row is rebuilt by the receivers; only the rows of the barcodes with several live
 * posteriors travel, in a list of at most capacity_rows per rank (rows_pad / 4; DEMUXALOT_AMD_EXCHANGE_COMPACT=<rows> sets it, =0
 * switches the compact form off).  Every rank reads every rank's count behind the all-gather - the exchange's one host
 * synchronisation - and all fall back to the all-gather of the whole table when a list overflowed.  The additions keep their bits
 * (a posterior that is not live contributes exactly +0).  E-steps exchanged compactly / that fell back, since the context was created. */
int dmx_get_exchange_compact(dmx_ctx *ctx, int64_t *taken, int64_t *overflows, int64_t *capacity_rows);
/* The same for the all-gather of genotype_prob behind the sliced P-step: a rank lists the rows of its slice that changed since it sent
 * them (27 % at the second EM iteration of 200k x 100k x 64, 1 % at the fifth), the receivers - whose copies are what was sent last -
 * write them; capacity slice_rows / 4, the whole slices when a list overflowed or the table was written by somebody else
 * (dmx_set_probs, the first P-step of a layout).  Bit-identical tables.  P-steps exchanged compactly / that fell back. */
int dmx_get_exchange_compact_table(dmx_ctx *ctx, int64_t *taken, int64_t *overflows, int64_t *capacity_rows);

/* ------------------------------------------------------------------------- *
 * Device self-tests of the float32 building blocks (used by tests/ on the GPU box):
 * the device restatements of numpy's float32 log / exp and of scipy's row softmax.
 * ------------------------------------------------------------------------- */
int dmx_test_logf(dmx_ctx *ctx, const float *in, float *out, int64_t n);
/* the form the E-step kernels inline: positive finite arguments only, range-restricted division */
int dmx_test_logf_hot(dmx_ctx *ctx, const float *in, float *out, int64_t n);
int dmx_test_expf(dmx_ctx *ctx, const float *in, float *out, int64_t n);
/* the hardware log2 (v_log_f32) the tolerance / guarded E-step modes take of a product's mantissa */
int dmx_test_log2_hw(dmx_ctx *ctx, const float *in, float *out, int64_t n);
int dmx_test_softmax(dmx_ctx *ctx, const float *in, float *out, int64_t rows, int64_t cols);

/* ------------------------------------------------------------------------- *
 * Read-outs that describe what the library did or loaded, for tests, bench.py and diagnostics; no front-end needs them to
 * run the path (they sat in demux_hip.h until the coverage entry points took their places there: the public header stays
 * at 64 entry points at most).
 * ------------------------------------------------------------------------- */
/* Barcodes the guarded E-steps computed with the exact kernel (the queued ones, or all of them in an E-step that ran direct): in the last E-step, and in all E-steps / out of how many barcode rows since the context was created or
 * dmx_reset_timings (instrumentation; any pointer may be NULL). */
int dmx_get_guard_stats(dmx_ctx *ctx, int64_t *redone_last, int64_t *redone_total, int64_t *rows_total);

/* The exchange the resident problem runs (demux_hip.h "Multi-GPU"): no communicator, or with one attached the M-step sharded on
 * variants / the reduce-scatter of the sums / the all-reduce of the sums (with one rank nothing travels either way). */
#define DMX_EXCHANGE_NONE 0
#define DMX_EXCHANGE_VARIANT 1
#define DMX_EXCHANGE_REDUCE_SCATTER 2
#define DMX_EXCHANGE_ALLREDUCE 3
int dmx_get_exchange_mode(dmx_ctx *ctx, int32_t *mode);

/* Which HIP / RCCL runtime files this process has mapped, one "key=path" per line: hip=... (one line per distinct
 * libamdhip64 - exactly one in a healthy process), rccl_mapped=..., rccl_loaded=<the file dmx_comm_* bound, if any>.
 * RCCL is always taken from the directory of the HIP runtime libdemux_hip.so itself resolved, and dmx_comm_unique_id /
 * dmx_comm_init refuse a process that has two HIP runtimes mapped (e.g. one that imported torch): streams and
 * buffers of one runtime must not be handed to collectives of another.  Environment: DEMUXALOT_AMD_RCCL=<file>,
 * DEMUXALOT_AMD_ALLOW_FOREIGN_RCCL=1. */
int dmx_runtime_info(char *out, int64_t capacity);

/* Streamed read counting (product API, not a debug switch: it is declared here because demux_hip.h is kept to 64 entry points).
 * The reads of one chromosome pushed in chunks, in read order, in device memory bounded by the chunk and the
 * molecules still open (DESIGN.md "Read counting", "Streaming").  One stream per context.
 *   dmx_count_reads_begin  opens the stream: positions and qual_table41 as for dmx_count_reads, uploaded and checked once.
 *   dmx_count_reads_push   counts carry + chunk, where the carry is the reads of the molecules no event has flushed so far.
 *                          A push that is not final emits the molecules an event of this chunk flushes and keeps the reads of
 *                          the others (duplicates included) on the device; the final push (final != 0) emits everything.
 *                          chunk may be NULL or empty.  cigar_begin / seq_begin count from the chunk's own cigar / seq.
 *                          *n_molecules, *n_calls: the records THIS push emitted; dmx_count_reads_fetch returns them, with
 *                          molecule_index counting on across the pushes of the stream.  The pushes' records, concatenated, are
 *                          the records of one dmx_count_reads on all the reads.  The number of reads of a stream is not limited.
 *                          DMX_ERR_INVALID: no stream, a push after the final push or after a failed one, a chunk whose first
 *                          reference_start lies below the previous chunk's last, and whatever dmx_count_reads refuses (errors
 *                          in reads that count are decided when their molecule is emitted).  DMX_ERR_UNSUPPORTED: carry +
 *                          chunk above 2^31 - 1 reads, more than 2^31 - 1 molecules in the stream.  After a failed push the
 *                          stream is dead: the records of its earlier pushes stand for nothing, dmx_count_reads_end is left.
 *   dmx_count_reads_end    closes the stream and drops the carry (the records of the last push stay fetchable).
 *                          dmx_release_problem and dmx_destroy close it too.
 * While a stream is open, dmx_count_reads and a second dmx_count_reads_begin answer DMX_ERR_INVALID. */
int dmx_count_reads_begin(dmx_ctx *ctx, const int32_t *positions, int64_t n_positions, const double *qual_table41);
int dmx_count_reads_push(dmx_ctx *ctx, const dmx_decoded_reads *chunk, int final, int64_t *n_molecules, int64_t *n_calls);
int dmx_count_reads_end(dmx_ctx *ctx);

/* Stage times of the last dmx_count_reads, milliseconds between hipEvents on the ctx stream (scripts/count_reads_timing.py):
 * stage_ms[7] = upload, CIGAR walk + events, molecules, duplicates + p_group_misaligned, observations (emit + sort),
 * per-position folds, order + records (csrc/count_reads.hip). */
int dmx_get_count_reads_timings(dmx_ctx *ctx, double *stage_ms);
/* The same for the last dmx_count_reads_push: upload holds the carry's device-to-device copy as well, order + records the
 * compaction of the next carry.
 * dmx_get_count_reads_carry: reads the last push of the open stream left on the device as the carry (0 without a stream).
 * dmx_get_count_reads_peak_bytes: bytes the last dmx_count_reads or dmx_count_reads_push held at its end, when it holds the
 * most: the temporaries and the input on the device (for a push: carry + chunk, the stream's positions and table, the next
 * carry), as asked of the context's allocator.  For the resident calls ("Resident reads" below): the call's own temporaries
 * and the input it gathered (positions and table; for a push: carry + the gathered range, the next carry) - NOT the set, whose
 * bytes dmx_reads_info reports. */
int dmx_get_count_reads_carry(dmx_ctx *ctx, int64_t *n_reads);
int dmx_get_count_reads_peak_bytes(dmx_ctx *ctx, int64_t *bytes);

/* The accumulation form of dmx_coverage_count (csrc/coverage.hip): no-return global atomics into the dense window, or position
 * tiles in LDS that are stored once (the default: DESIGN.md "Coverage and candidates" has the measurements).  Both give the
 * same integers; the switch exists for scripts/coverage_timing.py and for the tests that compare the two. */
#define DMX_COVERAGE_ATOMIC 0
#define DMX_COVERAGE_TILED 1
int dmx_set_coverage_form(dmx_ctx *ctx, int form);
/* Stage times of the last dmx_coverage_count and dmx_coverage_candidates, milliseconds between hipEvents on the ctx stream
 * (scripts/coverage_timing.py): stage_ms[6] = upload (with clearing the window), CIGAR walk + prefix maximum, window / tile bounds,
 * accumulate; filter + compaction, top-n + emit (0 until dmx_coverage_candidates has run on the window). */
int dmx_get_coverage_timings(dmx_ctx *ctx, double *stage_ms);

/* ------------------------------------------------------------------------- *
 * Resident reads (product API; declared here because demux_hip.h is kept to 64 entry points).
 * The arrays of one dmx_decoded_reads uploaded ONCE into buffers the context owns, named by a handle, and taken by the
 * read-side passes in place of host arrays: counting, coverage and the pushes of a stream then move no read to the device
 * (DESIGN.md "Resident reads").  Several sets may be resident at once (one per chromosome).  A set is read-only to every pass.
 *   dmx_reads_upload    copies the arrays and returns the handle.  It refuses only what the host-array calls refuse before they
 *                       upload (n_reads outside 0 .. 2^31 - 1, negative sizes, null cigar / seq / qual or per-read arrays):
 *                       whether a READ is invalid stays the decision of the pass that consumes it - counting judges the reads
 *                       that count, coverage every read -, with the status the host-array call gives on the same reads.
 *                       compressed_cb, compressed_ub, p_misaligned and alignment_score may be null, as for dmx_coverage_count
 *                       (all four are kept, or none): such a set serves coverage only, counting on it answers
 *                       DMX_ERR_INVALID.  Handles are unique in the process and never reused: a released handle and a handle
 *                       of another context answer DMX_ERR_INVALID everywhere.  The caller's arrays are free when it returns.
 *   dmx_reads_release   frees one set.  dmx_destroy frees what is left; dmx_release_problem does NOT: the sets are the caller's,
 *                       not part of the problem.
 *   dmx_reads_info      info[5] = n_reads, n_cigar_ops, n_bases, device bytes held, the largest reference_end: reference_start
 *                       plus the lengths of the operations 0, 2, 3, 7, 8 (M D N = X; the rule both CIGAR walkers share), found
 *                       on the device at upload; a read whose CIGAR range lies outside the array ends where it starts; 0 for
 *                       no reads.
 *   dmx_count_reads_resident      dmx_count_reads on the set.
 *   dmx_coverage_count_resident   dmx_coverage_count on the set.
 *   dmx_count_reads_push_resident dmx_count_reads_push with the reads [first_read, last_read) of the set as the chunk (cigar_begin
 *                       and seq_begin of a set are arbitrary offsets: the range is gathered behind the carry on the device).
 *                       A bad handle or range (first_read < 0, last_read < first_read, last_read > n_reads) is refused before the
 *                       stream is looked at and leaves it open; every other failure ends the stream as a failed
 *                       dmx_count_reads_push does.
 *   dmx_get_reads_upload_bytes    cumulative bytes of decoded-read arrays this context copied host to device: by
 *                       dmx_reads_upload, dmx_count_reads, dmx_count_reads_push (twelve arrays) and dmx_coverage_count (the
 *                       eight it reads).  Positions and tables are not reads.  The resident calls add nothing.
 * Records, coverage arrays, candidates, status codes and error flags of a resident call are those of the host-array call on
 * the same reads, float fields bit for bit; fetch, candidates, timings, carry and the stream's begin / end are the existing
 * entry points. */
int dmx_reads_upload(dmx_ctx *ctx, const dmx_decoded_reads *reads, int64_t *handle);
int dmx_reads_release(dmx_ctx *ctx, int64_t handle);
int dmx_reads_info(dmx_ctx *ctx, int64_t handle, int64_t *info);
int dmx_count_reads_resident(dmx_ctx *ctx, int64_t handle, const int32_t *positions, int64_t n_positions, const double *qual_table41,
                             int64_t *n_molecules, int64_t *n_calls);
int dmx_coverage_count_resident(dmx_ctx *ctx, int64_t handle, int32_t start, int32_t stop, int32_t quality_threshold,
                                int32_t *coverage_out);
int dmx_count_reads_push_resident(dmx_ctx *ctx, int64_t handle, int64_t first_read, int64_t last_read, int final, int64_t *n_molecules,
                                  int64_t *n_calls);
int dmx_get_reads_upload_bytes(dmx_ctx *ctx, int64_t *bytes);

/* ------------------------------------------------------------------------- *
 * Resident calls (product API; declared here because demux_hip.h is kept to 64 entry points).
 * The two record arrays of one CompressedSNPCalls (one chromosome) held in blocks the context owns, named by a handle, and taken
 * by the pack and by the SNP counts in place of host containers: a run from reads to posteriors, or from reads to selected SNPs,
 * then moves no call record over the link (DESIGN.md "Resident calls").  The records are bytewise the host records: 12-byte
 * molecules, 13-byte snp_calls, unaligned.  A set is OPEN while it is filled and IMMUTABLE once sealed; view, fetch, concatenate
 * and the counts take sealed sets only (an open one answers DMX_ERR_INVALID).  Handles are unique in the process and never
 * reused: a released handle and a handle of another context answer DMX_ERR_INVALID everywhere.  The sets are the caller's:
 * dmx_release_problem leaves them, dmx_destroy frees what is left.  Their blocks are not part of dmx_device_bytes.
 *   dmx_calls_upload          copies the two arrays of a host container and seals the set.  One lane per call checks
 *                             0 <= molecule_index < n_molecules; status and message are those of dmx_stage_containers on the same
 *                             container.  The caller's arrays are free when it returns.
 *   dmx_calls_open            a new, empty, open set.
 *   dmx_calls_append_counted  appends the records of the last dmx_count_reads, dmx_count_reads_resident, dmx_count_reads_push or
 *                             dmx_count_reads_push_resident of this context, device to device (molecule_index counts on across the
 *                             pushes of a stream, so an append is a copy; the blocks grow by doubling).  A push that emitted
 *                             nothing appends nothing.  DMX_ERR_INVALID: a sealed set, no records (none counted, or the last
 *                             count or push failed), records whose molecules do not count on from the set's.
 *   dmx_calls_seal            waits for the stream; from then on the set is read-only.
 *   dmx_calls_concatenate     CompressedSNPCalls.concatenate on the device: a new sealed set, the parts (sealed sets of this
 *                             context) in list order, every part's molecule_index shifted by the molecules before it.
 *                             DMX_ERR_UNSUPPORTED: 2^31 molecules or more in all.
 *   dmx_calls_view            device pointers and sizes of a sealed set (chrom 0), as dmx_stage_device_containers and
 *                             dmx_snp_count_device take them; valid until the set is released.
 *   dmx_calls_info            info[4] = n_molecules, n_snp_calls, device bytes held, sealed (0 / 1).
 *   dmx_calls_fetch           copies the records of a sealed set to the host.
 *   dmx_calls_release         frees one set.
 *   dmx_calls_barcode_counts  the counters of the reference's summarize_counted_SNPs (utils.py:163-180): molecules per
 *                             compressed_cb, and calls per compressed_cb of their molecule, int64[n_barcodes] each (integer
 *                             atomics).  DMX_ERR_INVALID: a compressed_cb outside [0, n_barcodes).
 *   dmx_stage_device_containers  dmx_stage_containers with DEVICE pointers (views): no upload, the same field extraction, the
 *                             same check and message; dmx_pack_staged_and_set_problem follows unchanged.  A set may belong to
 *                             another context of the same device (a sealed set's stream has been waited for).  Every pointer must
 *                             be device memory of the context's device and the records must lie inside its allocation
 *                             (hipPointerGetAttributes), else DMX_ERR_INVALID.  The stream is drained before it returns, so the
 *                             owner may release the set afterwards.
 *   dmx_snp_count_device      dmx_snp_count with device views, under the same rules.
 *   dmx_get_calls_transfer_bytes  bytes[2] = cumulative bytes of call records this context copied host to device (dmx_stage_containers,
 *                             dmx_pack_containers_and_set_problem, dmx_snp_count, dmx_calls_upload) and device to host
 *                             (dmx_count_reads_fetch, dmx_calls_fetch).  The resident entry points add nothing.
 * ------------------------------------------------------------------------- */
int dmx_calls_upload(dmx_ctx *ctx, const dmx_call_container *host, int64_t *handle);
int dmx_calls_open(dmx_ctx *ctx, int64_t *handle);
int dmx_calls_append_counted(dmx_ctx *ctx, int64_t handle);
int dmx_calls_seal(dmx_ctx *ctx, int64_t handle);
int dmx_calls_concatenate(dmx_ctx *ctx, const int64_t *handles, int32_t n_handles, int64_t *handle);
int dmx_calls_view(dmx_ctx *ctx, int64_t handle, dmx_call_container *view);
int dmx_calls_info(dmx_ctx *ctx, int64_t handle, int64_t *info);
int dmx_calls_fetch(dmx_ctx *ctx, int64_t handle, void *molecules_out, void *snp_calls_out);
int dmx_calls_release(dmx_ctx *ctx, int64_t handle);
int dmx_calls_barcode_counts(dmx_ctx *ctx, int64_t handle, int64_t n_barcodes, int64_t *calls_per_barcode, int64_t *molecules_per_barcode);
int dmx_stage_device_containers(dmx_ctx *ctx, const dmx_call_container *views, int32_t n_views);
int dmx_snp_count_device(dmx_ctx *ctx, const dmx_call_container *views, int32_t n_views, const int32_t *donor_of_barcode,
                         int64_t n_barcodes, int32_t n_donors, float p_threshold, int32_t cap, int64_t *n_positions);
int dmx_get_calls_transfer_bytes(dmx_ctx *ctx, int64_t *bytes);

/* ------------------------------------------------------------------------- *
 * Donor-level read-outs of the posteriors (product API; declared here because demux_hip.h is kept to 64 entry points).
 * Reductions of the resident float32 posteriors [B, K] of the last dmx_estep / dmx_em, like dmx_get_top_options and
 * dmx_get_option_sums (call order: after dmx_estep / dmx_em; B == 0 returns 0), that fold the pair columns of a doublet run
 * back onto donors (csrc/results.hip).  Columns as everywhere: singlets 0 .. G-1, pair (g1 < g2) at
 * G + g1 (2G - g1 - 1) / 2 + (g2 - g1 - 1); a run without doublets has K == G and no pair columns.
 *   dmx_get_donor_readout  one pass over the matrix; every output is B long but donor_marginals [B, G], and any may be NULL:
 *                          singlet_mass / doublet_mass  float64 sums of the singlet / of the pair columns (0 without pairs), in
 *                              a fixed order: the same bits from run to run, within (K - 1) 2^-53 relative of any other order;
 *                          best_singlet / best_pair     the first maximum over the singlet / the pair columns, as a COLUMN index,
 *                              with its posterior: ties go to the lower column and NaNs never win (the rule of
 *                              dmx_get_top_options); -1 and NaN where there is no such column (best_pair without doublets);
 *                          donor_marginals[b, g]        the posterior mass of every option that contains donor g: the float32
 *                              values widened to float64 and added sequentially in ASCENDING COLUMN ORDER - singlet g, then
 *                              (0, g) .. (g-1, g), then (g, g+1) .. (g, G-1) -, rounded to float32 once: reproducible and
 *                              checkable bit for bit.  NULL: neither computed nor allocated.
 *   dmx_get_allowed_mass   the device half of the reference's utils._compute_qualities (utils.py:265-296).  The options allowed
 *                          for barcode b are allowed_options[allowed_start[b] .. allowed_start[b + 1]) (CSR, B + 1 starts).
 *                          mass[b]: the listed posteriors widened to float64 and added sequentially in list order (an option
 *                          listed twice is added twice, an empty list gives 0); best_is_allowed[b]: 1 when the first maximum of
 *                          the whole row (dmx_get_top_options, k = 1) is in the list.  Either output may be NULL.
 *                          DMX_ERR_INVALID before anything is launched: allowed_start[0] != 0, a decreasing allowed_start, an
 *                          option outside [0, K).
 * ------------------------------------------------------------------------- */
int dmx_get_donor_readout(dmx_ctx *ctx, double *singlet_mass, double *doublet_mass, int32_t *best_singlet, float *best_singlet_prob,
                          int32_t *best_pair, float *best_pair_prob, float *donor_marginals);
int dmx_get_allowed_mass(dmx_ctx *ctx, const int64_t *allowed_start, const int32_t *allowed_options, double *mass,
                         int32_t *best_is_allowed);

/* ------------------------------------------------------------------------- *
 * The pooled E-step (product API; declared here because demux_hip.h is kept to 64 entry points; csrc/estep_pools.hip).
 * Every barcode is scored against the donors of its own POOL only - a lane, hashtag group or sub-experiment that holds a known
 * subset of the donors -, all pools in one pass over the resident call records and the one resident genotype table
 * (call order: a problem and dmx_probs_from_betas / dmx_set_probs; single GPU).
 *   pools       pool p is the strictly ascending list pool_donors[pool_start[p] .. pool_start[p + 1]) of g_p >= 1 table columns.
 *               Its options are the reference's for that genotype list (demux.py:175-191): the g_p singlets in list order, then,
 *               with_doublets, the pairs (i < j), i-major: K_p = g_p or g_p (g_p + 1) / 2 options, at most 1024 (44 donors with
 *               doublets, 1024 without).
 *   logit       logit[b, k] = f32(f64(pen) + sum over the calls of b in their stored order of f64(log_f32(q keep + floor))),
 *               q = prob[v, d] for a singlet and (prob[v, d1] + prob[v, d2]) * 0.5f for a pair, pen = 0 for a singlet and
 *               pair_penalty[p] for a pair: the exact E-step's arithmetic, whatever dmx_set_estep_mode says.  The posterior
 *               row is the float32 softmax of dmx_estep's exact forms.  So the row of a barcode of pool p equals, bit for bit,
 *               what the reference computes for the genotype list of p on the column subset of the same table.
 *   rows        compact: barcode b owns entries row_ptr[b] .. row_ptr[b + 1) of logits_out / probs_out (float32[row_ptr[B]],
 *               nullable), K_p of them, none when pool_of_barcode[b] == -1 (in no pool).
 *   read-outs   per barcode, each nullable: best_option = the first arg-max inside the pool's option list (ties to the lower
 *               index, NaN never wins) with its posterior best_prob; doublet_mass = the pair posteriors widened to float64 and
 *               added sequentially in ascending option order (0 without doublets).  A barcode in no pool gets -1 / NaN / NaN.
 * Checked on the host before anything is launched.  DMX_ERR_INVALID: pool_start[0] != 0 or decreasing, an empty pool, donors not
 * strictly ascending or outside [0, G), a pool id outside [-1, n_pools), a row_ptr other than the pool sizes imply, no problem or
 * no table.  DMX_ERR_UNSUPPORTED: a pool of more than 1024 options, a communicator attached.  The resident results of the last
 * dmx_estep / dmx_em are left as they are; the pass is counted in the DMX_T_ESTEP slot of dmx_get_timings.
 * ------------------------------------------------------------------------- */
int dmx_estep_pools(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                    const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                    const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                    float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                    int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */);

/* ------------------------------------------------------------------------- *
 * Learning within pools (product API).  The reference's EM loop (demux.py:86-118) with its E-step replaced by the
 * pooled one: a donor outside a barcode's pool has posterior 0 for that barcode.
 *   dense       the singlet posteriors of a pooled pass as the M-step reads them: float32[B, G], dense[b, d_p[i]] = row_b[i] for
 *               i < g_p (p the pool of b), every other entry +0 - a barcode in no pool is a row of zeros and contributes nothing,
 *               a donor in no pool keeps an all-zero addition column.
 *   dmx_estep_pools_resident   the arguments, the pass and the results of dmx_estep_pools.  It also leaves `dense` as the context's
 *               resident posteriors with K = G (and their bitmaps and codes), so that dmx_mstep may follow; dmx_get_probs then
 *               returns that [B, G] matrix.  The logits of the pass are the compact ones only: dmx_get_logits is refused.
 *   dmx_em_pools   n_iterations >= 1 of: genotype_prob from betas + addition clipped to [lo, hi] (the addition starts at 0), the
 *               dense pooled E-step, addition = the M-step of `dense` with `power` - the loop of dmx_em, the M-step after the
 *               last E-step left out.  The outputs (each nullable) are the last iteration's compact rows and read-outs, as
 *               dmx_estep_pools defines them, and addition_out float32[V, G], the addition its E-step used.  dmx_get_learnt_betas
 *               and dmx_get_probs work afterwards.  (call order: a problem and dmx_set_betas / dmx_set_prior_betas)
 * Exactness: the pooled E-step has no tolerance arithmetic; with dmx_set_exact_additions(ctx, 1) posteriors, logits, additions and
 * learnt betas are the restated loop's bit for bit; with the default additions the M-step is dmx_mstep's, with its bound.
 * Both validate exactly as dmx_estep_pools does, before anything is uploaded or launched, and return DMX_ERR_UNSUPPORTED with a
 * communicator attached (dmx_comm_init*) or more than one rank; dmx_em_pools returns DMX_ERR_INVALID for n_iterations < 1.
 * ------------------------------------------------------------------------- */
int dmx_estep_pools_resident(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                             const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                             const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                             float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                             int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */);
int dmx_em_pools(dmx_ctx *ctx, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools,
                 const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                 const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */, float power,
                 float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                 int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                 float *addition_out /* nullable, float32[V, G] */);

/* ------------------------------------------------------------------------- *
 * Ambient RNA fractions (product API; declared here because demux_hip.h is kept to 64 entry points; csrc/ambient_profile.hip;
 * DESIGN.md 4.6).  How much of a barcode's signal is NOT from the option it was assigned to: the log-likelihood of its calls on a
 * grid of contamination fractions, in one pass over the resident call records and the resident genotype table (call order: a
 * problem and dmx_probs_from_betas / dmx_set_probs; single GPU).
 *   alphas      float32[n_alphas], 1 <= n_alphas <= 64, every value finite and in [0, 1]; any order, duplicates allowed.
 *   donor1/2    int32[B]: the assigned option of barcode b as table columns.  donor1 == -1: skipped; donor2 == -1: the singlet
 *               donor1; otherwise the pair 0 <= donor1 < donor2 < G.
 *   ambient     float32[V], nullable: the soup's allele profile per table row, every value finite and in [0, 1].  NULL: derived
 *               from the resident calls - with c[v] the barcode-level calls of variant v (padding not counted), the P-step's
 *               own formula (demux.py:267-274) on the one-column table beta[v] = f32(c[v] + 1), clipped to [lo, hi]: a SNP
 *               nobody called comes out uniform.  DMX_ERR_UNSUPPORTED where a variant has 2^24 calls or more.
 *   loglik      for barcode b and grid point j, in float32 without contraction, over the calls of b in stored order:
 *                 q = prob[v, d1]  or  (prob[v, d1] + prob[v, d2]) * 0.5f
 *                 m = q * (1.0f - alphas[j]) + ambient[v] * alphas[j]          two products, one sum, each rounded
 *                 L[b, j] = f32( sum of f64( log_f32(m * keep + floor) ) )     the exact E-step's log, sequential float64 sum
 *               At alphas[j] == 0, m == q: that column of a singlet is the donor's column of the reference's logits, bit for bit.
 *   outputs     each nullable: loglik float32[B, n_alphas]; best int32[B], the first maximum over j (ties to the lower index,
 *               NaN never wins); ll_best, ll_zero float32[B]: L[b, best] and L[b, j0], j0 the first j with alphas[j] == 0 (NaN
 *               where the grid has no 0); ambient_out float32[V]: the profile that was used.  A skipped barcode gets NaN / -1 /
 *               NaN / NaN; a barcode without calls +0.0 in every column and best 0.
 * Checked on the host before anything is uploaded or launched.  DMX_ERR_INVALID: no problem or no table, n_alphas < 1, a grid or
 * ambient value that is not finite or outside [0, 1], donors that break the rules above.  DMX_ERR_UNSUPPORTED: n_alphas > 64, a
 * communicator attached.  The resident results of the last dmx_estep / dmx_em are left as they are; the pass is counted in the
 * DMX_T_ESTEP slot of dmx_get_timings.
 * ------------------------------------------------------------------------- */
int dmx_ambient_profile(dmx_ctx *ctx, float lo, float hi, int32_t n_alphas, const float *alphas /* [n_alphas] */,
                        const int32_t *donor1, const int32_t *donor2 /* [B] */, const float *ambient /* nullable, [V] */,
                        float *loglik /* nullable, [B, n_alphas] */, int32_t *best, float *ll_best, float *ll_zero /* nullable, [B] */,
                        float *ambient_out /* nullable, [V] */);

/* ------------------------------------------------------------------------- *
 * The pooled E-step under per-barcode ambient RNA fractions (product API; csrc/estep_ambient.hip).  dmx_estep_pools
 * with every option scored under the barcode's own contamination fraction: a contaminated singlet - its donor plus a little of
 * everybody - is no longer taken for a doublet.  (call order: a problem and dmx_probs_from_betas / dmx_set_probs; single GPU)
 *   pools, rows, read-outs   the arguments of dmx_estep_pools, with its meaning.
 *   alpha       float32[B]: the fraction of barcode b, finite and in [0, 1]; not looked at for a barcode in no pool.
 *   ambient     float32[V], nullable: the soup's allele profile, as dmx_ambient_profile takes it; NULL: derived exactly as
 *               dmx_ambient_profile derives it, clipped to [lo, hi].  ambient_out (nullable, float32[V]): the profile that was used.
 *   logit       for barcode b of pool p and option k of that pool, in float32 without contraction, over the calls of b in stored order:
 *                 q = prob[v, d]  or  (prob[v, d1] + prob[v, d2]) * 0.5f                  as dmx_estep_pools
 *                 m = q * (1.0f - alpha[b]) + ambient[v] * alpha[b]                       two products, one sum, each rounded
 *                 logit[b, k] = f32( f64(pen) + sum of f64( log_f32(m * keep + floor) ) )  pen = 0 for a singlet, pair_penalty[p] for a pair
 *               The softmax, the compact rows and the read-outs are dmx_estep_pools'.
 * Two identities: with alpha all 0, m == q, and every output equals dmx_estep_pools' on the same arguments bit for bit; with
 * pair_penalty 0, logit[b, k] equals dmx_ambient_profile's L[b, j] for the option's donors and alphas[j] == alpha[b], bit for bit.
 * Checked on the host before anything is uploaded or launched (csrc/ambient_scoring_plan.h).  DMX_ERR_INVALID: everything
 * dmx_estep_pools refuses so, a null alpha with B > 0, an alpha of a pooled barcode or an ambient value that is not finite or outside
 * [0, 1].  DMX_ERR_UNSUPPORTED: a pool of more than 1024 options, a communicator attached, a genotype table in a padded exchange
 * layout.  The resident results of the last dmx_estep / dmx_em are left as they are; the pass is counted in the DMX_T_ESTEP slot.
 * ------------------------------------------------------------------------- */
int dmx_estep_ambient(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                      const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                      const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                      float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                      int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                      float lo, float hi, const float *alpha /* [B] */, const float *ambient /* nullable, [V] */,
                      float *ambient_out /* nullable, [V] */);

/* ------------------------------------------------------------------------- *
 * The pooled E-step with every option scored at its own best ambient fraction (product API; csrc/estep_ambient_grid.hip;
 * DESIGN.md 4.8).  dmx_estep_ambient needs a fraction per barcode, and a fraction estimated under the best singlet absorbs a true
 * doublet's second donor as contamination.  Here every option, singlets and pairs, is scored on a grid of fractions and enters the
 * softmax with its own maximum: the choice between "contaminated singlet" and "doublet" is made inside one softmax, in one pass.
 * (call order: a problem and dmx_probs_from_betas / dmx_set_probs; single GPU)
 *   pools, rows, read-outs   the arguments of dmx_estep_pools, with its meaning.
 *   lo, hi, ambient, ambient_out   as dmx_estep_ambient takes them.
 *   alphas      float32[n_alphas], the grid under dmx_ambient_profile's rules: 1 <= n_alphas <= 64, every value finite and in
 *               [0, 1]; any order, duplicates allowed.
 *   logit       for barcode b of pool p, option k of that pool and grid point j, in float32 without contraction, over the calls of
 *               b in stored order:
 *                 q = prob[v, d]  or  (prob[v, d1] + prob[v, d2]) * 0.5f                     as dmx_estep_pools
 *                 m = q * (1.0f - alphas[j]) + ambient[v] * alphas[j]                        two products, one sum, each rounded
 *                 lambda[b, k, j] = f32( f64(pen) + sum of f64( log_f32(m * keep + floor) ) )   pen as dmx_estep_pools
 *                 j*[b, k] = the first maximum of lambda[b, k, .] in float32 (ties to the lower j, NaN never wins; -1 if all NaN)
 *                 logit[b, k] = lambda[b, k, j*]                                              NaN if j* == -1
 *               The softmax, the compact rows and the read-outs are dmx_estep_pools' on these logits.  A barcode without calls
 *               has lambda = pen for every j, hence j* = 0.
 *   outputs     beside dmx_estep_pools', each nullable: alpha_index int32[row_ptr[B]], j* per option, compact like the logits;
 *               best_alpha_index int32[B], j* of best_option (-1 where best_option is -1 or the barcode is in no pool);
 *               profile_out float32[row_ptr[B] * n_alphas], lambda itself, the grid point minor - n_alphas times the logits'
 *               memory, for small runs and tests.
 * Three identities, bit for bit: with n_alphas == 1 every shared output is dmx_estep_ambient's with alpha[b] = alphas[0] for all b
 * (so alphas = {0} gives dmx_estep_pools); column j of profile_out is dmx_estep_ambient's logits_out with alpha = alphas[j]
 * everywhere; with pair_penalty 0, lambda[b, k, .] is dmx_ambient_profile's L[b, .] for that option's donors and j*[b, k] its best.
 * Checked on the host before anything is uploaded or launched (csrc/ambient_grid_plan.h).  DMX_ERR_INVALID: everything
 * dmx_estep_pools refuses so, n_alphas < 1, null alphas, a grid or ambient value that is not finite or outside [0, 1].
 * DMX_ERR_UNSUPPORTED: n_alphas > 64, a pool of more than 1024 options, a communicator attached, a genotype table in a padded
 * exchange layout.  The resident results of the last dmx_estep / dmx_em are left as they are; the pass is counted in the
 * DMX_T_ESTEP slot.
 * ------------------------------------------------------------------------- */
int dmx_estep_ambient_grid(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                           const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                           const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                           float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                           int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                           float lo, float hi, int32_t n_alphas, const float *alphas /* [n_alphas] */,
                           const float *ambient /* nullable, [V] */, float *ambient_out /* nullable, [V] */,
                           int32_t *alpha_index /* nullable, int32[row_ptr[B]] */, int32_t *best_alpha_index /* nullable, [B] */,
                           float *profile_out /* nullable, float32[row_ptr[B] * n_alphas] */);

/* ------------------------------------------------------------------------- *
 * The same pass with the grid summed instead of searched (product API; csrc/estep_ambient_grid.hip: the MARGINAL forms;
 * DESIGN.md 4.10).  The maximum gives an option no credit for fitting over a wide range of fractions; here an option's logit is the
 * log of the sum over the grid of exp(lambda + log_weights), in a defined order.  The arguments are dmx_estep_ambient_grid's without
 * profile_out, and:
 *   log_weights      float32[n_alphas], nullable (NULL: all 0): the log of a prior over the grid; every value finite.
 *   alpha_mean       float32[row_ptr[B]], nullable, compact like the logits; best_alpha_mean float32[B], nullable.
 * lambda[b, k, j], pen and the float64 sum S[b, k, j] of the log terms are dmx_estep_ambient_grid's: lambda = f32(f64(pen) + S).  Per
 * option, j ascending, in float32, every operation rounded, no contraction (exp and log are the E-step's own float32 kernels):
 *     t = lambda[j] + log_weights[j]                                  a NaN is skipped
 *     first t:    jm = j; m = t; s = 1; u = alphas[j]
 *     t >  m:     r = exp(m - t); s = s * r + 1; u = u * r + alphas[j]; m = t; jm = j
 *     t == m:     s = s + 1; u = u + alphas[j]                        (-inf == -inf among them)
 *     t <  m:     x = exp(t - m); s = s + x; u = u + alphas[j] * x
 *   after the grid:
 *     logit[b, k]      = f32( f64(pen) + ( S[b, k, jm] + f64( f32(log_weights[jm] + log(s)) ) ) )     NaN if no t was a number
 *     alpha_index      = jm (-1 if none): the first maximum of lambda + log_weights
 *     alpha_mean[b, k] = u / s                                        IEEE float32 division; NaN if none
 * The softmax, the compact rows and the read-outs are dmx_estep_pools' on these logits; best_alpha_index[b] and best_alpha_mean[b]
 * are best_option's entries (-1 / NaN where there is none).
 * Identities, bit for bit: with n_alphas == 1 and log_weights NULL or {0} every shared output is dmx_estep_ambient_grid's (and so
 * dmx_estep_ambient's; with alphas = {0} dmx_estep_pools'), and alpha_mean is alphas[0] wherever the logit is no NaN; with
 * log_weights NULL alpha_index and best_alpha_index are dmx_estep_ambient_grid's and every logit is >= its logit; with the grid
 * {a, a} the logit is f32(f64(pen) + (S + f64(log(2.0f)))); log_weights of all zeros is log_weights NULL.
 * Checked on the host before anything is uploaded or launched (csrc/ambient_grid_plan.h: check_marginal): everything
 * dmx_estep_ambient_grid refuses, with its codes, and DMX_ERR_INVALID for a log weight that is not finite.  The resident results of
 * the last dmx_estep / dmx_em are left as they are; the pass is counted in the DMX_T_ESTEP slot.
 * ------------------------------------------------------------------------- */
int dmx_estep_ambient_grid_marginal(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                                    const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                                    const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                                    float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                                    int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                                    float lo, float hi, int32_t n_alphas, const float *alphas /* [n_alphas] */,
                                    const float *ambient /* nullable, [V] */, float *ambient_out /* nullable, [V] */,
                                    int32_t *alpha_index /* nullable, int32[row_ptr[B]] */, int32_t *best_alpha_index /* nullable, [B] */,
                                    const float *log_weights /* nullable, [n_alphas] */,
                                    float *alpha_mean /* nullable, float32[row_ptr[B]] */, float *best_alpha_mean /* nullable, [B] */);

/* ------------------------------------------------------------------------- *
 * The pooled E-step with every pair option summed over a grid of mixing shares (product API; csrc/estep_pair_shares.hip;
 * DESIGN.md 4.12).  dmx_estep_pools scores a pair as the even mixture (p1 + p2) * 0.5; two cells of different RNA content share a
 * droplet unevenly, and an uneven doublet scored at 0.5 looks like its major donor.  Here a pair's logit is the log of the weighted sum
 * over a grid of shares of its first donor.  Pools, rows, read-outs, the no-pool and no-call conventions and the option order are
 * dmx_estep_pools'; singlet options are untouched.  Beyond its arguments:
 *   shares           float32[n_shares], 1 .. 64 values in [0, 1], any order, duplicates allowed: the share of d1 in a pair (d1, d2),
 *                    d1 ahead of d2 in the pool's option order.
 *   log_weights      float32[n_shares], nullable (NULL: all 0): the log of a prior over the grid; every value finite.
 *   share_index, share_mean            int32 / float32[row_ptr[B]], nullable, compact like the logits
 *   best_share_index, best_share_mean  int32 / float32[B], nullable
 * Pair option k = (d1, d2) of barcode b in pool p, grid point j; float32, every operation rounded, no contraction, over the calls of b
 * in stored order:
 *     w1 = shares[j];  w2 = 1.0f - shares[j]
 *     q  = prob[v, d1] * w1 + prob[v, d2] * w2                         two products, one sum
 *     S[b, k, j] = sum of f64( log_f32(q * keep + floor) )             the exact E-step's log, sequential float64 sum
 *     lambda[b, k, j] = f32( f64(pen) + S[b, k, j] )                   pen = pair_penalty[p]
 * Across the grid, j ascending: dmx_estep_ambient_grid_marginal's recurrence above with shares[j] for alphas[j] - its t, m, s, u, jm,
 * its exp and log, its treatment of equal t, -inf and NaN:
 *     logit[b, k]       = f32( f64(pen) + ( S[b, k, jm] + f64( f32(log_weights[jm] + log(s)) ) ) )    NaN if no t was a number
 *     share_index[b, k] = jm (-1 if none);   share_mean[b, k] = u / s  IEEE float32 division; NaN if none
 * A singlet option's logit is dmx_estep_pools' own, f32(f64(0) + S) with q = prob[v, d]; the grid and the weights do not enter it,
 * its share_index is -1 and its share_mean NaN.  best_share_index[b] and best_share_mean[b] are best_option's entries: -1 / NaN
 * where best_option is a singlet, where it is -1, or where the barcode is in no pool.
 * The normalisation of the weights matters here, unlike in dmx_estep_ambient_grid_marginal: singlets do not go through the grid, so a
 * constant added to every log weight moves every pair against every singlet.  With log_weights NULL a pair's logit is the log of a
 * SUM over the grid, not of a mean; the uniform prior is log_weights[j] = -log(n_shares).
 * Identities, bit for bit: (S1) shares = {0.5}, log_weights NULL or {0}: every shared output is dmx_estep_pools' - halving is exact,
 * fl(p1 / 2 + p2 / 2) = fl(p1 + p2) / 2, on a table whose non-zero entries are at least 2^-125 (no halved entry is subnormal) - and
 * share_mean is 0.5 on every pair option; (S2) with_doublets == 0 is dmx_estep_pools, the share outputs are -1 / NaN and no grid
 * kernel is launched; (S3) shares = {1}, log_weights NULL: a pair's logit is f32(f64(pen) + S) with S the float64 sum of its first
 * donor's singlet option in the same row (shares = {0}: the second donor's); (S4) the grid {a, a}, log_weights NULL:
 * logit = f32(f64(pen) + (S + f64(log_f32(2.0f)))); (S5) log_weights of all zeros is log_weights NULL.
 * Checked on the host before anything is uploaded or launched (csrc/pair_shares_plan.h), in this order: everything dmx_estep_pools
 * and the pooled entries under ambient fractions refuse of the context and the pools, with their codes and words (a communicator, a
 * padded table layout, more than 1024 options in a pool among them); DMX_ERR_INVALID for n_shares < 1, null shares, a share that is
 * not finite or outside [0, 1], a log weight that is not finite; DMX_ERR_UNSUPPORTED for n_shares > 64.  The resident results of the
 * last dmx_estep / dmx_em and the pooled slot (dmx_set_keep_pooled) are left as they are; the pass is counted in the DMX_T_ESTEP slot.
 * ------------------------------------------------------------------------- */
int dmx_estep_pair_shares(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                          const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                          const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                          float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                          int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                          int32_t n_shares, const float *shares /* [n_shares] */, const float *log_weights /* nullable, [n_shares] */,
                          int32_t *share_index /* nullable, int32[row_ptr[B]] */, float *share_mean /* nullable, float32[row_ptr[B]] */,
                          int32_t *best_share_index /* nullable, [B] */, float *best_share_mean /* nullable, [B] */);

/* ------------------------------------------------------------------------- *
 * Pooled results kept resident (product API; declared here because demux_hip.h is kept to 64 entry points;
 * csrc/pooled_readout.hip).  The context owns one "pooled slot": the compact result of a pooled pass - the pool
 * layout, pool_of_barcode, row_ptr, the compact posteriors, the compact logits (may be absent), from the grid passes the compact
 * alpha_index and from the marginal pass also alpha_mean, and every pool's barcodes in ascending order - on the device.  The slot is
 * independent of the resident results of dmx_estep / dmx_em: neither touches the other, and the dense read-outs do not see it.
 * dmx_destroy and dmx_release_problem drop it.
 *   dmx_set_keep_pooled   keep = 1: dmx_estep_pools, dmx_estep_ambient, dmx_estep_ambient_grid and dmx_estep_ambient_grid_marginal
 *                         leave their compact result in the slot on a successful return (default 0: nothing is kept, nothing
 *                         changes).  The buffers are handed over from the pass's temporaries, not copied.  Every output pointer of
 *                         those entries keeps its meaning; with NULL for logits_out / probs_out nothing of size row_ptr[B] is
 *                         downloaded.  A kept result replaces the previous one; a failed call leaves the previous one in place.
 *                         dmx_estep_pools_resident, dmx_estep_ambient_resident, dmx_em_pools and dmx_em_ambient never touch the slot.
 *   dmx_pooled_upload     fills the slot from host arrays (a result saved earlier; tests).  Needs no problem on the context.  The
 *                         pool arguments are dmx_estep_pools' (without penalties) and are refused as it refuses them, G being
 *                         the number of table columns the donors index; probs must not be NULL when row_ptr[B] > 0.
 *   dmx_pooled_info       info[8] = present, B, n_pools, n_values (= row_ptr[B]), with_doublets, has_logits, has_alpha_index,
 *                         has_alpha_mean.
 *   dmx_pooled_release    drops the slot (nothing to drop: no error).
 *   dmx_pooled_get        entries row_ptr[b0] .. row_ptr[b1] of matrix `what` (0 logits, 1 probs: float32; 2 alpha_index: int32;
 *                         3 alpha_mean: float32) - the rows of barcodes b0 <= b < b1, contiguous.
 *   dmx_pooled_get_pool   the rows of one pool's barcodes, in ascending barcode order, as a dense [n_p, K_p] block of `what`
 *                         (gathered on the device, one download).
 * Read-outs of the slot's posteriors.  Option indices are POOL-LOCAL: for a pool of g donors option i < g is singlet i, pair
 * (i < j) is at g + i (2g - i - 1) / 2 + (j - i - 1); K_p = g or g (g + 1) / 2 <= 1024.  The order of additions is the contract.
 *   dmx_pooled_readout    one pass; every output nullable and B long but donor_marginals:
 *                         singlet_mass / doublet_mass   float64: the row's singlet / pair entries widened and added sequentially
 *                             in ascending option order - dmx_estep_pools' own doublet_mass, bit for bit (0 without doublets);
 *                         best_option / best_singlet / best_pair with their posteriors: the first maximum over the whole row /
 *                             its singlets / its pairs (ties to the lower index, NaN never wins); -1 and NaN where there is none;
 *                         donor_marginals   compact float32: barcode b owns entries marg_ptr[b] .. marg_ptr[b + 1), g_p of them
 *                             (marg_ptr_out int64[B + 1], nullable); entry i is singlet i, then pairs (0, i) .. (i-1, i), then
 *                             (i, i+1) .. (i, g-1), widened to float64, added in that order and rounded once.  NULL: neither
 *                             computed nor allocated.
 *                         A barcode in no pool gets -1 / NaN everywhere (masses included) and no marginal entries.
 *   dmx_pooled_top_options  the k (1..4) best options per barcode, best first, as dmx_get_top_options: int32 / float32 [B, k],
 *                         -1 / NaN where the row is shorter than k or the barcode is in no pool.
 *   dmx_pooled_option_sums  sums float64[opt_ptr[P]] (pool after pool, K_p entries each), n_barcodes int64[P]; either nullable.
 *                         Per pool and option the float64 sum over the pool's n_p barcodes in ascending order, in a fixed order:
 *                         per = ceil(n_p / 512); slab j = list positions [j per, min((j + 1) per, n_p)) added sequentially; then
 *                         the 512 slab sums in slab order (dmx_get_option_sums' rule).  An empty pool gives zeros.
 *   dmx_pooled_allowed_mass  dmx_get_allowed_mass with pool-local options.  DMX_ERR_INVALID before anything is launched:
 *                         allowed_start[0] != 0, a decreasing start, an option outside [0, K_p(b)), a non-empty list for a barcode
 *                         in no pool - which gets mass NaN and best_is_allowed 0.
 * Every entry but dmx_set_keep_pooled, dmx_pooled_upload, dmx_pooled_info and dmx_pooled_release returns DMX_ERR_INVALID with a
 * call-order message while the slot is empty.
 * ------------------------------------------------------------------------- */
int dmx_set_keep_pooled(dmx_ctx *ctx, int keep);
int dmx_pooled_upload(dmx_ctx *ctx, int64_t B, int32_t G, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                      const int32_t *pool_donors, const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                      const float *logits /* nullable */, const float *probs /* float32[row_ptr[B]] */);
int dmx_pooled_info(dmx_ctx *ctx, int64_t info[8]);
int dmx_pooled_release(dmx_ctx *ctx);
int dmx_pooled_get(dmx_ctx *ctx, int what, int64_t b0, int64_t b1, void *out);
int dmx_pooled_get_pool(dmx_ctx *ctx, int what, int32_t pool, void *out /* [n_p, K_p] */);
int dmx_pooled_readout(dmx_ctx *ctx, double *singlet_mass, double *doublet_mass, int32_t *best_option, float *best_prob,
                       int32_t *best_singlet, float *best_singlet_prob, int32_t *best_pair, float *best_pair_prob,
                       int64_t *marg_ptr_out /* [B+1] */, float *donor_marginals /* float32[marg_ptr[B]] */);
int dmx_pooled_top_options(dmx_ctx *ctx, int32_t k, int32_t *options, float *probs);
int dmx_pooled_option_sums(dmx_ctx *ctx, double *sums /* [opt_ptr[P]] */, int64_t *n_barcodes /* [P] */);
int dmx_pooled_allowed_mass(dmx_ctx *ctx, const int64_t *allowed_start, const int32_t *allowed_options, double *mass,
                            int32_t *best_is_allowed);

/* ------------------------------------------------------------------------- *
 * Learning under per-barcode ambient RNA fractions (product API; csrc/mstep_ambient.hip, csrc/estep_ambient.hip).
 * dmx_em_pools' loop with two changes per iteration: the pooled row is dmx_estep_ambient's, and every call's contribution to the
 * M-step is weighted by the probability that the call came from the donor and not from the soup.  For variant v, donor column g and
 * the calls c of v in stored variant-major order, b = cb_c, in float32 without contraction:
 *     own = prob[v, g] * (1.0f - alpha[b])
 *     mix = own + ambient[v] * alpha[b]
 *     r   = own == 0 ? 0.0f : own / mix                          IEEE float32 division, correctly rounded
 *     w   = ((dense[b, g] * keep_c) * r) ^ power                 power 2: one float32 product w * w; another power:
 *                                                                f32(pow(f64(base), f64(power))), where dmx_mstep has powf
 *     addition[v, g] = f32( sum over c of f64(w) )               one float64 accumulator, in call order
 * prob is the table the E-step of `dense` read; `dense` as "Learning within pools" defines it.  With alpha[b] == 0, r == 1 for every
 * table entry other than 0, and w is dmx_mstep's: with every fraction 0 the loop is dmx_em_pools with exact additions, bit for bit (on a
 * table without zeros: lo > 0; with another power than 2: to float32 accuracy).  alpha[b] == 1 gives r == 0: a droplet that is all
 * soup teaches nothing.
 * There is ONE arithmetic: the sums are float64 in the reference's order whatever dmx_set_estep_mode / dmx_set_exact_additions say;
 * the fixed-point, tile-major and incremental M-step forms do not apply (the weights change with the table).  Only the singlet
 * columns are learnt from, with_doublets or not.  The soup's profile is fixed for the call: supplied, or derived once from the calls
 * as dmx_ambient_profile derives it; it does not depend on the betas.
 *   dmx_estep_ambient_resident   the arguments, the pass and the results of dmx_estep_ambient.  It also leaves `dense` as the
 *               context's resident posteriors with K = G (and their bitmaps and codes), as dmx_estep_pools_resident does:
 *               dmx_get_probs, dmx_mstep, dmx_mstep_ambient and dmx_get_learnt_betas work after it.
 *   dmx_mstep_ambient   stateless: the M-step above of the context's resident posteriors (singlet columns) and the table of the
 *               last P-step (dmx_probs_from_betas / dmx_set_probs), with alpha float32[B] (EVERY barcode's is read), ambient
 *               float32[V] or NULL (derived, clipped to [lo, hi]).  The addition becomes the context's (dmx_get_learnt_betas, the
 *               next P-step) and is copied to addition_out (nullable, float32[V, G]).  DMX_ERR_INVALID without a problem, a
 *               table or posteriors.
 *   dmx_em_ambient   n_iterations >= 1 of: genotype_prob from betas + addition clipped to [lo, hi] (the addition starts at 0), the
 *               dense E-step under the fractions, the M-step above - all on the device, the M-step after the last E-step left out;
 *               the pools' round trip, the uploads, the profile and the soup's terms are paid once.  Outputs (each nullable): what
 *               dmx_em_pools returns, and ambient_out float32[V], the profile that was used.  (call order: a problem and
 *               dmx_set_betas / dmx_set_prior_betas)
 * Checked on the host before anything is uploaded or launched (csrc/ambient_learning_plan.h).  DMX_ERR_INVALID: n_iterations < 1, a
 * power that is not finite or not above 0, everything dmx_estep_ambient refuses so.  DMX_ERR_UNSUPPORTED: a communicator attached or
 * more than one rank, a pool of more than 1024 options, a genotype table in a padded exchange layout.  The E-steps are counted in
 * the DMX_T_ESTEP slot, the walk of the M-step in DMX_T_MSTEP, its combining pass and the redo in DMX_T_MCOMBINE; dmx_get_redo_count
 * returns the sums the last M-step redid in call order.
 * ------------------------------------------------------------------------- */
int dmx_estep_ambient_resident(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                               const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                               const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                               float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                               int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                               float lo, float hi, const float *alpha /* [B] */, const float *ambient /* nullable, [V] */,
                               float *ambient_out /* nullable, [V] */);
int dmx_mstep_ambient(dmx_ctx *ctx, float power, const float *alpha /* [B] */, const float *ambient /* nullable, [V] */, float lo, float hi,
                      float *addition_out /* nullable, float32[V, G] */);
int dmx_em_ambient(dmx_ctx *ctx, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools,
                   const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                   const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */, float power,
                   const float *alpha /* [B] */, const float *ambient /* nullable, [V] */,
                   float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                   int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                   float *addition_out /* nullable, float32[V, G] */, float *ambient_out /* nullable, [V] */);

/* ------------------------------------------------------------------------- *
 * Learning the soup's allele profile (product API; csrc/mstep_soup.hip): the third M-step of the ambient model.  The
 * complement of the weight above, s = 1 - r in exact arithmetic, is the probability that a call came from the soup; summed per
 * variant it gives the soup's expected allele counts.  For variant v, donor column g and the calls c of v in stored variant-major
 * order, b = cb_c, in float32 without contraction:
 *     amb = ambient[v] * alpha[b]
 *     own = prob[v, g] * (1.0f - alpha[b])
 *     mix = own + amb
 *     s   = amb == 0 ? 0.0f : amb / mix                          IEEE float32 division, correctly rounded
 *     t   = (dense[b, g] * keep_c) * s                           power 1: expected counts
 *     count[v, g] = f32( sum over c of f64(t) )                  one float64 accumulator, in call order, over dense[b, g] != 0
 *     total[v]    = f32( sum over g of f64(count[v, g]) )        one float64 accumulator, g ascending
 *     beta[v]     = total[v] + pseudo_count
 *     ambient'[v] = the P-step's formula on the one column beta, clipped to [lo, hi]   (as dmx_ambient_profile derives a profile)
 * prob and ambient are the table and the profile the E-step of `dense` read.  alpha[b] == 0 gives s == 0 exactly: with every
 * fraction 0 every count is +0 and ambient' is the pseudo-counts' uniform share within each SNP.  alpha[b] == 1 with
 * ambient[v] != 0 gives s == 1 exactly.  Only the singlet columns are counted, with_doublets or not; a posterior is live when it is
 * not 0.  One arithmetic, whatever dmx_set_estep_mode / dmx_set_exact_additions say.
 *   dmx_mstep_soup   stateless: the step above on the context's resident posteriors and the table of the last P-step, with alpha
 *               float32[B] (EVERY barcode's is read) and ambient float32[V] or NULL (derived, clipped to [lo, hi]).  ambient_out
 *               (nullable, float32[V]) receives ambient', counts_out (nullable, float32[V]) total.  The counts live in scratch:
 *               the context's addition, posteriors, table and dmx_get_learnt_betas are bit for bit what they were before the
 *               call (the codes of the posteriors are rebuilt at floor 0 when they were written above it: additions that follow
 *               keep their bits).  dmx_get_redo_count returns the sums this step redid in call order.
 *   dmx_em_ambient_soup   dmx_em_ambient with the profile learnt.  Per iteration: the P-step; the dense E-step under the fractions
 *               with the current profile (the soup's terms are rebuilt whenever the profile has changed); except after the last
 *               E-step the step above and dmx_mstep_ambient's, both with the profile that E-step read.  The new profile takes
 *               effect in the next iteration.  Outputs (each nullable): what dmx_em_ambient returns - ambient_out the profile of
 *               the LAST E-step - and counts_out float32[V], the totals that profile was formed from (+0 with one iteration: no
 *               step ran).  With the profile unchanged the genotype additions are dmx_em_ambient's bit for bit.
 * Checked on the host before anything is uploaded or launched (csrc/soup_learning_plan.h).  DMX_ERR_INVALID: a pseudo_count that is
 * not finite or not above 0, and everything dmx_mstep_ambient / dmx_em_ambient refuse, with their codes.  The walk is counted in
 * DMX_T_MSTEP, the combining pass and the redo in DMX_T_MCOMBINE, the totals and the profile in DMX_T_PSTEP.
 * ------------------------------------------------------------------------- */
int dmx_mstep_soup(dmx_ctx *ctx, const float *alpha /* [B] */, const float *ambient /* nullable, [V] */, float pseudo_count, float lo, float hi,
                   float *ambient_out /* nullable, [V] */, float *counts_out /* nullable, [V] */);
int dmx_em_ambient_soup(dmx_ctx *ctx, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools,
                        const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                        const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */, float power,
                        const float *alpha /* [B] */, const float *ambient /* nullable, [V] */, float pseudo_count,
                        float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                        int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                        float *addition_out /* nullable, float32[V, G] */, float *ambient_out /* nullable, [V] */,
                        float *counts_out /* nullable, [V] */);

/* ------------------------------------------------------------------------- *
 * Learning from doublet posteriors (product API; csrc/mstep_doublets.hip).  dmx_em_pools' loop with one change per
 * iteration: the M-step credits each donor of a pair option of the barcode's row with its share of every call.  The E-step is
 * dmx_em_pools' dense pooled pass; it leaves the compact rows post[row_ptr[b] ...] in pool-local option order (singlets, then the
 * pairs i < j, i-major) and the dense singlets dense[B, G].  For variant v, donor column g and the calls c of v in stored
 * variant-major order, b = cb_c, in float32 without contraction:
 *     credit = dense[b, g] when it is live (above 2^-80 at power 2, not 0 at another power), else +0
 *     for every pair option k of b's row with post[k] >= min_pair_posterior that contains g, in the row's option order, h its other donor:
 *         own = prob[v, g];  other = prob[v, h]
 *         r   = own == 0 ? 0.0f : own / (own + other)             IEEE float32 division, correctly rounded
 *         credit = credit + post[k] * r
 *     w   = (credit * keep_c) ^ power                             power 2: one float32 product w * w; another power:
 *                                                                f32(pow(f64(base), f64(power)))
 *     addition[v, g] = f32( sum over c of f64(w) )               one float64 accumulator, in call order
 * prob is the table the E-step read; r is the donor's responsibility for the call in the even mixture (p_g + p_h) / 2 the pair was
 * scored with.  A pair below min_pair_posterior is not credited: that is part of the contract.  min_pair_posterior is finite and
 * above 0; above 1 it credits no pair, and then, as with with_doublets == 0, the loop is dmx_em_pools with exact additions bit for
 * bit (another power than 2: to float32 accuracy).  A barcode in no pool contributes nothing.
 * There is ONE arithmetic: the sums are float64 in the reference's order whatever dmx_set_estep_mode / dmx_set_exact_additions say;
 * the fixed-point, tile-major and incremental M-step forms do not apply (the weights change with the table).
 *   dmx_em_doublets   n_iterations >= 1 of: genotype_prob from betas + addition clipped to [lo, hi] (the addition starts at 0), the
 *               dense pooled E-step, the list of the live pairs, the M-step above - all on the device, the M-step after the last
 *               E-step left out; the pools' round trip is paid once.  Outputs (each nullable): what dmx_em_pools returns.  (call
 *               order: a problem and dmx_set_betas / dmx_set_prior_betas)
 *   dmx_mstep_doublets   stateless: the M-step above of the context's resident dense posteriors (dmx_estep_pools_resident), the table
 *               of the last P-step and the compact rows post_rows float32[n_rows] that E-step returned, with the pools it was called
 *               with (n_rows == row_ptr[B]).  The addition becomes the context's and is copied to addition_out (nullable,
 *               float32[V, G]).  DMX_ERR_INVALID without a problem, a table or posteriors.
 * Checked on the host before anything is uploaded or launched (csrc/doublet_learning_plan.h).  DMX_ERR_INVALID: n_iterations < 1, a
 * power or a threshold that is not finite or not above 0, rows of another length than row_ptr[B], a row value that is not finite or
 * outside [0, 1], everything dmx_estep_pools refuses so.  DMX_ERR_UNSUPPORTED: a communicator attached or more than one rank, a pool
 * of more than 1024 options, a genotype table in a padded exchange layout.  The E-steps and the list's build are counted in the
 * DMX_T_ESTEP slot (a span each), the walk of the M-step in DMX_T_MSTEP, its combining pass and the redo in DMX_T_MCOMBINE;
 * dmx_get_redo_count returns the sums the last M-step redid in call order.
 * ------------------------------------------------------------------------- */
int dmx_em_doublets(dmx_ctx *ctx, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools,
                    const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                    const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */, float power,
                    float min_pair_posterior,
                    float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                    int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                    float *addition_out /* nullable, float32[V, G] */);
int dmx_mstep_doublets(dmx_ctx *ctx, float power, float min_pair_posterior, int with_doublets, int32_t n_pools,
                       const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                       const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                       const float *post_rows /* [n_rows] */, int64_t n_rows, float *addition_out /* nullable, float32[V, G] */);

/* ------------------------------------------------------------------------- *
 * Learning from doublets of unequal shares (product API; csrc/mstep_doublet_shares.hip, csrc/estep_pair_shares.hip: the DENSE form;
 * DESIGN.md 4.17).  "Learning from doublet posteriors" above with two changes per iteration: the E-step is dmx_estep_pair_shares'
 * pass - its contract of logits, posteriors, share_index and share_mean, word for word - which also leaves dense[B, G], and the
 * M-step credits a live pair's donors at the pair's posterior mean share.  Let k = (d1, d2) be a pair option of b's row with
 * post[k] >= min_pair_posterior, d1 ahead of d2 in the pool's option order, and w = share_mean[b, k]; float32, every operation rounded:
 *     w_own = w for g == d1;  w_own = 1.0f - w for g == d2 (rounded once);  w_other = the other of the two
 *     a = prob[v, g] * w_own;  o = prob[v, h] * w_other
 *     r = a == 0 ? 0.0f : a / (a + o)                               IEEE float32 division, correctly rounded
 *     credit = credit + post[k] * r
 * Everything else - the live dense credit, the threshold, the row's option order, w = (credit * keep_c) ^ power, the one float64
 * accumulator per (v, g) in call order, ONE arithmetic whatever dmx_set_estep_mode says - is dmx_mstep_doublets'.  A live pair's
 * share_mean lies in [0, 1] (u is a monotone float32 sum of terms fl(e_j share_j) <= e_j, so u <= s); nothing is clamped.
 * Identities, bit for bit: (D1) shares = {0.5}, log_weights NULL or {0}: every output and every iteration's addition is
 * dmx_em_doublets' - share_mean is exactly 0.5, halving is exact on a clipped table and (own / 2) / fl(own / 2 + other / 2) =
 * own / fl(own + other); (D2) the same grid with a threshold above 1, or any grid with with_doublets == 0, is dmx_em_pools with exact additions (without doublets no
 * grid kernel is launched); (D3) shares = {1}: a live pair credits its first donor post[k] where prob[v, d1] > 0 and its second
 * donor nothing; shares = {0} is the mirror image.
 *   dmx_em_doublet_shares   dmx_em_doublets' arguments, loop and outputs with the grid (n_shares, shares, log_weights: as
 *               dmx_estep_pair_shares takes them) and, each nullable, share_index / share_mean / best_share_index / best_share_mean
 *               of the last E-step.  Everything stays on the device between the steps; one read-back.
 *   dmx_estep_pair_shares_resident   the arguments, the pass and the results of dmx_estep_pair_shares.  It also leaves `dense` as the
 *               context's resident posteriors with K = G (and their bitmaps and codes), as dmx_estep_pools_resident does.
 *   dmx_mstep_doublet_shares   stateless: dmx_mstep_doublets with share_rows float32[n_rows] beside post_rows, the compact share_mean
 *               that E-step returned.  Only the entries of pair options are read.
 * Checked on the host before anything is uploaded or launched (csrc/doublet_shares_learning_plan.h): what dmx_estep_pair_shares
 * refuses, then what dmx_em_doublets / dmx_mstep_doublets refuse, with their codes and words; dmx_mstep_doublet_shares also gives
 * DMX_ERR_INVALID for null share_rows (whatever n_rows) and for a pair entry of share_rows that is not finite or outside [0, 1], with its
 * index.  The timer slots are dmx_em_doublets'.  The pooled slot (dmx_set_keep_pooled) is left as it is.
 * ------------------------------------------------------------------------- */
int dmx_em_doublet_shares(dmx_ctx *ctx, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools,
                          const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                          const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */, float power,
                          float min_pair_posterior, int32_t n_shares, const float *shares /* [n_shares] */,
                          const float *log_weights /* nullable, [n_shares] */,
                          float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                          int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                          float *addition_out /* nullable, float32[V, G] */,
                          int32_t *share_index /* nullable, int32[row_ptr[B]] */, float *share_mean /* nullable, float32[row_ptr[B]] */,
                          int32_t *best_share_index /* nullable, [B] */, float *best_share_mean /* nullable, [B] */);
int dmx_estep_pair_shares_resident(dmx_ctx *ctx, int with_doublets, int32_t n_pools, const int64_t *pool_start /* [n_pools+1] */,
                                   const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                                   const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                                   float *logits_out, float *probs_out,          /* nullable, float32[row_ptr[B]] */
                                   int32_t *best_option, float *best_prob, double *doublet_mass /* nullable, [B] */,
                                   int32_t n_shares, const float *shares /* [n_shares] */, const float *log_weights /* nullable, [n_shares] */,
                                   int32_t *share_index /* nullable, int32[row_ptr[B]] */, float *share_mean /* nullable, float32[row_ptr[B]] */,
                                   int32_t *best_share_index /* nullable, [B] */, float *best_share_mean /* nullable, [B] */);
int dmx_mstep_doublet_shares(dmx_ctx *ctx, float power, float min_pair_posterior, int with_doublets, int32_t n_pools,
                             const int64_t *pool_start /* [n_pools+1] */, const int32_t *pool_donors, const float *pair_penalty /* [n_pools] */,
                             const int32_t *pool_of_barcode /* [B], -1: none */, const int64_t *row_ptr /* [B+1] */,
                             const float *post_rows /* [n_rows] */, const float *share_rows /* [n_rows] */, int64_t n_rows,
                             float *addition_out /* nullable, float32[V, G] */);

#ifdef __cplusplus
}
#endif
#endif /* DEMUX_HIP_DEBUG_H */
