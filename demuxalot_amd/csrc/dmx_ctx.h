// dmx_ctx.h -- the context object behind the opaque dmx_ctx of the C ABI, shared by the
// translation units of libdemux_hip.so (dmx_api.cpp, repack_device.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "ctx_state.h"
#include "dmx_internal.h"
#include "kernels.h"

using dmx::fail;

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return fail(DMX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

#define DMX_TRY(expr)         \
    do {                      \
        int _s = (expr);      \
        if (_s != 0) return _s; \
    } while (0)

// ------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------
// Phase timers (dmx_get_timings).  A stamp is one recorded event; a span is two of them.  Two phases that follow each other
// inside one API call share the stamp between them: an event record is a barrier packet of its own on the queue, and two of them
// back to back at each of an EM iteration's four phase boundaries were 10 us each - 40 us of a 1.14 ms iteration (round 5,
// scripts/iteration_timeline.sh).  Events release to the device only (hipEventReleaseToDevice): nothing on the host reads what the
// kernels wrote at a phase boundary.
struct TimerStamp {
    hipEvent_t ev = nullptr;
    int refs = 0;
};
typedef std::pair<TimerStamp *, TimerStamp *> TimerSpan;

struct TimerSlot {
    std::vector<TimerSpan> pending;
    double ms = 0.0;
    int64_t launches = 0;
    int64_t timed = 0;  // launches that were bracketed by events (phase timers on)
};

// A device buffer of the context and the number of elements it was allocated for (dev_alloc / raw_alloc below).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
};

// The twelve arrays of a dmx_decoded_reads (include/demux_hip.h) on the device.  Every struct that holds them names them alike
// (ReadColumns here; the pointer structs of read_columns.h), and each_read_column below is the one place that lists them.
enum ReadExtent { PER_READ, PER_OP, PER_BASE };

struct ReadCounts {
    long long n = 0, n_ops = 0, n_bases = 0;
    size_t of(ReadExtent e) const { return (size_t)(e == PER_READ ? n : e == PER_OP ? n_ops : n_bases); }
};

// f(extent, counting_only, column ...) for every column, with that column of every struct given; the first status that is
// not 0 ends the round and is returned.  counting_only: read by the counting passes alone (a coverage pass leaves them null).
template <typename F, typename... Structs>
int each_read_column(F &&f, Structs &...s)
{
    DMX_TRY(f(PER_READ, false, s.start...));
    DMX_TRY(f(PER_READ, true, s.cb...));
    DMX_TRY(f(PER_READ, true, s.ub...));
    DMX_TRY(f(PER_READ, true, s.p_misaligned...));
    DMX_TRY(f(PER_READ, true, s.score...));
    DMX_TRY(f(PER_READ, false, s.cigar_begin...));
    DMX_TRY(f(PER_READ, false, s.n_cigar...));
    DMX_TRY(f(PER_READ, false, s.seq_begin...));
    DMX_TRY(f(PER_READ, false, s.l_seq...));
    DMX_TRY(f(PER_OP, false, s.cigar...));
    DMX_TRY(f(PER_BASE, false, s.seq...));
    DMX_TRY(f(PER_BASE, false, s.qual...));
    return 0;
}

// The columns in buffers of the context, laid out as the caller's dmx_decoded_reads: a resident read set, a stream's carry.
struct ReadColumns : ReadCounts {
    DevBuf<int> start, cb, ub, score, n_cigar, l_seq;
    DevBuf<double> p_misaligned;
    DevBuf<long long> cigar_begin, seq_begin;
    DevBuf<unsigned> cigar;
    DevBuf<unsigned char> seq, qual;
};

// A resident read set (include/demux_hip_debug.h "Resident reads"; csrc/resident_reads.hip): the arrays of one dmx_decoded_reads
// in buffers of the context.  Read-only to every pass.
struct ResidentReads {
    ReadColumns columns;
    long long reference_length = 0;  // the largest reference_end (0 without reads)
    bool countable = false;          // the counting-only columns are held (else the set serves coverage only)
    int64_t bytes = 0;               // device bytes held
};

// A resident call set (include/demux_hip_debug.h "Resident calls"; csrc/resident_calls.hip): the two record arrays of one
// CompressedSNPCalls, bytewise the host records, in blocks of the context's cache.  Open while it is filled, read-only once sealed.
// Its blocks are NOT counted in dmx_ctx::bytes (dmx_device_bytes is the problem's and the passes'; dmx_calls_info reports a set's).
struct ResidentCalls {
    unsigned char *molecules = nullptr, *calls = nullptr;  // [cap_molecules * 12], [cap_calls * 13]
    long long n_molecules = 0, n_calls = 0;
    long long cap_molecules = 0, cap_calls = 0;  // records the blocks have room for (0: no block)
    bool sealed = false;
};

// The resident compact result of a pooled pass (include/demux_hip_debug.h "Pooled results kept resident"; csrc/pooled_readout.hip;
// DESIGN.md 4.11): the pool layout, the compact rows and every pool's barcode list in blocks of the context's cache, beside host
// copies of what the entries validate against.  Independent of have_post / d_post; its blocks are NOT counted in dmx_ctx::bytes
// (dmx_pooled_info reports them).
struct PooledSlot {
    bool present = false;
    bool with_doublets = false;
    long long B = 0, n_pools = 0, n_values = 0;
    long long *opt_ptr = nullptr;        // [n_pools + 1] first option of every pool in `opts`
    unsigned *opts = nullptr;            // d1 | d2 << 16 (PoolEstepArgs::opts)
    int *pool_size = nullptr;            // [n_pools]
    int *pool_of = nullptr;              // [B]
    long long *row_ptr = nullptr;        // [B + 1]
    float *post = nullptr, *logits = nullptr;  // compact rows (logits may be absent)
    int *alpha_index = nullptr;          // compact, from the grid passes
    float *alpha_mean = nullptr;         // compact, from the marginal pass
    long long *marg_ptr = nullptr;       // [B + 1] first donor marginal of every barcode (g_p entries each)
    long long *pool_list_ptr = nullptr;  // [n_pools + 1]
    int *pool_list = nullptr;            // every pool's barcodes, ascending
    std::vector<int64_t> h_opt_ptr, h_row_ptr, h_pool_list_ptr, h_marg_ptr;
    std::vector<int> h_pool_size;
    std::vector<int32_t> h_pool_of;
    int64_t bytes = 0;                   // device bytes held
};

// (which derived device data is current: the flags and every write of them are CtxState's, ctx_state.h)
struct dmx_ctx : dmx::CtxState {
    int device = 0;
    hipStream_t stream = nullptr;
    long long B = 0, V = 0, N = 0, S = 0;
    int G = 0, K = 0;
    bool have_problem = false, have_betas = false;

    DevBuf<long long> d_pair_ptr;
    DevBuf<dmx::CallPair> d_call_pairs;
    DevBuf<unsigned> d_call_rows;  // table row of every call of d_call_pairs (EstepArgs::call_rows)
    long long n_pairs = 0;
    DevBuf<uint2> d_csc;
    long long n_csc = 0;  // M-step records held: N, or the calls of this rank's variant slice over the barcodes of all ranks
    DevBuf<long long> d_item_start;
    DevBuf<int> d_item_len;
    DevBuf<long long> d_item_ptr;
    DevBuf<int> d_item_variant;  // [n_items] variant of every work item (MstepArgs::item_variant)
    DevBuf<int> d_bc_order, d_item_order;
    long long n_items = 0;
    // tile-major E-step schedule (repack_device.hip; n_bins == 0: not built)
    long long n_bins = 0;
    int n_tiles = 0, bin_rows_cap = 0;       // rows per bin (<= TILE_R_MAX)
    DevBuf<int> d_bin_rows, d_bin_order;
    DevBuf<long long> d_bin_ptr;          // [n_bins + 1] first stream group of every bin
    DevBuf<dmx::CallPair> d_tile_stream;  // the E-step records once more, in the order the bins consume them
    DevBuf<int> d_v2snp, d_snp_ptr, d_snp_vars;
    DevBuf<float> d_prior, d_add, d_prob;
    DevBuf<float> d_raw;  // the raw betas dmx_set_prior_betas was given (dmx_get_learnt_betas: raw + addition); have_raw
    bool have_raw = false;
    DevBuf<unsigned short> d_prob16;  // d_prob as binary16 at the same row offsets (the coarse pass of the guarded E-step), room for [prob_rows + 1, G]
    DevBuf<unsigned> d_coarse_stream;      // the coarse pass's records (kernels.hip: coarse_walk); built at the first
    DevBuf<long long> d_coarse_bin_ptr;    //   admissible E-step of a problem from the tile-major stream; [n_bins + 1]
    DevBuf<double> d_log2_keep;            // [B]
    bool coarse_ready = false;
    int coarse_pass = 1;                 // dmx_set_coarse_pass
    int lean_memory = 0;                 // dmx_set_lean_memory: the tile-major E-step stream goes once the coarse pass's records are built from it
    bool logits_needed = true;           // dmx_set_logits_needed: the last E-step of a dmx_em / dmx_run_iterations call keeps its logits readable
    DevBuf<double> d_add64, d_partial;
    DevBuf<float> d_logits, d_post;
    DevBuf<unsigned long long> d_nz;
    DevBuf<unsigned long long> d_redo;  // (variant, genotype) sums to be redone in order (k_mcombine)
    DevBuf<unsigned> d_n_redo;
    bool mstep_wide = false;  // dmx_set_mstep_wide_addresses
    // tile-major M-step (kernels.hip: k_mstep_tiles; built on first use by build_mstep_tiles, n_mt == 0: not built / not eligible)
    DevBuf<uint2> d_mt_stream;   // the M-step records once more (with the padding calls' slots when built from the barcode-major records), sorted by (variant tile, barcode row): x = row | variant in tile << 24
    DevBuf<long long> d_mt_ptr;  // [n_mt + 1] first record of every tile
    DevBuf<int> d_mt_first;      // [n_mt + 1] first variant of every tile
    DevBuf<int> d_mt_order;      // [n_mt] tiles by decreasing number of calls
    DevBuf<int> d_mt_shift;      // [n_mt] fixed-point exponent of every tile (MTileArgs::shift)
    DevBuf<unsigned char> d_mt_shift_v;  // [V] the same per variant (incremental M-step, fixed-point work-item form; one context's own records only)
    // incremental M-step (kernels.h: MIncrArgs): the tiles' integer sums and the posteriors they were formed from, kept between M-steps
    DevBuf<unsigned long long> d_acc64;  // [V, G]
    DevBuf<float> d_prev_post;           // [B, G]
    DevBuf<uint2> d_prev_first;          // [B]
    DevBuf<int> d_incr_list;             // [B]
    DevBuf<unsigned char> d_incr_touched;  // [V]
    DevBuf<unsigned> d_incr_state;       // [2 x IS_WORDS] the state words of this and of the next M-step, alternating
    int incr_parity = 0;
    int mstep_incremental = 1;              // dmx_set_mstep_incremental
    long long mstep_incr_launches = 0;      // M-steps that went through the incremental launch sequence
    long long n_mt = 0;
    std::vector<long long> h_col_ptr;  // [V + 1] first M-step record of every variant (host copy made by the repack: the tiles are cut from it)
    int mt_tv = 0;                  // variants per tile at most
    bool mt_tried = false;          // a build was attempted for the resident M-step records
    bool mt_shift_tried = false;    // ... the tile cut for the exponents alone (plan_mstep_shifts)
    int mstep_tiles = 1;            // dmx_set_mstep_tiles: 0 never, 1 when building the records pays, 2 always
    long long msteps_done = 0;      // M-steps run on the resident problem
    long long incr_rows = 0;        // barcode rows the incremental state was allocated for (a variant-sharded rank: those of all ranks)
    DevBuf<unsigned char> d_incr_map;  // [incr_rows] flags of the changed barcodes (variant-sharded rank: MIncrArgs::changed_map)
    // variant-sharded rank, incremental M-step: the slice's records once more, BARCODE-major over the rows of all ranks ({variant, bits(1-e)},
    // a row's calls by variant; build_slice_row_index at the first incremental M-step) - the delta pass reads the changed barcodes' calls only
    DevBuf<uint2> d_slice_rec;         // [calls of the slice]
    DevBuf<long long> d_slice_ptr;     // [incr_rows + 1]
    bool slice_index_tried = false;
    bool incr_heavy = false;        // the incremental M-step keeps falling back to full passes on this problem: the tile-major records pay (run_mstep)
    int msteps_ahead = 0;           // M-steps the running dmx_em / dmx_run_iterations call still has to do (0 outside)
    long long msteps_expected = 0;  // dmx_set_msteps_expected: M-steps the caller says it will still run (counted down as they run)
    double mt_build_ms = 0.0;       // host wall time of the last build of the tile-major records
    int mstep_form = 0;             // form of the last M-step launch: 0 none, 1 work items, 2 tiles, 3 fixed-point work items (dmx_get_mstep_form; mstep_plan.h)
    DevBuf<int> d_sum_plan;  // np.sum over a row of K values as a leaf / level plan (dmx_api.cpp: ensure_options)
    long long sum_plan_k = -1;
    int sum_plan_values = 0;    // leaves + inner nodes
    int item_calls = 1024;  // work-item length of the resident problem (kernels.h: item_calls_for)
    bool exact_additions = true;  // dmx_set_exact_additions
    int estep_mode = DMX_ESTEP_EXACT;  // dmx_set_estep_mode
    // guarded mode: barcodes queued by the epilogues of the fast kernels for the exact redo (kernels.h: EstepArgs::guard)
    DevBuf<unsigned> d_guard_count;  // [GUARD_STATE_WORDS] device state of the guarded mode (kernels.h: GS_*)
    int guard_adaptive = 1;             // dmx_set_guard_adaptive: the device picks coarse pass / fine pass / the exact kernel on every barcode per E-step from its own timings
    DevBuf<int> d_guard_list;        // [B] EstepArgs::guard_list
    DevBuf<int> d_guard_sub;         // [GUARD_QUEUES x guard_sub_cap] EstepArgs::guard_sub
    unsigned guard_sub_cap = 0;
    long long guard_rows_total = 0;     // barcode rows the guarded kernels have walked since the last reset
    int tiled_estep = 1;               // dmx_set_estep_schedule: 0 never, 1 when it pays, 2 whenever the repack built one
    // dictionary form of the E-step (estep_dict.hip): tried when the genotype table was computed without a beta
    // addition (or supplied by the caller), used when every row has few distinct values
    int dict_mode = 1;            // dmx_set_estep_dictionary: 0 never, 1 when the table is a candidate, 2 try always
    int estep_form = 0;           // form of the last E-step: DMX_FORM_*
    int estep_packing = 1;        // dmx_set_estep_packing: 0 never, 1 where it pays, 2 wherever the shape exists
    long long max_row_calls = 0;  // calls of the longest barcode row (device repack)
    int n_simd = 0;               // SIMDs of the device (4 per CU)
    long long long_row_calls[3] = {0, 0, 0};  // calls per SIMD at 8 / 4 / 2 barcodes per wavefront (device repack) ...
    long long n_long_rows[3] = {0, 0, 0};     // ... and how many barcode rows have more
    int dict_distinct = 0;        // most distinct values per row found by the last dictionary build (0: none built)
    DevBuf<float> d_dict;             // [prob_rows, DICT_CAP]
    DevBuf<unsigned char> d_codes;    // [prob_rows, G]
    DevBuf<unsigned char> d_dtab;     // the packed table the kernel reads (estep_dict.hip: DictRow)
    DevBuf<unsigned> d_dict_stat;     // [1]
    // split rows of the tolerance / guarded E-step (kernels.h: EstepArgs::segs; dmx_api.cpp: build_row_segments)
    DevBuf<dmx::EstepSegment> d_segs;
    DevBuf<int> d_split_first;
    DevBuf<double> d_seg_sums;
    long long n_segs = 0, n_split = 0;
    int live_floor_grid = 1;   // dmx_set_live_floor_on_grid: an E-step ahead of a fixed-point M-step writes them at live_floor_fixed (kernels.h)
    DevBuf<uint2> d_first;  // [B] {posterior of the lowest live singlet column, count | first live columns} (G <= 64): EstepArgs::first
    DevBuf<unsigned long long> d_dense_calls;  // [1] E-step statistic read by the M-step kernels (kernels.h)
    DevBuf<float> d_pen;
    DevBuf<unsigned> d_pairs;
    DevBuf<unsigned> d_pair_blocks;  // EstepArgs::pair_blocks (doublet runs whose options go to the workgroup-per-barcode forms)
    int n_pair_blocks = 0;
    DevBuf<unsigned char> d_prior_logits;
    DevBuf<int> d_best;
    DevBuf<float> d_bestp;
    // unique (variant, barcode) calls left by the device pack (variant-major), kept for dmx_get_packed_calls
    DevBuf<int> d_u_variant, d_u_cb;
    DevBuf<float> d_u_p;
    DevBuf<long long> d_u_count;
    long long n_u = 0;
    DevBuf<unsigned long long> d_mol;  // matched molecule calls per variant (device pack), for the data prior
    // aggregate_on_snps (snp_aggregate.hip): matched molecule calls grouped by (barcode, SNP)
    bool keep_molecule_calls = false;     // dmx_set_keep_molecule_calls: the device pack leaves them behind
    DevBuf<int> d_mc_variant;          // [molecule calls] variant row | 0x80000000 on the first call of a pair
    DevBuf<float> d_mc_e;              // [molecule calls] p_base_wrong
    DevBuf<long long> d_mc_start;      // [B + 1] first call of every barcode
    unsigned mc_max_count = 0;            // most molecule calls in one (barcode, SNP) pair
    DevBuf<double> d_logits64, d_post64;  // float64 results of dmx_estep_snp
    DevBuf<unsigned char> d_scratch;  // self tests
    // SNP detection (snp_detect.hip): read and written by the dmx_snp_* entry points only; sd_P < 0: no counts
    DevBuf<unsigned long long> d_sd_pos;  // [sd_P] chrom << 32 | (position ^ 0x80000000), ascending (the canonical order)
    DevBuf<int> d_sd_counts;              // [sd_P, sd_D, 4]
    DevBuf<double> d_sd_imp;              // [sd_P, sd_D] importances (dmx_snp_score)
    long long sd_P = -1;
    int sd_D = 0;
    bool sd_scored = false;
    // read counting (count_reads.hip): the records of the last dmx_count_reads; cr_molecules < 0: none
    DevBuf<unsigned char> d_cr_molecules;  // [cr_molecules] packed 12-byte molecule records
    DevBuf<unsigned char> d_cr_calls;      // [cr_calls] packed 13-byte call records
    long long cr_molecules = -1, cr_calls = 0;
    double cr_stage_ms[dmx::COUNT_READS_STAGES] = {};
    int64_t cr_peak_bytes = 0;  // scratch + input the last call or push held at its end, when it holds the most (dmx_get_count_reads_peak_bytes)
    long long cr_carried = 0;   // reads the last push left as the carry (dmx_get_count_reads_carry)
    // streamed read counting (dmx_count_reads_begin / _push / _end; one stream per context): the stream's positions and quality
    // table, and the carry: the reads of the molecules no event has flushed yet, in read order, a ReadColumns of their own
    DevBuf<int> d_crs_positions;  // [crs_P]
    DevBuf<double> d_crs_table;   // [41]
    ReadColumns crs_carry;        // crs_carry.n reads, their operations and bases behind one another; allocated while n > 0
    int crs_state = 0;  // 0: no stream, 1: open, 2: the final push is done, 3: a push failed (count_reads.hip: STREAM_*)
    long long crs_P = 0;
    long long crs_molecules = 0;       // molecules the stream has emitted: the molecule_index of the next push counts on from here
    long long crs_previous_start = 0;  // reference_start of the last read of the last non-empty chunk ...
    bool crs_has_previous = false;     // ... if there was one
    // coverage (coverage.hip): the counts of the last dmx_coverage_count and the candidates of the last dmx_coverage_candidates,
    // read and written by the dmx_coverage_* entry points only; cov_W < 0: no window counted, cov_candidates < 0: none selected
    DevBuf<int> d_cov_counts;       // [4, cov_W] rows A, C, G, T
    DevBuf<int> d_cov_cand_pos;     // [cov_candidates] absolute positions, ascending
    DevBuf<int> d_cov_cand_counts;  // [cov_candidates, 4]
    long long cov_W = -1, cov_start = 0, cov_candidates = -1;
    int coverage_form = DMX_COVERAGE_TILED;  // dmx_set_coverage_form
    double cov_stage_ms[dmx::COVERAGE_STAGES] = {};
    // resident read sets (resident_reads.hip): the caller's, by handle; they outlive dmx_release_problem, dmx_destroy frees them
    std::map<int64_t, ResidentReads> resident_reads;
    int64_t reads_upload_bytes = 0;  // decoded-read arrays copied host to device so far (dmx_get_reads_upload_bytes)
    // resident call sets (resident_calls.hip): the caller's, by handle, with the life cycle of the resident read sets
    std::map<int64_t, ResidentCalls> resident_calls;
    int64_t calls_transfer_bytes[2] = {0, 0};  // call records copied host to device / device to host so far (dmx_get_calls_transfer_bytes)
    // the pooled slot (pooled_readout.hip): dmx_release_problem and dmx_destroy drop it; nothing of the dense path reads or writes it
    PooledSlot pooled;
    int keep_pooled = 0;  // dmx_set_keep_pooled: dmx_estep_pools, dmx_estep_ambient and the two grid passes leave their compact result there

    // ---- multi-GPU (dmx_api.cpp: "exchange") ----
    // The [V, G] tables that cross ranks live in a PADDED row layout: the variants are cut into nranks slices at
    // SNP boundaries, every slice padded to slice_rows rows, so that slice r of any such table is the contiguous,
    // equally sized block ncclReduceScatter / ncclAllGather want.  prow(v) = padded row of variant v.  With one
    // rank (or SNPs whose variants are not contiguous: `sliced` false) the layout is the dense one.
    ncclComm_t comm = nullptr;                // RCCL communicator (dmx_comm_init), or
    dmx_host_collective host_coll = nullptr;  // the caller's collectives over host buffers (dmx_comm_init_host)
    void *host_user = nullptr;
    void *h_stage = nullptr;                  // pinned staging of the host collectives
    size_t h_stage_bytes = 0;
    // Emulated wire (dmx_comm_init_emulated): the collectives move nothing between processes - this rank's block is copied
    // where the collective would leave it, then the stream waits for the modelled wire time.  For measuring what of the
    // exchange a schedule leaves exposed on a box with one GPU; the results of such a run are not a real EM.
    bool emulated = false;
    double emu_link_gbps = 50.0, emu_latency_us = 10.0;
    bool in_group = false, group_paid = false;  // coll_group_begin .. coll_group_end: several collectives, one launch
    double group_ns = 0.0;                       // emulated wire: the group's modelled time, held by ONE delay at its end
    double emu_ticks_per_ns = 0.1;            // wall-clock ticks of the delay kernel per nanosecond
    bool attached() const { return comm != nullptr || host_coll != nullptr || emulated; }
    int rank = 0, nranks = 1, reduce_dtype = DMX_F64;
    bool sliced = false;            // reduce-scatter + sliced P-step + all-gather (else: all-reduce + replicated P-step)
    long long slice_rows = 0;       // rows per slice of the padded tables
    long long prob_rows = 0;        // rows of d_prob (= nranks * slice_rows when sliced, else V)
    std::vector<long long> cut;     // [nranks + 1] first variant of every slice
    std::vector<int> h_v2snp;       // host copy of v2snp (layout decisions)
    DevBuf<int> d_prow;          // [V] padded row of every variant (sliced mode)
    DevBuf<int> d_row_variant;   // [prob_rows] ... and back (padding rows: variant 0; the incremental M-step of a rank that exchanges sums)
    // M-step sharded on variants (dmx_api.cpp: shard_mstep_by_variant): d_csc and the work items hold the calls of this rank's
    // variant slice from the barcodes of ALL ranks; the three tables the M-step reads of a barcode are global
    // (row = owner rank * rows_pad + barcode), filled block by block by the ranks' E-steps and all-gathered
    bool mshard = false;
    long long rows_pad = 0, rows_total = 0;  // barcode rows per rank block / of all ranks
    DevBuf<uint2> d_first_g;              // [rows_total] EstepArgs::first of every barcode
    DevBuf<unsigned long long> d_nz_g;    // [rows_total, ceil(G / 64)]
    DevBuf<float> d_post_g;               // [rows_total, G] singlet posteriors
    bool emu_post_filled = false;            // emulated wire: the other ranks' blocks were filled once
    // compact exchange of the posterior rows (gather_posteriors; G <= 64): per rank a block of {rows listed, 3 pad, cap x (row, G floats)}
    DevBuf<unsigned> d_post_compact;      // [nranks * post_compact_words]
    DevBuf<uint2> d_post_seen;            // [rows_total] the code every row of d_post_g was last rebuilt from (0xFF..: unknown)
    DevBuf<float> d_post_sent;            // [B, G] this rank's rows with several live posteriors as the other ranks hold them ...
    DevBuf<unsigned char> d_post_sent_multi;  // [B] ... where they do (0: the row was rebuilt from its code since, or never listed)
    unsigned *h_post_counts = nullptr;       // pinned, [nranks + 1]: the lists' lengths, read behind the all-gather, and the sequence number the host polls
    unsigned list_seq = 0;                   // (k_post_counts / wait_counts)
    size_t post_compact_words = 0;           // words per rank block (0: the whole table travels, as until round 6)
    unsigned post_compact_cap = 0;           // rows a block can list at most
    unsigned post_cap_now = 0;               // ... in the coming exchange: twice what the longest list of the last one held (every rank reads every count: the same choice everywhere)
    long long post_compact_taken = 0, post_compact_overflows = 0;  // E-steps exchanged compactly / that fell back to the whole table
    // compact exchange of the genotype table (run_pstep; sliced P-step): the rows of this rank's slice that changed since it sent them
    DevBuf<unsigned> d_prob_list;         // [nranks * prob_list_words] {rows listed, 3 pad, cap x (row, G floats)} per rank
    DevBuf<float> d_prob_prev;            // [slice_rows, G] this rank's slice as the other ranks hold it
    size_t prob_list_words = 0;              // (0: the whole slices travel)
    unsigned prob_list_cap = 0;
    unsigned prob_cap_now = 0;               // (as post_cap_now)
    unsigned *h_prob_counts = nullptr;       // pinned, [nranks + 1]
    long long prob_compact_taken = 0, prob_compact_overflows = 0;
    DevBuf<unsigned char> d_exch;         // padded send buffer of the reduce-scatter (float64 or float32 partial sums; the incremental
                                          // M-step keeps them there between two M-steps, the padding rows stay zero)
    DevBuf<unsigned char> d_recv;         // this rank's reduced slice
    DevBuf<unsigned char> d_add_stage;    // [nranks * slice_rows, G] float32: the all-gather of the addition's slices (ensure_full_addition)

    // flat call arrays of staged containers (dmx_stage_containers -> dmx_pack_staged_and_set_problem); n_staged < 0: none
    int *st_chrom = nullptr, *st_pos = nullptr, *st_cb = nullptr;
    unsigned char *st_base = nullptr;
    float *st_p = nullptr;
    long long n_staged = -1;
    int64_t bytes = 0;
    TimerSlot timers[DMX_T_COUNT];
    bool phase_timers = false;  // dmx_set_phase_timers: events around the phases (off: the launch counts only)
    std::vector<TimerStamp *> idle_stamps;
    TimerStamp *boundary = nullptr;  // the stamp the last phase ended on, while nothing else has been enqueued behind it (bind() clears it)

    // Device blocks this context has released, kept for its next allocations (ctx_malloc / ctx_free below).
    std::multimap<size_t, void *> idle_blocks;          // capacity -> block
    std::unordered_map<void *, size_t> block_capacity;  // every block handed out through ctx_malloc, idle or not
    size_t idle_bytes = 0;
    std::mutex cache_lock;  // the three above: another context's out-of-memory retry may trim this one's idle blocks
};

// Why the context keeps its device blocks: a second predict / learn call on a context frees the previous problem
// (gigabytes in ~100 blocks) and allocates the next one, and on this stack ONE hipMalloc after such a round of hipFree
// took 350 ms (rocprofv3 --hip-trace of scripts/e2e_breakdown.py: 87 ms for the first pack of 78.65 M calls, 430 ms for
// every later one).  Blocks go back to the context that allocated them and are handed out again to requests of
// (nearly) their size; everything a context launches is ordered on its stream, so a block can be re-used while the
// work of its previous life is still queued.  DEMUXALOT_AMD_CACHE_GB caps the idle bytes per context (default 24; 0 =
// free at once).  dmx_destroy and dmx_trim release them.
size_t ctx_cache_limit();
int ctx_malloc(dmx_ctx *c, void **p, size_t bytes);
void ctx_free(dmx_ctx *c, void *p);
void ctx_trim(dmx_ctx *c, size_t keep_bytes);
void ctx_retire(dmx_ctx *c);  // dmx_destroy: idle blocks to the device's retired list (for contexts created later)
void ctx_register(dmx_ctx *c);    // dmx_create / dmx_destroy: the live contexts of a device, whose idle blocks an
void ctx_unregister(dmx_ctx *c);  // out-of-memory retry anywhere on that device may give back
size_t trim_device_caches(int device);  // idle blocks of every live context + the retired list; returns the bytes freed

// The context's buffers of the block cache, counted in c->bytes (dmx_device_bytes).  A buffer of no elements takes the
// room of one: every allocation is a block of its own.
template <typename T>
inline size_t dev_bytes(const DevBuf<T> &b)
{
    return (b.n ? b.n : 1) * sizeof(T);
}

template <typename T>
inline int dev_alloc(dmx_ctx *c, DevBuf<T> &b, size_t n)
{
    b = DevBuf<T>{nullptr, n};
    if (const int rc = ctx_malloc(c, (void **)&b.p, dev_bytes(b))) {
        b = DevBuf<T>();
        return rc;
    }
    c->bytes += (int64_t)dev_bytes(b);
    return 0;
}

template <typename T>
inline void dev_free(dmx_ctx *c, DevBuf<T> &b)
{
    if (b.p) {
        ctx_free(c, (void *)b.p);
        c->bytes -= (int64_t)dev_bytes(b);
    }
    b = DevBuf<T>();
}

// room for n elements at least: a smaller buffer is freed and allocated anew (its contents go)
template <typename T>
inline int dev_grow(dmx_ctx *c, DevBuf<T> &b, size_t n)
{
    if (n <= b.n) return 0;
    dev_free(c, b);
    return dev_alloc(c, b, n);
}

// A ReadColumns as a whole: buffers for `counts` elements (the counting-only columns only where asked for; a failure leaves
// what was allocated to free_read_columns), all of them back, the bytes of those that are held.
inline int alloc_read_columns(dmx_ctx *c, ReadColumns &cols, const ReadCounts &counts, bool with_counting)
{
    static_cast<ReadCounts &>(cols) = counts;
    return each_read_column([&](ReadExtent e, bool counting, auto &b) { return counting && !with_counting ? 0 : dev_alloc(c, b, counts.of(e)); }, cols);
}

inline void free_read_columns(dmx_ctx *c, ReadColumns &cols)
{
    (void)each_read_column([&](ReadExtent, bool, auto &b) { return dev_free(c, b), 0; }, cols);
    cols = ReadColumns();
}

inline size_t read_columns_bytes(const ReadColumns &cols)
{
    size_t bytes = 0;
    (void)each_read_column([&](ReadExtent, bool, const auto &b) { return bytes += b.p ? dev_bytes(b) : 0, 0; }, cols);
    return bytes;
}

// hipMalloc / hipFree outside the block cache (the exchange's buffers, the prior logits), counted in c->bytes as well
int raw_alloc(dmx_ctx *c, DevBuf<unsigned char> &b, size_t bytes);
void raw_free(dmx_ctx *c, DevBuf<unsigned char> &b);


namespace dmx {
// Derives the E-step call records (barcode-major, padded pairs), the M-step records
// (variant-major), the work items and the length-sorted work lists on the GPU from the
// uploaded COO columns, and stores them in the ctx (repack_device.hip).
int repack_on_device(dmx_ctx *c, const int32_t *h_variant, const int32_t *h_cb, const float *h_p);
// Variant matching + de-duplication of molecule calls on the GPU (demux.py:276-300, 332-365), then the
// layouts; sets c->N to the number of unique calls.
int pack_on_device(dmx_ctx *c, long long V, const int *var_chrom, const int *var_pos, const unsigned char *var_base,
                   long long n_calls, const int *call_chrom, const int *call_pos, const unsigned char *call_base,
                   const int *call_cb, const float *call_p, long long *n_matched, long long *n_unique,
                   long long *mol_per_variant);
// matched molecule calls (molecule order) -> the (barcode, SNP)-grouped layout of the aggregate_on_snps E-step
int ensure_sum_plan(dmx_ctx *c, long long K);  // dmx_api.cpp
// multi-GPU, M-step records by variant slice (repack_device.hip)
int wire_records_of(dmx_ctx *c, long long row_base, uint4 *d_out, long long capacity);
int install_mstep_records(dmx_ctx *c, const uint4 *d_rec, long long n, long long v_lo, long long v_hi);
// tile-major M-step records of variants [v_lo, v_hi) (the ctx's M-step records must cover exactly those); leaves n_mt == 0
// when the problem does not fit the form
int build_mstep_tiles(dmx_ctx *c, long long v_lo, long long v_hi);
int build_slice_row_index(dmx_ctx *c);  // d_slice_rec / d_slice_ptr of a variant-sharded rank (left null where it does not apply)
int plan_mstep_shifts(dmx_ctx *c);  // the tiles' fixed-point exponents per variant without the tile-major records (fixed-point work-item M-step)
void release_mstep_tiles(dmx_ctx *c);
int build_snp_groups(dmx_ctx *c, const unsigned long long *vb_keys, const unsigned *src_idx, const float *src_p, long long m);
int stage_containers_on_device(dmx_ctx *c, const dmx_call_container *parts, int n_parts);
// the same from views of resident call sets: the pointers are device memory (checked by the caller), nothing is uploaded
int stage_device_containers(dmx_ctx *c, const dmx_call_container *views, int n_views);
int pack_staged_on_device(dmx_ctx *c, long long V, const int *var_chrom, const int *var_pos, const unsigned char *var_base,
                          const int *chrom_table, int n_table, long long *n_matched, long long *n_unique, long long *mol_per_variant);
void release_staged_calls(dmx_ctx *c);
int pack_containers_on_device(dmx_ctx *c, long long V, const int *var_chrom, const int *var_pos,
                              const unsigned char *var_base, const dmx_call_container *parts, int n_parts,
                              long long *n_matched, long long *n_unique, long long *mol_per_variant);
}  // namespace dmx
