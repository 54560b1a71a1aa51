// estep_plan.h -- the E-step's policy as pure functions of plain values: which arithmetic runs, whether the dictionary or the packed form
// takes the E-step, what a guarded E-step builds, releases and converts, what its fine level walks, and which kernel a launch is.
// Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp: run_estep fills Facts from the context, asks these in stages (a build, a
// release or a download may change what is there: it refreshes the facts behind them) and acts on the answers; kernels.hip: launch_estep asks
// kernel() once and switches on the answer; kernels.h includes this header, so device code sees the same constants;
// tests/estep_plan_check.cpp walks the fact space on the CPU; the table: DESIGN.md 4.1.
#pragma once

namespace dmx {
namespace eplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

enum Mode { MODE_EXACT = 0, MODE_FAST = 1, MODE_GUARDED = 2 };  // (the values of DMX_ESTEP_*)

struct Facts {
    Mode mode;                  // dmx_set_estep_mode
    bool with_doublets;         // the option table is the pairs' (K = G (G + 1) / 2), else the singlets' (K = G)
    bool with_prior;            // prior logits are added
    bool logits_kept;           // somebody can read this E-step's logits (it is the last one of the call)
    int G;                      // genotypes
    int K;                      // options
    long long B;                // barcodes
    long long table_rows;       // rows of the genotype table (prob_rows)
    int schedule;               // dmx_set_estep_schedule: 0 never, 1 when it pays (tolerance arithmetic), 2 whenever built
    long long n_bins;           // bins of the tile-major schedule the repack built (0: not built for this problem)
    bool tile_stream;           // its call records are there (dmx_set_lean_memory releases them)
    bool coarse_ready;          // the coarse pass's records are built
    int coarse_pass;            // dmx_set_coarse_pass: 0 never, 1 where nobody reads the logits, 2 also where somebody does
    bool guard_adaptive;        // the device chooses the level of a guarded E-step (dmx_set_guard_adaptive)
    bool lean_memory;           // dmx_set_lean_memory
    float lo;                   // lower clip of the P-step that wrote the table
    bool prob16_valid;          // the binary16 table is the current one
    bool sliced;                // the table travels in slices (reduce-scatter runs) ...
    bool table_lists;           // ... as lists of changed rows
    int dict_mode;              // dmx_set_dictionary: 0 never, 1 where it pays, 2 wherever it exists
    bool dict_candidate;        // the table was written without addition (few distinct values per row are likely)
    bool call_rows;             // the dictionary form's row array is there (dmx_set_lean_memory releases it)
    bool records_below_4g;      // the barcode-major records take 32-bit offsets
    int packing;                // dmx_set_estep_packing: 0 never, 1 where it pays, 2 every barcode packed, 3 the split wherever the shape exists
    bool row_statistic;         // the repack counted the long rows (not a host-packed problem)
    long long n_long_rows[3];   // barcodes with more calls than a third of a SIMD's share, for 8 / 16 / 32 lanes per barcode
    bool segments;              // split rows were cut (build_row_segments)
    int n_pair_blocks;          // 2 x 3 blocks of the option triangle (ensure_options; 0: none)
};

// ---- the shapes, each once ----
// the tile-major schedule's kernels (k_estep_tiled, _coarse, _fine8) exist for singlet tables of 17 .. 128 genotypes
inline bool singlet_tile_shape(int K, bool pairs) { return !pairs && K > 16 && K <= 128; }
// Workgroup-per-barcode shape: option tables beyond 1024; doublet tables of more than 512 options (256 with the tolerance arithmetic):
// with 16 accumulators + two row offsets per lane the lane-per-option form is down to 2 (1) waves per SIMD
// (20k x 20k x 32 with doublets, K = 528: 3.50 -> 2.97 ms, tolerance mode 4.54 -> 1.49 ms; at K = 496 it is still
// ahead in the exact mode, 2.44 against 2.65 ms, and behind in the tolerance mode, 2.04 against 1.20 ms).
inline bool block_shape(int K, bool pairs, bool fast) { return K > 1024 || (pairs && (K > 512 || (fast && K > 256))); }
// lanes per barcode of the dictionary form's lane kernel (estep_dict.hip: k_estep_dictq; doublet runs: at least 8)
inline int dict_lanes(int K, bool pairs) { return K <= 16 && !pairs ? 4 : K <= 32 ? 8 : K <= 64 ? 16 : K <= 128 ? 32 : 64; }
constexpr int DICT_CAP = 8;       // distinct values per row the dictionary form handles (singlet runs)
constexpr int DICT_PAIR_CAP = 4;  // ... in doublet runs (10 pair values)
constexpr int DICT_LANE_K = 256;  // option tables up to this width take the lane-per-four-options dictionary kernel
// Lane-group shape of the packed form (estep_packed.hip) for a doublet table of K options over G genotypes; false: the direct form is as good or better.
inline bool estep_packed_shape(int K, int G, int *lanes, int *slots)
{
    constexpr int shapes[][2] = {{8, 3}, {8, 5}, {16, 3}, {16, 5}, {32, 3}, {32, 5}};
    int direct = 4;  // slots the direct form spends on a row: next power of two up to 64, then multiples of 64 x {1, 2, 4, 8, 16}
    while (direct < K && direct < 64) direct <<= 1;
    while (direct < K) direct <<= 1;
    int best = direct, bl = 0, ba = 0;
    for (const auto &sh : shapes) {
        const int cap = sh[0] * sh[1];
        if (cap >= K && G <= sh[0] && cap < best) {
            best = cap;
            bl = sh[0];
            ba = sh[1];
        }
    }
    if (!bl) return false;
    *lanes = bl;
    *slots = ba;
    return true;
}
// the coarse pass's records (launch_build_coarse_stream): cpg = calls per gather: 1 for 65 .. 128 genotypes, 2 for 33 .. 64, 4 for 17 .. 32
constexpr int coarse_calls_per_gather(int K) { return K > 64 ? 1 : K > 32 ? 2 : 4; }
constexpr int coarse_batches_per_record(int cpg) { return cpg; }  // (kernels.hip: CoarseShape<CPG>::BPR)
// The guard's allowances per call (estep_epilogue.h: GUARD_PER_CALL is the tolerance arithmetic's own).
constexpr float GUARD_PER_CALL_PLAIN = 7.0e-8f;
// The fine pass on the coarse pass's records (kernels.hip: k_estep_tiled_fine8; the tile-major stream released: dmx_set_lean_memory): float32 table,
// float64 sums, a term keep (p + r): 4 x 2^-24 relative against the reference's float32 term (r's division, the sum's rounding, the
// reference's two), the slot tag in one r of a block's 8 / cpg per batch (2^-19 of r <= 1.91e-6 of the term), the product's roundings and
// the mantissa's log as GUARD_PER_CALL prices them.  Every block of a barcode's batch carries exactly one tagged r and the guard counts
// padded calls, so the tag is charged to one call in 8 / cpg.
inline float guard_per_call_fine8(int cpg) { return 1.91e-6f / (float)(8 / cpg) + 4.0f * 6.0e-8f + 7.0e-8f; }

inline long long bins(const Facts &f) { return f.schedule ? f.n_bins : 0; }  // the schedule as the E-step may use it
// (dmx_set_lean_memory: the tile-major schedule is the singlet runs'; a run with doublets never reads its stream - 6.4 GB of configs[4])
inline bool unused_stream_release_due(const Facts &f) { return f.lean_memory && f.with_doublets && f.tile_stream && !f.coarse_ready; }
// split rows are the lane-per-option forms' (kernels.h: EstepArgs::segs)
inline bool segments_offered(const Facts &f) { return f.segments && f.K <= 1024; }

// ---- arithmetic ----
// Guarded mode: the tolerance-mode kernels wherever a lane-per-option one exists (estep_epilogue.h: estep_guard), the exact mode for
// the workgroup-per-barcode shapes with a prior: those forms - option tables beyond 1024, doublet tables beyond 256 - evaluate the guard
// in k_softmax_rows from the logits alone, which does not cover prior logits.  (So the guarded mode never brings the tolerance arithmetic
// to a doublet table of 257 .. 512 options without the block shape: block_shape above is what the launch asks with the same answer.)
inline bool guarded(const Facts &f) { return f.mode == MODE_GUARDED && !(block_shape(f.K, f.with_doublets, true) && f.with_prior); }
inline bool tolerance_arithmetic(const Facts &f) { return f.mode == MODE_FAST || guarded(f); }

// ---- the coarse pass ----
// Whether the E-step behind a P-step with clip `lo` can take the coarse pass (kernels.hip: k_estep_tiled_coarse): singlets, 17 .. 128
// genotypes, the tile-major schedule, a table whose clip keeps binary16 normal, the table and its all-zero row below 4 GiB.  Its records
// are there, or can be built from the tile-major stream (dmx_set_lean_memory releases that one behind the build).  Asked by run_estep of
// the table it finds and by dmx_em / dmx_run_iterations ahead of the P-step that writes it.
inline bool coarse_capable(const Facts &f, float lo)
{
    return f.coarse_pass && f.mode == MODE_GUARDED && singlet_tile_shape(f.K, f.with_doublets) && bins(f) > 0 && (f.coarse_ready || f.tile_stream) &&
           lo >= 6.2e-5f && ((unsigned long long)f.table_rows + 1ull) * (unsigned long long)f.G * 4ull < (1ull << 32);
}

// ---- the dictionary form (estep_dict.hip), three stages ----
// It is exact and faster than the fine pass, but not than the COARSE pass (200k x 100k x 64: 1.1 ms with its dictionary build against
// 0.75): an E-step whose logits nobody reads - the first of a dmx_em call of several iterations - takes the coarse pass like the ones
// behind it (its records are built there instead of one E-step later), and the dictionary is not tried.
inline bool coarse_first(const Facts &f) { return !f.logits_kept && f.guard_adaptive && coarse_capable(f, f.lo) && f.dict_mode == 1; }
inline bool dictionary_block_form(const Facts &f) { return f.with_doublets && f.K > DICT_LANE_K; }  // wide doublet tables: workgroup per barcode
// everything that is known before anything is built
inline bool dictionary_admissible(const Facts &f)
{
    const bool wanted = f.dict_mode == 2 || (f.dict_mode == 1 && f.dict_candidate);
    if (!wanted || f.mode == MODE_FAST || f.B == 0 || f.table_rows == 0) return false;  // (guarded: exact and faster)
    const bool block_form = dictionary_block_form(f);
    if (!f.call_rows) return false;  // (dmx_set_lean_memory: the form's row array was released)
    // singlet tables beyond 256: the direct forms; 24-bit row x pitch; 32-bit record offsets
    if (!block_form && (f.K > DICT_LANE_K || f.table_rows >= (1 << 24) || !f.records_below_4g)) return false;
    if (block_form && (unsigned long long)f.G * 72 + 9 * 1024 > 160 * 1024) return false;  // the code rows of a chunk must fit the LDS
    if (f.G > 1024) return false;  // widest k_build_dict instantiation (ensure_options refuses such runs anyway)
    if (f.dict_mode == 1 && !block_form) {
        // Where the lane form pays (measured): singlet runs with enough barcodes for several rounds of
        // wavefronts.  A launch of one round lasts as long as its longest barcode, whose calls this form walks in
        // batches with a memory latency each (20k x 10k x 64: 0.31 ms against 0.25 ms direct), and the 16 entry slots of
        // a doublet run leave two calls per barcode and batch (20k x 20k x 8 with doublets: 0.60 against 0.28 ms).
        if (f.with_doublets || f.B * dict_lanes(f.K, false) / 64 < 8192) return false;
    }
    return true;
}
// ... behind the build and its one download: `distinct` = most distinct values in a row (0 / beyond the cap: some row does not fit);
// `pitch` = bytes per row of the lane form's packed table (dict_table_pitch; the block form reads the build's arrays themselves)
enum DictForm { DICT_NONE, DICT_LANE, DICT_BLOCK };
inline DictForm dictionary_candidate_form(const Facts &f, unsigned distinct)  // the caps alone: what the pitch is computed for
{
    if (distinct == 0 || distinct > (unsigned)(f.with_doublets ? DICT_PAIR_CAP : DICT_CAP)) return DICT_NONE;
    return dictionary_block_form(f) ? DICT_BLOCK : DICT_LANE;
}
inline DictForm dictionary_form(const Facts &f, unsigned distinct, unsigned long long pitch)
{
    const DictForm form = dictionary_candidate_form(f, distinct);
    return form == DICT_LANE && (unsigned long long)f.table_rows * pitch >= (1ull << 32) ? DICT_NONE : form;  // buffer addressing
}

// ---- the packed form (estep_packed.hip; neither dictionary form runs) ----
// Several option slots per lane make a barcode's serial walk `slots` times longer, and a launch
// lasts at least as long as its longest barcode.  So the barcodes with more calls than a third of what a SIMD
// gets on average (counted by the repack) walk on 64 lanes inside the same launch; when that is more than an
// eighth of them the problem is one of few, long rows and the direct form takes it.  20k x 20k x 8 with
// doublets (longest row 3 500 calls): all packed 0.72 ms, split at 1 000 / 2 000 rows 0.32 / 0.30 ms, direct
// 0.28 ms - the wavefronts of a launch that fits the chip at once stay where they were placed, the heaviest
// 64-lane walks next to the heaviest packed ones; see DESIGN.md 4.1c.  Mode 2: every barcode packed; 3: the split
// wherever the shape exists.
// (guarded mode: where the packed form is taken it is exact AND faster than the tolerance-mode kernel on 64 lanes -
// 200k x 20k x 8 with doublets: 1.94 against 2.08 ms -, so it runs as it is, without guard and without the tolerance arithmetic)
struct Packed {
    bool shape;        // the form exists for the problem
    bool split;        // long rows walk on 64 lanes (not mode 2)
    long long n_long;  // ... that many of them (the first entries of the order)
};
inline Packed packed_candidate(const Facts &f)
{
    int lanes = 0, slots = 0;
    if (!(f.packing && f.with_doublets && f.mode != MODE_FAST && f.records_below_4g && estep_packed_shape(f.K, f.G, &lanes, &slots))) return {false, false, 0};
    if (f.packing == 2) return {true, false, 0};
    return {true, true, f.row_statistic ? f.n_long_rows[lanes == 8 ? 0 : lanes == 16 ? 1 : 2] : f.B};  // no statistic (host-packed problem): not packed
}
inline bool packed_runs(const Facts &f, const Packed &p) { return p.shape && !(f.packing == 1 && 8 * p.n_long > f.B); }

// ---- the guarded step (guarded(f), neither dictionary nor packed form) ----
// Fast kernels with the guard evaluated per barcode, then the exact kernel over the barcodes they queued.  The coarse pass is admissible
// when nobody can read this E-step's logits (or dmx_set_coarse_pass(2)).  Which of coarse pass, fine pass and the direct form runs is the
// device's choice (k_guard_begin): both fast launches are issued, the one that is not taken stands back.
inline bool allow_coarse(const Facts &f) { return coarse_capable(f, f.lo) && (!f.logits_kept || f.coarse_pass == 2); }
// once per problem: the coarse pass's records - 8 bytes per call where the tile-major stream has 16 - and the log2 of the keep factors per barcode
inline bool coarse_build_due(const Facts &f) { return allow_coarse(f) && !f.coarse_ready; }
// dmx_set_lean_memory: the tile-major stream has done its last job behind that build, and the compact row array of the dictionary form
// goes with it (4 bytes per call): an E-step that keeps its logits on the prior table then runs the tolerance kernel too
inline bool lean_release_due(const Facts &f) { return coarse_build_due(f) && f.lean_memory; }
inline bool prob16_conversion_due(const Facts &f) { return allow_coarse(f) && !f.prob16_valid; }  // (else the P-step of the call has written it)
// a sliced run whose slices travel as lists of changed rows keeps the binary16 table up to date row by row from the conversion on
// (run_pstep): converted whatever level the device takes, so that the host knows it valid
inline bool prob16_stays_valid(const Facts &f) { return f.sliced && f.table_lists; }

// ---- what a launch walks: decided once, for the fine level of a guarded E-step and for an E-step without guard ----
// The tile-major stream while it is there.  Released (dmx_set_lean_memory): the tolerance kernels walk the coarse pass's records where they
// exist (k_estep_tiled_fine8: the float32 table, float64 sums), everything else a barcode per wavefront the barcode-major ones.
enum Walk { WALK_TILE_STREAM, WALK_COARSE_RECORDS, WALK_BARCODE_MAJOR };
inline Walk walk(const Facts &f)
{
    if (bins(f) <= 0) return WALK_BARCODE_MAJOR;
    if (f.tile_stream) return WALK_TILE_STREAM;
    return f.coarse_ready && singlet_tile_shape(f.K, f.with_doublets) && tolerance_arithmetic(f) ? WALK_COARSE_RECORDS : WALK_BARCODE_MAJOR;
}
inline float fine_allowance(const Facts &f, Walk w) { return w == WALK_COARSE_RECORDS ? guard_per_call_fine8(coarse_calls_per_gather(f.K)) : GUARD_PER_CALL_PLAIN; }

// ---- kernel choice: what one launch_estep is ----
enum KernelKind {
    KERNEL_REFUSED,          // no kernel for the request
    KERNEL_DIRECT,           // k_estep_direct<L, A, pairs, U, fast>: a barcode per L lanes, A options per lane
    KERNEL_DIRECT_SPLIT,     // ... over the segments of the split rows, then k_estep_join<A>
    KERNEL_TILED,            // k_estep_tiled<A, fast>
    KERNEL_TILED_TWO_CALLS,  // k_estep_tiled<1, true, true>: two calls per gather
    KERNEL_COARSE,           // k_estep_tiled_coarse<cpg>
    KERNEL_FINE8,            // k_estep_tiled_fine8<cpg>
    KERNEL_BLOCK_TILES,      // k_estep_block<tile, fast> per option tile, then k_softmax_rows
    KERNEL_PAIR_BLOCKS       // k_estep_pairblocks<.., threads> per `threads` blocks of the option triangle, then k_softmax_rows
};
struct Request {
    int K;
    bool pairs;
    bool fast;          // the tolerance arithmetic is wanted
    int schedule;       // Facts::schedule
    Walk walk;
    bool coarse;        // the launch is the coarse level's (the binary16 table, the coarse pass's records)
    bool segments;      // split rows are offered
    bool listed;        // the barcodes are a list whose length only the device knows (the redo of a guarded E-step)
    int n_pair_blocks;  // 0: none
};
// EstepArgs is the kernels' argument block and has no field for walk and level: run_estep hands them to launch_estep as the arrays
// themselves.  The two directions, side by side: handover() is what run_estep sets, request_of() what launch_estep reads back.
struct Handover {
    bool bins;            // the schedule's bins stay in the arguments (else n_bins = 0: a barcode per wavefront)
    bool coarse_records;  // the coarse pass's records are attached
    bool prob16;          // the binary16 table is attached: the coarse level
};
inline Handover handover(Walk w, bool coarse) { return {w != WALK_BARCODE_MAJOR, w == WALK_COARSE_RECORDS || coarse, coarse}; }
inline Request request_of(int K, bool pairs, bool fast, int schedule, long long n_bins, bool prob16, bool coarse_records, bool segments, bool listed, int n_pair_blocks)
{
    return {K, pairs, fast, schedule, n_bins <= 0 ? WALK_BARCODE_MAJOR : coarse_records ? WALK_COARSE_RECORDS : WALK_TILE_STREAM, prob16, segments, listed, n_pair_blocks};
}
struct Kernel {
    KernelKind kind;
    bool fast;     // the tolerance arithmetic (direct: wanted - launch_direct may still find the row shape missing)
    int L, A, U;   // direct: lanes per barcode, options per lane, calls in flight; tiled: A
    int cpg;       // coarse, fine8: calls per gather
    int tile;      // block tiles: options per thread
    int launches;  // block tiles, pair blocks: launches ahead of the softmax
    int threads;   // pair blocks: 256 or 512
};
inline Kernel kernel(const Request &r)
{
    const int K = r.K;
    Kernel k{KERNEL_REFUSED, r.fast, 0, 0, 0, 0, 0, 0, 0};
    // tile-major schedule (built by the repack for large singlet problems).  It pays in the tolerance mode, whose
    // time is the row gathers (1.50 ms against 1.72 ms on 200k x 100k x 64: L2 hit rate 44 % -> 68 %); the exact mode
    // is bound by its arithmetic and only pays the schedule's overhead (2.94 against 2.70 ms), so it keeps one
    // barcode per wavefront unless the schedule is forced (schedule == 2: tests; no exact tiled kernel below 33 genotypes).
    if (r.walk != WALK_BARCODE_MAJOR && singlet_tile_shape(K, r.pairs) && (r.fast || (r.schedule == 2 && K > 32))) {
        k.A = K <= 64 ? 1 : 2;
        k.cpg = coarse_calls_per_gather(K);
        if (r.fast && r.coarse) k.kind = KERNEL_COARSE;  // (its walk is its own records')
        else if (r.walk == WALK_COARSE_RECORDS) k.kind = r.fast ? KERNEL_FINE8 : KERNEL_REFUSED;  // (the exact kernels have no such walk: walk() never offers it)
        else k.kind = r.fast && K <= 32 ? KERNEL_TILED_TWO_CALLS : KERNEL_TILED;
        return k;
    }
    if (K <= 1024 && !block_shape(K, r.pairs, r.fast)) {  // register-resident up to 16 options per lane; slots past K are skipped wave-uniformly
        k.L = K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64;
        k.A = K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
        k.U = K <= 4 ? 4 : K <= 64 ? 8 : K <= 128 ? 4 : 2;
        k.kind = k.L == 64 && r.fast && r.segments && !r.listed ? KERNEL_DIRECT_SPLIT : KERNEL_DIRECT;
        return k;
    }
    if (!r.pairs) return k;  // K = G > 1024 singlets: not supported (ensure_options refuses them)
    // The options in tiles of up to 17 per thread, one launch per tile leaving its logits, then the softmax over complete rows.
    // What this form runs on is registers per thread, i.e. resident wavefronts:
    //   * the softmax fused into a single launch costs 40 VGPRs (3 waves per SIMD instead of 4): 12.2 ms against
    //     10.4 ms on 20k x 20k x 64 with doublets (K = 2080);
    //   * one launch with 33 accumulators per thread (236 VGPRs, 2 waves per SIMD) took 297 ms on 130k x 650k x 128 with
    //     doublets (K = 8256); two launches of 17 take 257 ms although every tile stages the barcode's genotype rows
    //     again; three of 12: 264 ms.
    // (Tiles of 65 accumulators per thread -- 385 VGPRs plus SGPR spills -- ended in GPU memory faults that narrower
    // tiles of the same source do not show: profiles/r2_block_tile65_experiment.txt.)
    if (r.fast && r.n_pair_blocks > 0 && !r.listed) {
        // tolerance arithmetic: 2 x 3 blocks of the option triangle.  512 threads share the staging of a chunk where there are blocks for
        // them (K = 8256: 1 450 blocks, 74.7 -> 69.7 ms; K = 528: 121 blocks, 1.24 ms with 256 threads against 1.84); 1024 threads: 103 ms
        k.kind = KERNEL_PAIR_BLOCKS;
        k.threads = r.n_pair_blocks >= 1024 ? 512 : 256;
        k.launches = (r.n_pair_blocks + k.threads - 1) / k.threads;
        return k;
    }
    const int need = (K + 255) / 256;
    k.tile = need <= 2 ? 2 : need <= 4 ? 4 : need <= 6 ? 6 : need <= 8 ? 8 : need <= 12 ? 12 : need <= 17 ? 17 : need <= 24 ? 12 : 17;
    // the tolerance mode carries a running product and an exponent per option besides the accumulator: tiles of 6
    // keep it at 4+ waves per SIMD (K = 8256: 170 ms with tiles of 17, 103 with 12, 87 with 6, 98 with 4; the exact
    // mode does not care: 214 / 220 / 218 / 230 ms)
    if (r.fast && need > 6) k.tile = 6;
    k.kind = KERNEL_BLOCK_TILES;
    k.launches = (K + k.tile * 256 - 1) / (k.tile * 256);
    return k;
}

}  // namespace eplan
}  // namespace dmx
