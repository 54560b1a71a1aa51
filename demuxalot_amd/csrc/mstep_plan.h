// mstep_plan.h -- the M-step's policy as pure functions of plain values: which form runs, whether it is incremental and of which kind,
// whether the tile records are to be built, where the sums go and what exchange follows.  Host only: nothing of HIP, nothing of dmx_ctx.
// dmx_steps.cpp: run_mstep fills Facts from the context, calls these in stages (the record build and plan_mstep_shifts may leave nothing:
// it refreshes the facts behind them) and acts on the answers; tests/mstep_plan_check.cpp walks the fact space on the CPU; the table: DESIGN.md 2.7.
#pragma once

#include <algorithm>

namespace dmx {
namespace mplan {

struct Facts {
    int mstep_tiles;            // dmx_set_mstep_tiles: 0 never, 1 when building the records pays, 2 always
    int mstep_incremental;      // dmx_set_mstep_incremental: 0 off, 1 on, 2 measurement (the sums built from nothing by the delta pass)
    bool exact_additions;       // dmx_set_exact_additions
    int G;                      // genotypes
    bool has_calls;             // n_csc > 0
    float power;                // the contribution power
    bool attached;              // some collective is attached (also with one rank)
    bool mshard;                // variant-sharded rank: its variant slice over the barcodes of all ranks
    bool sliced;                // reduce-scatter of the sums, sliced P-step
    bool reduce_f64;            // float64 wire
    bool has_call_pairs;        // which record arrays exist: d_call_pairs,
    bool has_item_variant;      // d_item_variant,
    bool has_shift_v;           // d_mt_shift_v,
    bool has_incr_state;        // d_incr_state,
    bool has_slice_rec;         // d_slice_rec (the slice's records by barcode row)
    long long n_mt;             // tile-major records held (0: not built / not eligible)
    bool mt_tried;              // a build was attempted
    long long msteps_done;      // the counters as they stand when the M-step begins: M-steps run on the resident problem,
    long long msteps_ahead;     // still to do in the running dmx_em / dmx_run_iterations call,
    long long msteps_expected;  // still to come as the caller announced (dmx_set_msteps_expected)
    bool incr_heavy;            // full passes keep coming on this problem (heavy_after_probe)
    long long rows_total;       // barcode rows of all ranks
    bool shift_tried;           // the tile cut for the exponents alone was attempted (plan_mstep_shifts; read by sums_on_grid only)
};

// The tile form's arithmetic - integer sums of rint(c 2^shift), in any order - is possible: not with the exact additions, which are the
// reference's float64 sum in the reference's order (power > 0: contributions in [0, 1])
inline bool fixed_point_possible(const Facts &f) { return !f.exact_additions && f.G <= 64 && f.has_calls && f.power > 0.0f; }

// One context with all calls of its barcodes and their barcode-major records.  A rank that exchanges SUMS - reduce-scatter of the partial
// sums of its own barcodes - is one too: its partial sums stay in the exchange buffer between two M-steps, the delta pass updates the rows
// it touched.  Not the all-reduce, which sums in place; not a variant-sharded rank, whose records are not its barcodes'.
inline bool own_records(const Facts &f) { return !f.mshard && (!f.attached || f.sliced) && f.has_call_pairs; }

// ... on which the work items can start the incremental M-step (shifts_wanted below)
inline bool items_can_start(const Facts &f) { return f.mstep_incremental && fixed_point_possible(f) && own_records(f) && f.has_item_variant; }
inline bool can_go_incremental(const Facts &f) { return f.mstep_tiles == 1 && items_can_start(f); }

// Building the records (a sort of the calls: 2.6 ms on 200k x 100k x 64, where an M-step + combine then takes 0.34 instead of
// 0.70 ms) pays from MSTEP_TILES_PAY M-steps on: taken when that many are still to come - in the running dmx_em /
// dmx_run_iterations call, or as the caller announced (dmx_set_msteps_expected) -, or the problem has seen that many
// already (somebody iterates call by call), or always (dmx_set_mstep_tiles(ctx, 2)).
// Under the INCREMENTAL M-step only the full passes cost anything, and since round 6 the work items can make them with the tile
// form's arithmetic (shifts_wanted below: 0.71 instead of 0.33 ms, no records): the records then pay only where full passes keep
// coming - a workload whose posteriors keep moving.  So a context that can go incremental starts on the work items and reads the
// device's count of full passes ONCE at its 4th, 16th and 64th M-step (a 4-byte download: the only host synchronisation of the
// policy); three full passes in the first four M-steps, or half of them later, and the records are built as before.  A converging
// 25-iteration call: M-steps 0.71 + 23 x 0.03 ms instead of 2.6 (build) + 0.33 + 23 x 0.03.
constexpr int MSTEP_TILES_PAY = 8;
inline bool probe_step(long long done) { return done == 4 || done == 16 || done == 64; }
inline bool probe_due(const Facts &f)
{
    return can_go_incremental(f) && !f.incr_heavy && f.n_mt == 0 && f.has_incr_state && probe_step(f.msteps_done);
}
inline bool heavy_after_probe(const Facts &f, unsigned full_passes)  // (the count the probe read)
{
    return f.msteps_done == 4 ? full_passes >= 3u : 2ull * full_passes >= (unsigned long long)f.msteps_done;
}
inline bool records_wanted(const Facts &f)  // (incr_heavy: as the probe left it)
{
    const bool long_run = std::max(f.msteps_ahead, f.msteps_expected) >= MSTEP_TILES_PAY || f.msteps_done >= MSTEP_TILES_PAY;
    const bool pays = f.n_mt > 0 || (long_run && (!can_go_incremental(f) || f.incr_heavy));
    return fixed_point_possible(f) && (f.mstep_tiles == 2 || (f.mstep_tiles == 1 && pays));
}
inline bool build_due(const Facts &f) { return records_wanted(f) && !f.mt_tried; }
// ---- behind the build (n_mt, has_shift_v as it left them) ----
inline bool tiles_ready(const Facts &f) { return records_wanted(f) && f.n_mt > 0; }

// Fixed-point WORK-ITEM form (kernels.h: MstepArgs::fixed_shift_v): where the tile-major records are not there - a call too short
// to pay for their sort, learn_genotypes' default of 5 iterations among them - the work items add the tile-major form's integers
// with the tile cut's exponents (plan_mstep_shifts: the host's cut, no sort), so that their sums are the tile-major form's bit for
// bit and the incremental M-step builds on them: one full pass of 0.7 ms, then delta passes, instead of 0.7 ms per M-step.
// (dmx_set_mstep_tiles(ctx, 0) or dmx_set_mstep_incremental(ctx, 0): the float64 work-item form, as before.)
inline bool shifts_wanted(const Facts &f) { return !tiles_ready(f) && f.mstep_tiles != 0 && items_can_start(f); }
// ---- behind plan_mstep_shifts (has_shift_v as it left it) ----
enum Incr { INCR_NONE, INCR_OWN_RECORDS, INCR_WORK_ITEMS, INCR_SHARDED };
struct Launch {
    int form;          // as dmx_get_mstep_form: 1 float64 work items (the exact additions' too), 2 tile-major, 3 fixed-point work items
    Incr incr;
    bool row_variant;  // the records' table rows are the exchange layout's padded rows (MIncrArgs::row_variant)
};
// Incremental form (kernels.h: MIncrArgs): one context with all calls of its barcodes, the tiles' per-variant exponents at hand.
// ... or a variant-sharded rank with the tile-major records of its slice (round 6; its sums go to d_add, nothing to exchange): the same
// sums over the barcodes of ALL ranks, the changed barcodes found in the gathered tables, the delta pass on the slice's records.
inline Launch launch(const Facts &f)
{
    const bool tiles = tiles_ready(f), items = shifts_wanted(f) && f.has_shift_v;
    const bool sharded = tiles && f.mstep_incremental == 1 && f.mshard && f.has_shift_v && f.has_item_variant && f.rows_total > 0;
    const bool own = (tiles || items) && f.mstep_incremental && own_records(f) && f.has_shift_v;
    const Incr incr = sharded ? INCR_SHARDED : !own ? INCR_NONE : items ? INCR_WORK_ITEMS : INCR_OWN_RECORDS;
    return {tiles ? 2 : incr == INCR_WORK_ITEMS ? 3 : 1, incr, own && f.sliced};
}
// AHEAD of the M-step - what the E-step before it asks (dmx_steps.cpp: run_estep, with the facts as that M-step will find them): will
// its sums be formed on the fixed-point grid (form 2 or 3)?  Then the codes and the bitmap may be written at the grid's live floor
// (kernels.h: live_floor_fixed).  Tiles ready, or their build due; or the work items' exponents wanted and at hand or still to be cut.
// Where neither a build nor a cut is pending the answer IS launch()'s: true <=> form 2 or 3 (tests/live_floor_check.cpp walks the fact
// space); a build or a cut that leaves nothing ends in form 1, and run_mstep rebuilds the codes once - the next E-step knows.
inline bool sums_on_grid(const Facts &f)
{
    return tiles_ready(f) || build_due(f) || (shifts_wanted(f) && (f.has_shift_v || !f.shift_tried));
}
// ... and only where the codes stay on this context: an attached one sends them to other ranks (k_post_compact_build,
// k_post_reconstruct), whose M-step forms are not this rank's to know.
inline bool live_floor_on_grid(const Facts &f) { return !f.attached && sums_on_grid(f); }
// what the codes' floor must not exceed for the form launch() chose: a float64 form (1) reads them for the reference's own sum
inline bool grid_floor_admitted(const Launch &l) { return l.form != 1; }

// a sharded rank's delta pass, behind the first-use build of its row index (build_slice_row_index): k_mincr_delta on the slice's records
// by barcode row - or, where the index does not apply, the masked walk of the variant-major records and its byte map
inline bool sharded_by_row_index(const Facts &f) { return f.has_slice_rec; }
// Where the sums go and what follows them.  One context, or a variant-sharded rank (its variant slice, summed over the barcodes of
// all ranks: final, exact, nothing to reduce): d_add.  Sliced: partial sums straight into the padded exchange buffer (row prow[v]),
// reduce-scatter, this rank's slice rounded into d_add.  Else - SNPs with scattered variants -: all-reduce of the dense sums in
// d_add / d_add64, P-step on every rank.
enum Exchange { EXCH_NONE, EXCH_REDUCE_SCATTER, EXCH_ALL_REDUCE };
struct Dest {
    bool exchange_buffer;  // d_exch with prow, else d_add
    bool f64;              // float64 sums: d_exch as doubles, d_add64
    Exchange then;
    bool slice_only;       // afterwards only this rank's slice of d_add is current (dmx_ctx::add_partial with several ranks)
};
inline Dest destination(const Facts &f)
{
    if (!f.attached || f.mshard) return {false, false, EXCH_NONE, f.attached};
    if (f.sliced) return {true, f.reduce_f64, EXCH_REDUCE_SCATTER, true};
    return {false, f.reduce_f64, EXCH_ALL_REDUCE, false};
}

// the variants whose records this context holds = the range of the record build and of the combine pass: the rank's cut, or all.
// (mshard on a context that is NOT attached - only after a dmx_comm_init that failed on a sharded problem, the old communicator
// already gone; no coherent state: its sums go to d_add unexchanged - combines over the cut its records were built for; run_mstep
// once built over the cut and combined over [0, V) there.)
struct Range {
    long long v0, v1;
};
inline Range variant_range(const Facts &f, const long long *cut, int rank, long long V)
{
    return f.mshard ? Range{cut[rank], cut[rank + 1]} : Range{0, V};
}

}  // namespace mplan
}  // namespace dmx
