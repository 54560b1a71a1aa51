// dmx_steps.cpp -- the step drivers behind dmx_probs_from_betas / dmx_estep / dmx_mstep / dmx_em / dmx_run_iterations: which form of
// which kernel runs (dictionary / packed / tiled / coarse / direct E-step under the guard; work-item / fixed-point / tile-major /
// incremental M-step), their device-side state, and the entry points themselves.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <array>
#include <chrono>
#include <functional>

#include <algorithm>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dmx_ctx.h"
#include "dmx_host.h"
#include "estep_plan.h"
#include "ambient_profile.h"
#include "ambient_grid_plan.h"
#include "ambient_learning_plan.h"
#include "ambient_scoring_plan.h"
#include "doublet_learning_plan.h"
#include "doublet_shares_learning_plan.h"
#include "estep_ambient.h"
#include "estep_ambient_grid.h"
#include "estep_pair_shares.h"
#include "estep_pools.h"
#include "mstep_ambient.h"
#include "mstep_doublet_shares.h"
#include "mstep_doublets.h"
#include "mstep_plan.h"
#include "mstep_soup.h"
#include "pair_shares_plan.h"
#include "pools_plan.h"
#include "soup_learning_plan.h"

using namespace dmx::host;

namespace dmx {
namespace host {

// Split rows of the tolerance / guarded E-step (kernels.h: EstepArgs::segs).  A wavefront walks its barcode's calls as a
// chain of memory latencies, so the longest row bounds a launch from below; rows with more CallPairs than half of what a
// wavefront slot of the chip gets on average (and at least 128) are cut into equal segments of whole 8-call groups.
// On the 200k-barcode bench workload nothing is cut (4 800 pairs per slot against rows of at most 2 000); on one rank's
// share of it on 8 GPUs (25k barcodes, 600 pairs per slot) the rows beyond 600 calls are.
int build_row_segments(dmx_ctx *c)
{
    c->n_segs = c->n_split = 0;
    const long long B = c->B;
    if (B == 0 || c->n_pairs == 0) return 0;
    if (!c->n_simd) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->n_simd = 4 * cus;
    }
    const long long slots = 8ll * std::max(1, c->n_simd);
    long long cap = std::max<long long>(128, c->n_pairs / (2 * slots));
    cap = (cap + 3) & ~3ll;
    std::vector<long long> pair_ptr((size_t)B + 1);
    std::vector<int> order((size_t)B);
    HIP_TRY(hipMemcpyAsync(pair_ptr.data(), c->d_pair_ptr.p, sizeof(long long) * (B + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(order.data(), c->d_bc_order.p, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<dmx::EstepSegment> segs;
    std::vector<int> first(1, 0);
    for (long long j = 0; j < B; j++) {  // `order` is sorted by decreasing length: the split rows are its first entries
        const int b = order[(size_t)j];
        const long long pairs = pair_ptr[(size_t)b + 1] - pair_ptr[(size_t)b];
        if (pairs <= cap) break;
        const long long pieces = (pairs + cap - 1) / cap;
        const long long groups = pairs / 4, per = (groups + pieces - 1) / pieces;  // whole 8-call groups per segment
        for (long long g0 = 0; g0 < groups; g0 += per)
            segs.push_back({b, (int)(4 * g0), (int)(4 * std::min(per, groups - g0)), 0});
        first.push_back((int)segs.size());
    }
    if (segs.empty()) return 0;
    // (the segments of one barcode stay adjacent and in order - split_first indexes them - and are of nearly equal length;
    // the barcodes come longest first, so the work list is roughly longest-first too)
    c->n_segs = (long long)segs.size();
    c->n_split = (long long)first.size() - 1;
    DMX_TRY(dev_alloc(c, c->d_segs, segs.size()));
    DMX_TRY(dev_alloc(c, c->d_split_first, first.size()));
    HIP_TRY(hipMemcpyAsync(c->d_segs.p, segs.data(), sizeof(dmx::EstepSegment) * segs.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_split_first.p, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // locals
    return 0;
}

int ensure_options(dmx_ctx *c, int with_doublets, const float *penalties)
{
    const int G = c->G;
    const long long K = with_doublets ? (long long)G * (G + 1) / 2 : G;
    if (K > (1 << 24)) return fail(DMX_ERR_UNSUPPORTED, "too many options (%lld)", K);
    if (G > 1024)  // one lane holds at most 16 genotype accumulators (E- and M-step); the block form stages G rows in LDS
        return fail(DMX_ERR_UNSUPPORTED, "more than 1024 genotypes are not supported (G=%d)", G);
    DMX_TRY(dev_grow(c, c->d_pen, (size_t)K));
    DMX_TRY(dev_grow(c, c->d_pairs, (size_t)K));
    DMX_TRY(dev_grow(c, c->d_logits, (size_t)(c->B * K)));
    DMX_TRY(dev_grow(c, c->d_post, (size_t)(c->B * K)));
    // option k -> (g1, g2): singlets (g, g) first, then g1 < g2 row-major (demux.py:175-191)
    std::vector<unsigned> pairs((size_t)K);
    for (int g = 0; g < G; g++) pairs[g] = (unsigned)g | ((unsigned)g << 16);
    if (with_doublets) {
        size_t k = G;
        for (int g1 = 0; g1 < G; g1++)
            for (int g2 = g1 + 1; g2 < G; g2++) pairs[k++] = (unsigned)g1 | ((unsigned)g2 << 16);
    }
    HIP_TRY(hipMemcpyAsync(c->d_pairs.p, pairs.data(), sizeof(unsigned) * K, hipMemcpyHostToDevice, c->stream));
    // 2 x 3 blocks of the (g1, g2) triangle for the tolerance mode's workgroup-per-barcode kernel (kernels.hip: k_estep_pairblocks)
    std::vector<unsigned> blocks;
    if (with_doublets && K > 256) {
        constexpr int R1 = dmx::PAIRBLOCK_R1, R2 = dmx::PAIRBLOCK_R2;
        for (int i = 0; R1 * i < G; i++)
            for (int j = 0; R2 * j < G; j++)
                if (R2 * j + R2 - 1 >= R1 * i) blocks.push_back((unsigned)i | ((unsigned)j << 16));  // some g2 of the block is >= its smallest g1
    }
    c->n_pair_blocks = (int)blocks.size();
    DMX_TRY(dev_grow(c, c->d_pair_blocks, blocks.size()));
    if (c->n_pair_blocks) HIP_TRY(hipMemcpyAsync(c->d_pair_blocks.p, blocks.data(), sizeof(unsigned) * blocks.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_pen.p, penalties, sizeof(float) * K, hipMemcpyHostToDevice, c->stream));
    DMX_TRY(dmx::ensure_sum_plan(c, K));
    DMX_TRY(dev_grow(c, c->d_seg_sums, (size_t)c->n_segs * (size_t)K));
    HIP_TRY(hipStreamSynchronize(c->stream));  // `pairs` is a local
    if ((int)K != c->K) c->float64_posteriors_dropped();  // (those of dmx_estep_snp)
    c->K = (int)K;
    return 0;
}

int upload_prior_logits(dmx_ctx *c, const void *prior, int dtype)
{
    if (!prior) return 0;
    if (dtype != DMX_F32 && dtype != DMX_F64) return fail(DMX_ERR_INVALID, "prior_dtype must be DMX_F32 or DMX_F64");
    const size_t bytes = (size_t)c->B * c->K * (dtype == DMX_F64 ? 8 : 4);
    if (bytes > c->d_prior_logits.n) {
        raw_free(c, c->d_prior_logits);
        DMX_TRY(raw_alloc(c, c->d_prior_logits, bytes));
    }
    HIP_TRY(hipMemcpyAsync(c->d_prior_logits.p, prior, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// [V, G] float32 table in the layout of d_prob <-> dense host table
int copy_prob_out(dmx_ctx *c, float *dst)
{
    if (!dst) return 0;
    const int G = c->G;
    if (!c->sliced) return copy_out(c, dst, c->d_prob.p, (size_t)c->V * G);
    for (int r = 0; r < c->nranks; r++) {
        const long long rows = c->cut[r + 1] - c->cut[r];
        if (rows) HIP_TRY(hipMemcpyAsync(dst + c->cut[r] * G, c->d_prob.p + (size_t)r * c->slice_rows * G, sizeof(float) * rows * G, hipMemcpyDeviceToHost, c->stream));
    }
    return 0;
}

int copy_prob_in(dmx_ctx *c, const float *src)
{
    const int G = c->G;
    c->sent_slice_forgotten();  // (the table is the caller's now)
    if (!c->sliced) {
        HIP_TRY(hipMemcpyAsync(c->d_prob.p, src, sizeof(float) * c->V * G, hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    for (int r = 0; r < c->nranks; r++) {
        const long long rows = c->cut[r + 1] - c->cut[r];
        if (rows) HIP_TRY(hipMemcpyAsync(c->d_prob.p + (size_t)r * c->slice_rows * G, src + c->cut[r] * G, sizeof(float) * rows * G, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// sliced mode: after an M-step only this rank's slice of d_add is current; assemble the whole table (collective:
// every rank must get here).  The gather has a buffer of its own: d_exch holds the partial sums the incremental M-step
// builds on, whatever host calls come between two M-steps.
int ensure_full_addition(dmx_ctx *c)
{
    if (!c->add_partial) return 0;
    const int G = c->G, n = c->nranks;
    float *stage = (float *)c->d_add_stage.p;
    const size_t block = (size_t)c->slice_rows * G;
    const long long mine = c->cut[c->rank + 1] - c->cut[c->rank];
    if (mine) HIP_TRY(hipMemcpyAsync(stage + c->rank * block, c->d_add.p + c->cut[c->rank] * G, sizeof(float) * mine * G, hipMemcpyDeviceToDevice, c->stream));
    DMX_TRY(coll_all_gather(c, stage, block, "addition"));
    for (int k = 0; k < n; k++) {
        const long long rows = c->cut[k + 1] - c->cut[k];
        if (rows && k != c->rank) HIP_TRY(hipMemcpyAsync(c->d_add.p + c->cut[k] * G, stage + k * block, sizeof(float) * rows * G, hipMemcpyDeviceToDevice, c->stream));
    }
    c->addition_gathered();
    return 0;
}

// the table as binary16 + the all-zero row the padding calls gather (EstepArgs::prob16)
int ensure_prob16(dmx_ctx *c)
{
    const size_t need16 = ((size_t)c->prob_rows + 1) * c->G * 2;
    if (need16 > c->d_prob16.n) {
        DMX_TRY(dev_grow(c, c->d_prob16, need16));
        c->half_table_reallocated();
        HIP_TRY(hipMemsetAsync(c->d_prob16.p, 0, need16 * sizeof(unsigned short), c->stream));
    }
    return 0;
}

// with_half: the E-step behind this P-step may take the coarse pass - the kernel writes the table as binary16 too (one rank, whole
// table; a sliced run converts behind the all-gather of the slices: run_estep)
int run_pstep(dmx_ctx *c, float lo, float hi, bool with_addition, bool with_half)
{
    // A sliced run converts the whole table behind the all-gather of the slices (run_estep) - unless the slices travel as lists of
    // changed rows: then this rank's slice is written as binary16 here, the others' changed rows where they are applied, and the table
    // that was valid before stays so.
    const bool half_rows = with_half && c->sliced && c->prob_list_words != 0 && c->prob_prev_valid && c->prob16_valid && c->d_prob16.p != nullptr;
    with_half = with_half && !c->sliced;
    if (with_half) DMX_TRY(ensure_prob16(c));
    c->pstep_begins();
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_PSTEP, &ev);
    const long long v0 = c->sliced ? c->cut[c->rank] : 0, v1 = c->sliced ? c->cut[c->rank + 1] : c->V;
    if (c->emulated && c->sliced && !c->emu_table_filled) {
        // emulated wire: nobody fills the other ranks' slices of genotype_prob; they hold the table without addition, so
        // that the E-step's rows are what an E-step sees (the posteriors decide which M-step kernel runs)
        for (int r = 0; r < c->nranks; r++)
            if (r != c->rank)
                HIP_TRY(dmx::launch_probs_from_betas(c->stream, c->d_prior.p, nullptr, c->d_v2snp.p, c->d_snp_ptr.p, c->d_snp_vars.p, c->cut[r],
                                                     c->cut[r + 1] - c->cut[r], -1LL, c->G, c->d_prow.p, lo, hi, c->d_prob.p));
        c->emulated_slices_filled();
    }
    HIP_TRY(dmx::launch_probs_from_betas(c->stream, c->d_prior.p, with_addition ? c->d_add.p : nullptr, c->d_v2snp.p,
                                         c->d_snp_ptr.p, c->d_snp_vars.p, v0, v1 - v0, c->sliced ? -1LL : (long long)c->S, c->G, c->d_prow.p, lo, hi,
                                         c->d_prob.p, (with_half || half_rows) ? c->d_prob16.p : nullptr));
    c->pstep_launched(with_half);
    timer_end(c, DMX_T_PSTEP, ev);
    if (c->sliced) {  // everybody gets everybody's slice of genotype_prob
        timer_begin(c, DMX_T_ALLREDUCE, &ev);
        const size_t block = (size_t)c->slice_rows * c->G;
        float *mine = c->d_prob.p + (size_t)c->rank * block;
        int rc = 0;
        bool whole = true;
        if (c->prob_list_words != 0 && c->prob_prev_valid) {
            // Compact form (kernels.hip: k_prob_changes_build): only the rows of this rank's slice that changed since it sent them; every
            // rank reads every rank's count behind the all-gather of the lists - one host synchronisation - and all take the whole
            // slices when a list overflowed.  The receivers' copies are what was sent last, so the table keeps its bits.
            // (the lists are sized from the last exchange's counts, as the posteriors' are: dmx_exchange.cpp, gather_posteriors)
            const unsigned cap_now = std::max(1u, std::min(c->prob_cap_now, c->prob_list_cap));
            const size_t words_now = 4 + (size_t)cap_now * (size_t)(1 + c->G);
            HIP_TRY(dmx::launch_prob_changes_build(c->stream, mine, c->d_prob_prev.p, c->slice_rows, c->G, cap_now,
                                                   c->d_prob_list.p + (size_t)c->rank * words_now,
                                                   c->emulated ? c->d_prob_list.p : nullptr, (unsigned long long)words_now, c->nranks, c->rank));
            rc = coll_all_gather(c, (float *)c->d_prob_list.p, words_now, "changed rows of genotype_prob");
            if (rc == 0) {
                // (the listed rows are written while the host polls for the counts: should a list have overflowed, the whole slices overwrite them)
                const unsigned seq = ++c->list_seq;
                HIP_TRY(dmx::launch_post_counts(c->stream, c->d_prob_list.p, (unsigned long long)words_now, c->nranks, c->h_prob_counts, seq));
                HIP_TRY(dmx::launch_prob_changes_apply(c->stream, c->d_prob.p, c->d_prob_list.p, (unsigned long long)words_now, c->slice_rows, c->G,
                                                       c->nranks, c->rank, cap_now, half_rows ? (unsigned short *)c->d_prob16.p : nullptr));
                DMX_TRY(wait_counts(c, c->h_prob_counts, c->nranks, seq));
                unsigned longest = 0;
                for (int r = 0; r < c->nranks; r++) longest = std::max(longest, c->h_prob_counts[r]);
                whole = longest > cap_now;
                if (std::getenv("DEMUXALOT_AMD_EXCHANGE_TRACE")) std::fprintf(stderr, "[table lists] longest %u capacity %u of %u\n", longest, cap_now, c->prob_list_cap);
                c->prob_cap_now = whole ? c->prob_list_cap : (unsigned)std::min<unsigned long long>(c->prob_list_cap, 4ull * longest + 512ull);
                if (!whole) {
                    c->prob_compact_taken++;
                    c->changed_rows_applied(half_rows);
                } else {
                    c->prob_compact_overflows++;
                }
            }
        } else if (c->prob_list_words != 0) {  // the first table of a layout (or behind a table somebody else wrote): what is sent now is what the others hold
            HIP_TRY(hipMemcpyAsync(c->d_prob_prev.p, mine, sizeof(float) * block, hipMemcpyDeviceToDevice, c->stream));
            c->sent_slice_recorded();
        }
        if (rc == 0 && whole) rc = coll_all_gather(c, c->d_prob.p, block, "genotype_prob");
        timer_end(c, DMX_T_ALLREDUCE, ev);
        if (rc) return rc;
    }
    c->table_written_by_pstep(lo, with_addition);
    return 0;
}

namespace ep = dmx::eplan;
static_assert(ep::MODE_EXACT == DMX_ESTEP_EXACT && ep::MODE_FAST == DMX_ESTEP_FAST && ep::MODE_GUARDED == DMX_ESTEP_GUARDED, "estep_plan.h: Mode");

// what the E-step's decisions read (estep_plan.h), as the context stands
static ep::Facts estep_facts(const dmx_ctx *c, int with_doublets, bool with_prior, bool logits_kept)
{
    ep::Facts f{};
    f.mode = (ep::Mode)c->estep_mode;
    f.with_doublets = with_doublets != 0;
    f.with_prior = with_prior;
    f.logits_kept = logits_kept;
    f.G = c->G;
    f.K = c->K;
    f.B = c->B;
    f.table_rows = c->prob_rows;
    f.schedule = c->tiled_estep;
    f.n_bins = c->n_bins;
    f.tile_stream = c->d_tile_stream.p != nullptr;
    f.coarse_ready = c->coarse_ready;
    f.coarse_pass = c->coarse_pass;
    f.guard_adaptive = c->guard_adaptive != 0;
    f.lean_memory = c->lean_memory != 0;
    f.lo = c->p_clip_lo;
    f.prob16_valid = c->prob16_valid;
    f.sliced = c->sliced;
    f.table_lists = c->prob_list_words != 0;
    f.dict_mode = c->dict_mode;
    f.dict_candidate = c->dict_candidate;
    f.call_rows = c->d_call_rows.p != nullptr;
    f.records_below_4g = ((unsigned long long)c->n_pairs + dmx::CALL_PAD_PAIRS) * sizeof(dmx::CallPair) < (1ull << 32);
    f.packing = c->estep_packing;
    f.row_statistic = c->max_row_calls > 0;
    for (int k = 0; k < 3; k++) f.n_long_rows[k] = c->n_long_rows[k];
    f.segments = c->n_segs > 0;
    f.n_pair_blocks = with_doublets && c->d_pair_blocks.p != nullptr ? c->n_pair_blocks : 0;
    return f;
}

// Dictionary form of the E-step (estep_dict.hip): distinct values per row of the current genotype table.  Returns
// the form to run in *form (DMX_FORM_DIRECT when some row does not fit or the form does not exist for the shape).
// The allocations, the build and its one download; estep_plan.h says before whether to build and behind which form the result allows.
int prepare_dictionary(dmx_ctx *c, bool pairs, dmx::EstepArgs &a, int *form)
{
    const ep::Facts f = estep_facts(c, pairs, false, true);  // (neither a prior nor who reads the logits matters to the dictionary)
    *form = DMX_FORM_DIRECT;
    a.dict_n = 0;
    c->dict_distinct = 0;
    if (!ep::dictionary_admissible(f)) return 0;
    const int G = c->G;
    const long long K = c->K, rows = c->prob_rows;
    const size_t code_pitch = (size_t)dmx::dict_code_pitch(G);
    DMX_TRY(dev_grow(c, c->d_dict, (size_t)rows * dmx::DICT_CAP));
    DMX_TRY(dev_grow(c, c->d_codes, (size_t)rows * code_pitch));
    if (!c->d_dict_stat.p) DMX_TRY(dev_alloc(c, c->d_dict_stat, (size_t)1));
    HIP_TRY(dmx::launch_build_dict(c->stream, c->d_prob.p, rows, G, c->d_dict.p, c->d_codes.p, c->d_dict_stat.p));
    unsigned distinct = 0;
    HIP_TRY(hipMemcpyAsync(&distinct, c->d_dict_stat.p, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->dict_distinct = (int)distinct;
    const size_t pitch = ep::dictionary_candidate_form(f, distinct) == ep::DICT_LANE ? (size_t)dmx::dict_table_pitch((int)distinct, (int)K, f.with_doublets) : 0;
    switch (ep::dictionary_form(f, distinct, pitch)) {
    case ep::DICT_NONE:
        return 0;
    case ep::DICT_BLOCK:
        a.dict_n = (int)distinct;
        a.dict = c->d_dict.p;
        a.codes = c->d_codes.p;
        *form = DMX_FORM_DICT_BLOCK;
        return 0;
    case ep::DICT_LANE:
        break;
    }
    const size_t need_bytes = (size_t)rows * pitch;
    DMX_TRY(dev_grow(c, c->d_dtab, need_bytes));
    HIP_TRY(dmx::launch_pack_rows(c->stream, c->d_dict.p, c->d_codes.p, c->d_pairs.p, rows, G, (int)K, f.with_doublets, (int)distinct, c->d_dtab.p));
    a.dict_n = (int)distinct;
    a.dtab = c->d_dtab.p;
    a.dtab_pitch = (int)pitch;
    a.dtab_bytes = (unsigned)need_bytes;
    *form = DMX_FORM_DICT;
    return 0;
}

// what the M-step's decisions read (mstep_plan.h), as the context stands: run_mstep's facts, and - asked ahead by run_estep, inside dmx_em /
// dmx_run_iterations with msteps_ahead already set for it - those of the M-step that follows an E-step (the counters move behind the plan)
static mplan::Facts mstep_facts(const dmx_ctx *c, float power)
{
    mplan::Facts f{};
    f.mstep_tiles = c->mstep_tiles;
    f.mstep_incremental = c->mstep_incremental;
    f.exact_additions = c->exact_additions;
    f.G = c->G;
    f.has_calls = c->n_csc > 0;
    f.power = power;
    f.attached = c->attached();  // also with one rank: keeps the collective path testable on one GPU
    f.mshard = c->mshard;
    f.sliced = c->sliced;
    f.reduce_f64 = c->reduce_dtype == DMX_F64;
    f.has_call_pairs = c->d_call_pairs.p != nullptr;
    f.has_item_variant = c->d_item_variant.p != nullptr;
    f.has_shift_v = c->d_mt_shift_v.p != nullptr;
    f.has_incr_state = c->d_incr_state.p != nullptr;
    f.has_slice_rec = c->d_slice_rec.p != nullptr;
    f.n_mt = c->n_mt;
    f.mt_tried = c->mt_tried;
    f.msteps_done = c->msteps_done;
    f.msteps_ahead = c->msteps_ahead;
    f.msteps_expected = c->msteps_expected;
    f.incr_heavy = c->incr_heavy;
    f.rows_total = c->rows_total;
    f.shift_tried = c->mt_shift_tried;
    return f;
}

// the argument block of the E-step's kernels as the context stands: no launch chosen yet (fast, segs, the guard's fields and what a
// launch walks are run_estep's to set from the plan)
static void fill_estep_args(dmx_ctx *c, dmx::EstepArgs &a, int with_doublets, bool with_prior, int prior_dtype, float power)
{
    a.pair_ptr = c->d_pair_ptr.p;
    a.order = c->d_bc_order.p;
    a.pairs = c->d_call_pairs.p;
    a.call_rows = c->d_call_rows.p;
    const unsigned long long rec_bytes = ((unsigned long long)c->n_pairs + dmx::CALL_PAD_PAIRS) * sizeof(dmx::CallPair);
    a.pairs_bytes = rec_bytes < (1ull << 32) ? (unsigned)rec_bytes : 0u;
    a.prob = c->d_prob.p;
    a.prob16 = nullptr;
    a.guard_accum = 0.0f;
    a.guard_alt_per_call = 0.0f;
    a.guard_alt_accum = 0.0f;
    a.guard_main_coarse = 0;
    a.opt_pairs = c->d_pairs.p;
    a.pair_blocks = with_doublets ? c->d_pair_blocks.p : nullptr;
    a.n_pair_blocks = with_doublets ? c->n_pair_blocks : 0;
    a.sum_plan = c->d_sum_plan.p;
    a.sum_plan_values = c->sum_plan_values;
    a.pen = c->d_pen.p;
    a.prior = with_prior ? c->d_prior_logits.p : nullptr;
    a.prior_dtype = prior_dtype;
    a.logits = c->d_logits.p;
    a.post = c->d_post.p;
    // variant-sharded M-step: the posteriors' codes / bitmaps / singlet columns go into this rank's block of the global tables
    const size_t row_base = c->mshard ? (size_t)c->rank * (size_t)c->rows_pad : 0;
    a.nz = c->mshard ? c->d_nz_g.p + row_base * ((c->G + 63) / 64) : c->d_nz.p;
    a.first = c->G <= 64 ? (c->mshard ? c->d_first_g.p + row_base : c->d_first.p) : nullptr;
    a.post_singlets = c->mshard ? c->d_post_g.p + row_base * c->G : nullptr;
    a.dense_calls = c->G <= 64 ? c->d_dense_calls.p : nullptr;
    // codes and bitmap at the floor the M-step that follows admits (kernels.h: live_floor_fixed); the regime statistic at its own
    a.dense_floor = dmx::live_floor_float64(power);
    a.nz_floor = c->live_floor_grid && mplan::live_floor_on_grid(mstep_facts(c, power)) ? dmx::live_floor_fixed(power) : a.dense_floor;
    a.B = c->B;
    a.prob_bytes = (unsigned)((unsigned long long)c->prob_rows * c->G * 4ull);
    a.G = c->G;
    a.K = c->K;
    a.fast = 0;
    a.guard = 0;
    a.guard_per_call = ep::GUARD_PER_CALL_PLAIN;  // estep_epilogue.h: GUARD_PER_CALL (launch_estep raises it for the form with pre-scaled rows)
    a.guard_count = c->d_guard_count.p;
    a.guard_list = c->d_guard_list.p;
    a.guard_sub = c->d_guard_sub.p;
    a.guard_sub_cap = c->guard_sub_cap;
    a.order_count = nullptr;
    a.direct = nullptr;
    a.order_direct = nullptr;
    a.segs = nullptr;
    a.n_segs = c->n_segs;
    a.n_split = c->n_split;
    a.split_first = c->d_split_first.p;
    a.seg_sums = c->d_seg_sums.p;
    a.tiled = c->tiled_estep;
    a.n_bins = 0;
    a.bin_rows_cap = c->bin_rows_cap;
    a.bin_order = c->d_bin_order.p;
    a.bin_rows = c->d_bin_rows.p;
    a.bin_ptr = c->d_bin_ptr.p;
    a.tile_stream = c->d_tile_stream.p;
    a.coarse_stream = nullptr;
    a.coarse_bin_ptr = nullptr;
    a.log2_keep = nullptr;
    a.n_long = 0;
    a.dict_n = 0;
    a.dtab = nullptr;
    a.dtab_bytes = 0;
    a.dtab_pitch = 0;
    a.dict = nullptr;
    a.codes = nullptr;
}

// what a launch walks and whether it is the coarse level's, handed to the kernels as the arrays themselves (estep_plan.h: handover;
// kernels.hip: launch_estep reads it back through request_of)
static void set_walk(const dmx_ctx *c, dmx::EstepArgs &a, ep::Walk walk, bool coarse = false)
{
    const ep::Handover h = ep::handover(walk, coarse);
    a.tile_stream = c->d_tile_stream.p;
    if (!h.bins) a.n_bins = 0;
    if (h.coarse_records) {
        a.coarse_stream = c->d_coarse_stream.p;
        a.coarse_bin_ptr = c->d_coarse_bin_ptr.p;
        a.log2_keep = c->d_log2_keep.p;
    }
    if (h.prob16) a.prob16 = c->d_prob16.p;
}

// The guarded step: fast kernels with the guard evaluated per barcode, then the exact kernel over the barcodes they queued (their
// number is only known on the device: a launch sized for all of them, the wavefronts past the queue's end
// return at once); the redo rewrites logits, posteriors, bitmaps and codes of those barcodes.  Adaptive
// (kernels.hip: k_guard_begin): the passes are timed on the device, and an E-step for which pass + redo would cost
// more than the exact kernel over every barcode runs that kernel directly - the fast kernels stand back.
// What is built, released and converted, and what the fine level walks: estep_plan.h, "the guarded step".
static int guarded_estep(dmx_ctx *c, ep::Facts &f, dmx::EstepArgs &a)
{
    const bool capable = ep::coarse_capable(f, f.lo), allow_coarse = ep::allow_coarse(f), release = ep::lean_release_due(f);
    // (the coarse guard's estimate of the fine level reads the fine level's allowance too: priced for the walk this E-step found, which is
    // not the one it leaves behind when the release comes with it)
    const float fine_allowance_found = ep::fine_allowance(f, ep::walk(f));
    if (ep::coarse_build_due(f)) {
        // ahead of k_guard_begin's time stamp (not part of the pass the device times)
        const int cpg = ep::coarse_calls_per_gather(f.K), bpr = ep::coarse_batches_per_record(cpg);
        const size_t words = (((size_t)c->n_pairs / 4 + (size_t)c->n_bins * (bpr - 1)) / bpr + 1) * (size_t)(cpg * 16);
        DMX_TRY(dev_alloc(c, c->d_coarse_stream, words));
        DMX_TRY(dev_alloc(c, c->d_coarse_bin_ptr, (size_t)c->n_bins + 1));
        DMX_TRY(dev_alloc(c, c->d_log2_keep, (size_t)c->B));
        // (the barcodes' sums of log2 keep come out of the same pass: every call's keep factor is read there once)
        HIP_TRY(dmx::launch_build_coarse_stream(c->stream, c->d_tile_stream.p, c->d_bin_ptr.p, c->n_bins, a.prob_bytes, cpg, c->d_coarse_bin_ptr.p, c->d_coarse_stream.p,
                                                c->d_bin_rows.p, c->bin_rows_cap, c->d_log2_keep.p));
        c->coarse_ready = f.coarse_ready = true;
        if (release) {  // (the blocks return to the context's cache behind the build, stream-ordered; the incremental M-step reads the rows from the records)
            dev_free(c, c->d_tile_stream);
            dev_free(c, c->d_call_rows);
            a.tile_stream = nullptr;
            a.call_rows = nullptr;
            f.tile_stream = f.call_rows = false;
        }
    }
    if (allow_coarse) DMX_TRY(ensure_prob16(c));
    HIP_TRY(dmx::launch_guard_begin(c->stream, c->d_guard_count.p, c->B, c->K, c->guard_adaptive, capable, allow_coarse));
    a.guard = 1;
    a.guard_per_call = fine_allowance_found;
    a.order_direct = c->d_bc_order.p;
    a.guard_main_coarse = 0;
    a.guard_alt_per_call = capable ? dmx::GUARD_PER_CALL_COARSE : 0.0f;
    a.guard_alt_accum = capable ? dmx::GUARD_ACCUM_F32 : 0.0f;
    if (allow_coarse) {
        if (ep::prob16_conversion_due(f)) {
            const bool kept = ep::prob16_stays_valid(f);
            HIP_TRY(dmx::launch_prob_to_half(c->stream, c->d_prob.p, c->prob_rows, c->G, c->d_prob16.p, kept ? nullptr : c->d_guard_count.p + dmx::GS_SKIP_COARSE));
            c->half_table_converted(kept);
        }
        dmx::EstepArgs coarse = a;
        set_walk(c, coarse, ep::WALK_COARSE_RECORDS, true);
        coarse.guard_per_call = dmx::GUARD_PER_CALL_COARSE;
        coarse.guard_accum = dmx::GUARD_ACCUM_F32;
        coarse.guard_main_coarse = 1;
        coarse.guard_alt_per_call = a.guard_per_call;
        coarse.guard_alt_accum = 0.0f;
        coarse.direct = c->d_guard_count.p + dmx::GS_SKIP_COARSE;
        HIP_TRY(dmx::launch_estep(c->stream, coarse, false));
    }
    a.direct = c->d_guard_count.p + dmx::GS_SKIP_FINE;
    const ep::Walk walk = ep::walk(f);  // (behind the release, where it came with this E-step)
    set_walk(c, a, walk);
    a.guard_per_call = ep::fine_allowance(f, walk);
    HIP_TRY(dmx::launch_estep(c->stream, a, f.with_doublets));
    a.coarse_stream = nullptr;  // (the redo below is the exact kernel's)
    HIP_TRY(dmx::launch_guard_compact(c->stream, c->d_guard_count.p, c->d_guard_sub.p, c->guard_sub_cap, c->d_guard_list.p, c->d_bc_order.p, c->B));
    dmx::EstepArgs redo = a;
    set_walk(c, redo, ep::WALK_BARCODE_MAJOR);
    redo.direct = c->d_guard_count.p + dmx::GS_DIRECT;
    redo.fast = 0;
    redo.guard = 2;
    redo.order = c->d_guard_list.p;
    redo.order_count = c->d_guard_count.p + dmx::GS_COUNT;
    HIP_TRY(dmx::launch_estep(c->stream, redo, f.with_doublets));
    c->guard_rows_total += c->B;
    c->guard_evaluated();
    return 0;
}

// logits_kept: somebody can read this E-step's logits (it is the last one of the call); else the next E-step of the same call
// overwrites them, and the guarded mode may take the coarse pass (kernels.hip: k_estep_tiled_coarse).
// Every decision is estep_plan.h's (the table: DESIGN.md 4.1); this is the sequence: arguments, facts, plan, builds and releases, launches, bookkeeping.
int run_estep(dmx_ctx *c, int with_doublets, bool with_prior, int prior_dtype, float power, bool logits_kept)
{
    dmx::EstepArgs a;
    fill_estep_args(c, a, with_doublets, with_prior, prior_dtype, power);
    // (the statistic's slots are zero: set at the install, left so by k_sum_dense at the end of every E-step that used them)
    c->estep_begins(a.dense_calls != nullptr, a.nz_floor);
    ep::Facts f = estep_facts(c, with_doublets, with_prior, logits_kept);
    if (ep::unused_stream_release_due(f)) {
        dev_free(c, c->d_tile_stream);
        a.tile_stream = nullptr;
        f.tile_stream = false;
    }
    a.fast = ep::tolerance_arithmetic(f);
    a.segs = ep::segments_offered(f) ? c->d_segs.p : nullptr;
    a.n_bins = ep::bins(f);
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);
    int form = DMX_FORM_DIRECT;
    if (!ep::coarse_first(f)) DMX_TRY(prepare_dictionary(c, f.with_doublets, a, &form));  // part of the E-step's time
    if (form == DMX_FORM_DICT)
        HIP_TRY(dmx::launch_estep_dict(c->stream, a, f.with_doublets));
    else if (form == DMX_FORM_DICT_BLOCK)
        HIP_TRY(dmx::launch_estep_dict_block(c->stream, a));
    else {
        ep::Packed packed = ep::packed_candidate(f);
#ifdef DMX_EXPERIMENTS  // experiment builds only (make EXPERIMENTS=1)
        if (const char *e = std::getenv("DEMUXALOT_AMD_PACKED_LONG"))
            if (packed.split) packed.n_long = std::min<long long>(c->B, std::max(0ll, atoll(e)));
#endif
        if (ep::packed_runs(f, packed)) {
            a.n_long = packed.n_long;
            a.fast = 0;
            HIP_TRY(dmx::launch_estep_packed(c->stream, a));
            form = DMX_FORM_PACKED;
        } else if (ep::guarded(f)) {
            DMX_TRY(guarded_estep(c, f, a));
        } else {
            set_walk(c, a, ep::walk(f));
            HIP_TRY(dmx::launch_estep(c->stream, a, f.with_doublets));
        }
    }
    c->estep_form = form;
    if (a.dense_calls) HIP_TRY(dmx::launch_sum_dense(c->stream, c->d_dense_calls.p, c->guard_ran ? c->d_guard_count.p : nullptr));
    else if (c->guard_ran) HIP_TRY(dmx::launch_guard_stamp(c->stream, c->d_guard_count.p, dmx::GS_T_END));
    timer_end(c, DMX_T_ESTEP, ev);
    c->estep_done(logits_kept);
    return 0;
}

// the incremental M-step's device state over incr_rows barcode rows: allocated at first use, reset when there is nothing to build on
static int ensure_incremental_state(dmx_ctx *c, bool sharded, long long incr_rows, float power)
{
    if (!c->d_acc64.p) {
        c->incr_rows = incr_rows;
        DMX_TRY(dev_alloc(c, c->d_acc64, (size_t)c->V * c->G));
        DMX_TRY(dev_alloc(c, c->d_prev_post, (size_t)incr_rows * c->G));
        DMX_TRY(dev_alloc(c, c->d_prev_first, (size_t)incr_rows));
        DMX_TRY(dev_alloc(c, c->d_incr_list, (size_t)incr_rows));
        if (sharded) {
            DMX_TRY(dmx::build_slice_row_index(c));  // (the slice's records by barcode row; without it: the masked walk and its byte map)
            if (c->d_slice_rec.p == nullptr) {
                DMX_TRY(dev_alloc(c, c->d_incr_map, (size_t)incr_rows));
                HIP_TRY(hipMemsetAsync(c->d_incr_map.p, 0, (size_t)incr_rows, c->stream));
            }
        }
        DMX_TRY(dev_alloc(c, c->d_incr_touched, (size_t)c->V));
        DMX_TRY(dev_alloc(c, c->d_incr_state, (size_t)(3 * dmx::IS_WORDS)));  // two alternating sets + the counters
        HIP_TRY(hipMemsetAsync(c->d_incr_state.p, 0, sizeof(unsigned) * 3 * dmx::IS_WORDS, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_incr_touched.p, 0, (size_t)c->V, c->stream));
        c->kept_sums_dropped();
    }
    if (!c->incr_valid || c->incr_power != power) {  // (nothing to build on: zeroed state words ask for the full pass)
        HIP_TRY(hipMemsetAsync(c->d_incr_state.p, 0, sizeof(unsigned) * 2 * dmx::IS_WORDS, c->stream));
        if (c->mstep_incremental == 2 && !c->attached()) {  // (measurement: the sums built from nothing by the delta pass instead of the full pass)
            const unsigned on[2] = {1u, 1u};
            HIP_TRY(hipMemsetAsync(c->d_acc64.p, 0, sizeof(unsigned long long) * (size_t)c->V * c->G, c->stream));
            HIP_TRY(hipMemsetAsync(c->d_prev_post.p, 0, sizeof(float) * (size_t)incr_rows * c->G, c->stream));
            HIP_TRY(hipMemsetAsync(c->d_prev_first.p, 0xFF, sizeof(uint2) * (size_t)incr_rows, c->stream));
            HIP_TRY(hipMemsetAsync(c->d_add.p, 0, sizeof(float) * (size_t)c->V * c->G, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_incr_state.p + dmx::IS_VALID, &on[0], sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_incr_state.p + dmx::IS_FORCE, &on[1], sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        c->incr_parity = 0;
        c->kept_sums_started(power);
    }
    return 0;
}

// Every decision is mstep_plan.h's (the table: DESIGN.md 2.7); this is the sequence: gather, probe, plan, build, state, arguments, launch, combine.
int run_mstep(dmx_ctx *c, float power)
{
    const bool mshard = c->mshard;
    const size_t row_base = mshard ? (size_t)c->rank * (size_t)c->rows_pad : 0;
    const int Wn = (c->G + 63) / 64;
    dmx::MstepArgs a;
    a.order = c->d_item_order.p;
    a.item_start = c->d_item_start.p;
    a.item_len = c->d_item_len.p;
    a.calls = c->d_csc.p;
    // variant-sharded: the barcodes of all ranks (global rows), singlet posteriors only (row stride G)
    a.post = mshard ? c->d_post_g.p : c->d_post.p;
    a.nz = mshard ? c->d_nz_g.p : c->d_nz.p;
    a.first = mshard ? c->d_first_g.p : c->d_first.p;
    const unsigned long long rows = mshard ? (unsigned long long)c->rows_total : (unsigned long long)c->B;
    a.K = mshard ? c->G : c->K;
    a.first_bytes = 8ull * rows;
    a.wide = c->mstep_wide;
    a.post_bytes = rows * (unsigned long long)a.K * 4ull;
    a.partial = c->d_partial.p;
    a.n_items = c->n_items;
    a.G = c->G;
    a.square = (power == 2.0f);
    a.power = power;
    a.dense_calls = c->dense_stat_valid && a.post_bytes < (1ull << 32) ? c->d_dense_calls.p : nullptr;
    a.total_calls = 2ull * (unsigned long long)c->n_pairs;
    // The codes and the bitmap are rebuilt from the stored posteriors when their floor is above what this M-step admits (the regime
    // statistic stays the E-step's: it has its own floor).  No launch in steady state: the E-step asked the plan ahead (run_estep).
    auto rebuild_codes = [&](float floor) -> int {
        HIP_TRY(dmx::launch_rebuild_nz(c->stream, c->d_post.p, c->B, c->K, c->G, floor, (mshard ? c->d_nz_g.p : c->d_nz.p) + row_base * Wn,
                                       c->G <= 64 ? (mshard ? c->d_first_g.p : c->d_first.p) + row_base : nullptr));
        c->codes_rebuilt(floor);
        return 0;
    };
    // before the codes travel: the E-step assumed a squaring M-step - the exact `!= 0` rule (whatever the form: live_floor_fixed is
    // live_floor_float64 for such a power)
    if (!a.square && c->nz_floor != 0.0f) DMX_TRY(rebuild_codes(0.0f));
    DMX_TRY(gather_posteriors(c));
    c->mstep_begins();
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    mplan::Facts f = mstep_facts(c, power);
    if (mplan::probe_due(f)) {
        unsigned full_passes = 0;
        HIP_TRY(hipMemcpyAsync(&full_passes, c->d_incr_state.p + 2 * dmx::IS_WORDS + 3, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        f.incr_heavy = c->incr_heavy = mplan::heavy_after_probe(f, full_passes);
    }
    if (c->msteps_expected > 0) c->msteps_expected--;  // (the plan reads the counters as they stood: f)
    c->msteps_done++;
    const mplan::Range own = mplan::variant_range(f, c->cut.data(), c->rank, c->V);
    if (mplan::build_due(f)) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (the build synchronises anyway; this makes its wall time its own)
        const auto t0 = std::chrono::steady_clock::now();
        DMX_TRY(dmx::build_mstep_tiles(c, own.v0, own.v1));
        c->mt_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        f.n_mt = c->n_mt;
    }
    if (mplan::shifts_wanted(f)) DMX_TRY(dmx::plan_mstep_shifts(c));
    f.has_shift_v = c->d_mt_shift_v.p != nullptr;
    const mplan::Launch plan = mplan::launch(f);
    const mplan::Dest dest = mplan::destination(f);
    // The form is known: a float64 form (1: the work items' float64 sums, the exact additions) reads the codes for the reference's own sum
    // and takes none written above its floor; the fixed-point forms take either (the dense regime's k_mstep_dense reads no codes at all).
    // Only a context that is not attached ever holds such codes (mplan::live_floor_on_grid), so nothing has travelled.
    if (!mplan::grid_floor_admitted(plan) && c->nz_floor > dmx::live_floor_float64(power)) DMX_TRY(rebuild_codes(dmx::live_floor_float64(power)));
    const bool incremental = plan.incr != mplan::INCR_NONE, sharded = plan.incr == mplan::INCR_SHARDED;
    const long long incr_rows = sharded ? c->rows_total : c->B;
    if (incremental) DMX_TRY(ensure_incremental_state(c, sharded, incr_rows, power));
    else c->kept_sums_dropped();  // (another form writes the addition)
    f.has_slice_rec = c->d_slice_rec.p != nullptr;
    const bool by_rows = sharded && mplan::sharded_by_row_index(f);
    // where k_mcombine writes: the variants of one work item are written there by the M-step kernels themselves
    a.item_variant = c->d_item_variant.p;
    a.item_ptr = c->d_item_ptr.p;
    a.prow = dest.exchange_buffer ? c->d_prow.p : nullptr;
    a.out32 = dest.f64 ? nullptr : dest.exchange_buffer ? (float *)c->d_exch.p : c->d_add.p;
    a.out64 = !dest.f64 ? nullptr : dest.exchange_buffer ? (double *)c->d_exch.p : c->d_add64.p;
    a.redo_cap = c->d_redo.n;
    a.tiles_done = plan.form == 2;
    a.incr_total = !sharded ? 0ull : by_rows ? (unsigned long long)c->n_csc : 2ull * (unsigned long long)incr_rows;
    dmx::MTileArgs tiles{};
    if (a.tiles_done) {
        tiles.stream = c->d_mt_stream.p;
        tiles.ptr = c->d_mt_ptr.p;
        tiles.first = c->d_mt_first.p;
        tiles.order = c->d_mt_order.p;
        tiles.shift = c->d_mt_shift.p;
        tiles.n_tiles = c->n_mt;
        tiles.tv = c->mt_tv;
    }
    dmx::MIncrArgs incr{};
    if (incremental) {
        incr.state = c->d_incr_state.p + c->incr_parity * dmx::IS_WORDS;
        incr.next = c->d_incr_state.p + (c->incr_parity ^ 1) * dmx::IS_WORDS;
        c->incr_parity ^= 1;
        incr.counters = c->d_incr_state.p + 2 * dmx::IS_WORDS;
        incr.acc64 = c->d_acc64.p;
        incr.prev = c->d_prev_post.p;
        incr.prev_first = c->d_prev_first.p;
        incr.list = c->d_incr_list.p;
        incr.touched = c->d_incr_touched.p;
        incr.shift_v = c->d_mt_shift_v.p;
        incr.pairs = sharded ? nullptr : c->d_call_pairs.p;
        incr.call_rows = sharded ? nullptr : c->d_call_rows.p;
        incr.pair_ptr = sharded ? nullptr : c->d_pair_ptr.p;
        incr.changed_map = sharded ? c->d_incr_map.p : nullptr;  // (null with the row index)
        incr.rec = sharded ? c->d_slice_rec.p : nullptr;
        incr.rec_ptr = by_rows ? c->d_slice_ptr.p : nullptr;
        incr.row_variant = plan.row_variant ? c->d_row_variant.p : nullptr;
        incr.B = incr_rows;
        incr.V = c->V;
        incr.floor = dmx::mincr_floor(power);
        tiles.acc64 = c->d_acc64.p;
        tiles.incr_state = incr.state;
        c->mstep_incr_launches++;
    }
    const bool fixed = plan.incr == mplan::INCR_WORK_ITEMS;  // (their full pass adds the tile form's integers: MstepArgs::fixed_shift_v)
    a.fixed_shift_v = fixed ? c->d_mt_shift_v.p : nullptr;
    a.fixed_acc64 = fixed ? c->d_acc64.p : nullptr;
    a.fixed_state = fixed ? incr.state : nullptr;
    timer_begin(c, DMX_T_MSTEP, &ev);
    HIP_TRY(incremental ? dmx::launch_mstep_incremental(c->stream, a, a.tiles_done ? &tiles : nullptr, incr)
            : a.tiles_done ? dmx::launch_mstep_tiles(c->stream, a, tiles) : dmx::launch_mstep(c->stream, a));
    c->mstep_form = plan.form;
    timer_end(c, DMX_T_MSTEP, ev);
    // combine into the plan's destination, then the exchange it names
    timer_begin(c, DMX_T_MCOMBINE, &ev);
    HIP_TRY(dmx::launch_mcombine(c->stream, a, c->d_item_ptr.p, own.v0, own.v1, a.prow, a.out32, a.out64, c->exact_additions ? c->d_redo.p : nullptr,
                                 c->d_n_redo.p, nullptr, true));
    timer_end(c, DMX_T_MCOMBINE, ev);
    int rc = 0;
    if (dest.then != mplan::EXCH_NONE) timer_begin(c, DMX_T_ALLREDUCE, &ev);
    if (dest.then == mplan::EXCH_REDUCE_SCATTER) {  // this rank's slice of the summed exchange buffer, rounded into d_add
        rc = coll_reduce_scatter(c, c->d_exch.p, c->d_recv.p, (size_t)c->slice_rows * c->G, dest.f64, c->stream);
        if (rc == 0)
            HIP_TRY(dmx::launch_store_slice(c->stream, c->d_recv.p, dest.f64, c->cut[c->rank], c->cut[c->rank + 1] - c->cut[c->rank], c->G, c->d_add.p));
    } else if (dest.then == mplan::EXCH_ALL_REDUCE) {
        rc = coll_all_reduce(c, dest.f64 ? (void *)c->d_add64.p : (void *)c->d_add.p, (size_t)c->V * c->G, dest.f64);
        if (rc == 0 && dest.f64) HIP_TRY(dmx::launch_f64_to_f32(c->stream, c->d_add64.p, c->d_add.p, (long long)c->V * c->G));
    }
    if (dest.then != mplan::EXCH_NONE) timer_end(c, DMX_T_ALLREDUCE, ev);
    if (rc == 0) c->addition_written_by_mstep(dest.slice_only, c->nranks);
    return rc;
}

}  // namespace host
}  // namespace dmx

extern "C" {

int dmx_set_addition(dmx_ctx *c, const float *addition)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem, "dmx_set_problem before dmx_set_addition"));
    const size_t vg = (size_t)c->V * c->G;
    c->kept_sums_dropped();  // (the addition is no longer the last M-step's: the incremental M-step starts over)
    if (addition) {
        HIP_TRY(hipMemcpyAsync(c->d_add.p, addition, sizeof(float) * vg, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        HIP_TRY(hipMemsetAsync(c->d_add.p, 0, sizeof(float) * (vg ? vg : 1), c->stream));
    }
    c->addition_set_by_caller(addition == nullptr);
    return 0;
}

int dmx_probs_from_betas(dmx_ctx *c, float lo, float hi, float *prob_out)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem && c->have_betas, "dmx_set_problem + dmx_set_betas before dmx_probs_from_betas"));
    DMX_TRY(run_pstep(c, lo, hi, true));
    DMX_TRY(copy_prob_out(c, prob_out));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_set_probs(dmx_ctx *c, const float *prob)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem, "dmx_set_problem before dmx_set_probs"));
    if (!prob && c->V > 0) return fail(DMX_ERR_INVALID, "null prob table");
    if (c->V) DMX_TRY(copy_prob_in(c, prob));
    // the E-step's log is the hot-path form (finite argument >= 1e-4): a table with entries outside [0, 1]
    // (or NaN) is refused rather than answered with numbers that mean nothing
    HIP_TRY(hipMemsetAsync(c->d_best.p, 0, sizeof(int), c->stream));
    HIP_TRY(dmx::launch_check_unit_range(c->stream, c->d_prob.p, c->prob_rows * c->G, c->d_best.p));
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, c->d_best.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flag) return fail(DMX_ERR_INVALID, "genotype_prob has entries outside [0, 1] (or NaN)");
    c->table_written_by_caller();
    return 0;
}

int dmx_probs_from_betas_f64(dmx_ctx *c, const double *betas, float lo, float hi, float *prob_out)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem, "dmx_set_problem before dmx_probs_from_betas_f64"));
    const size_t vg = (size_t)c->V * c->G;
    if (!betas && vg) return fail(DMX_ERR_INVALID, "null betas");
    double *d_b = nullptr;
    HIP_TRY(hipMalloc((void **)&d_b, (vg ? vg : 1) * sizeof(double)));
    hipError_t e = vg ? hipMemcpyAsync(d_b, betas, vg * sizeof(double), hipMemcpyHostToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess) {  // (a failed upload launches nothing, and its error is the one reported)
        c->sent_slice_forgotten();  // (every rank computes the whole table here)
        e = dmx::launch_probs_from_betas_f64(c->stream, d_b, c->d_v2snp.p, c->d_snp_ptr.p, c->d_snp_vars.p, c->V, c->S, c->G, c->d_prow.p, lo, hi, c->d_prob.p);
    }
    int rc_copy = 0;
    if (e == hipSuccess && vg) rc_copy = copy_prob_out(c, prob_out);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d_b);
    if (e != hipSuccess) return fail(DMX_ERR_HIP, "P-step from float64 betas: %s", hipGetErrorString(e));
    if (rc_copy) return rc_copy;
    c->table_written_from_f64_betas(lo);
    return 0;
}

int dmx_estep(dmx_ctx *c, int with_doublets, const float *penalties, const void *prior_logits, int prior_dtype,
              float *logits_out, float *probs_out)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem && c->have_probs, "genotype probabilities (dmx_probs_from_betas / dmx_set_probs) before dmx_estep"));
    if (!penalties) return fail(DMX_ERR_INVALID, "null penalties");
    DMX_TRY(ensure_options(c, with_doublets, penalties));
    DMX_TRY(upload_prior_logits(c, prior_logits, prior_dtype));
    DMX_TRY(run_estep(c, with_doublets, prior_logits != nullptr, prior_dtype, 2.0f));
    const size_t bk = (size_t)c->B * c->K;
    DMX_TRY(copy_out(c, logits_out, c->d_logits.p, bk));
    DMX_TRY(copy_out(c, probs_out, c->d_post.p, bk));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// What a plan header refuses (pools_plan.h, ambient_plan.h, ambient_scoring_plan.h, ambient_grid_plan.h), as the entry's error:
// "<who>: [<value> ]<text>[ (index <at>)]".
static int refuse(const char *who, int status, const char *what, long long at, long long value = -1)
{
    static_assert(dmx::pplan::OK == DMX_OK && dmx::pplan::INVALID == DMX_ERR_INVALID && dmx::pplan::UNSUPPORTED == DMX_ERR_UNSUPPORTED, "pools_plan.h restates the codes");
    char number[24] = "", index[40] = "";
    if (value >= 0) snprintf(number, sizeof number, "%lld ", value);
    if (at >= 0) snprintf(index, sizeof index, " (index %lld)", at);
    return fail(status, "%s: %s%s%s", who, number, what, index);
}

// the caller's result arrays of a pooled entry, in the order every entry of the family takes them (PoolsPlan says which are nullable)
struct PoolsOutputs {
    float *logits, *probs;
    int32_t *best_option;
    float *best_prob;
    double *doublet_mass;
};

// What every pooled entry does with the verdict of its plan header (pools_plan.h, ambient_scoring_plan.h, ambient_grid_plan.h,
// ambient_learning_plan.h): a refusal becomes the entry's error; what was accepted is laid out for the device half - the options,
// the caller's arrays and outputs.
static int accept_pools(const char *who, const dmx::pplan::Verdict &verdict, const dmx::pplan::Pools &pools, const PoolsOutputs &out,
                        dmx::PoolsPlan &plan)
{
    if (verdict.status != dmx::pplan::OK) return refuse(who, verdict.status, verdict.what, verdict.at, verdict.value);
    plan.with_doublets = pools.with_doublets != 0;
    plan.n_pools = pools.n_pools;
    dmx::pplan::layout(pools, plan.opt_ptr, plan.opts, plan.pool_size);
    plan.pair_penalty = pools.pair_penalty;
    plan.pool_of_barcode = pools.pool_of_barcode;
    plan.row_ptr = pools.row_ptr;
    plan.logits_out = out.logits;
    plan.probs_out = out.probs;
    plan.best_option = out.best_option;
    plan.best_prob = out.best_prob;
    plan.doublet_mass = out.doublet_mass;
    return 0;
}

// The pooled E-step (estep_pools.hip).  Everything is checked on the host (pools_plan.h) before anything is uploaded or launched: one
// function for dmx_estep_pools, dmx_estep_pools_resident and dmx_em_pools.  resident: the entry leaves the dense singlet posteriors in
// the context (single GPU, no communicator).
static int plan_pools(dmx_ctx *c, const char *who, bool resident, bool need_betas, const dmx::pplan::Pools &pools, const PoolsOutputs &out,
                      dmx::PoolsPlan &plan)
{
    if (need_betas) {
        if (!(c->have_problem && c->have_betas)) return fail(DMX_ERR_INVALID, "call order: dmx_set_problem + dmx_set_betas before %s", who);
    } else if (!(c->have_problem && c->have_probs)) {
        return fail(DMX_ERR_INVALID, "call order: genotype probabilities (dmx_probs_from_betas / dmx_set_probs) before %s", who);
    }
    if (c->nranks > 1) return fail(DMX_ERR_UNSUPPORTED, "%s: single GPU only", who);
    if (resident && c->attached()) return fail(DMX_ERR_UNSUPPORTED, "%s: a context with a communicator attached is not supported", who);
    return accept_pools(who, dmx::pplan::check(c->G, c->B, pools), pools, out, plan);
}

// what the plan headers of the entries under ambient fractions read of the context (ambient_plan.h: Facts).  have_table: what the
// entry computes from - the genotype probabilities, or for dmx_em_ambient, whose P-step forms them, the betas
static dmx::aplan::Facts ambient_facts(const dmx_ctx *c, bool have_table)
{
    return {c->have_problem, have_table, c->attached(), c->nranks, !c->sliced && c->prob_rows == c->V && c->d_prow.p == nullptr, c->B, c->V, c->G};
}

// what a dense pooled E-step writes into: the context's own result arrays with K = G, the [B, G] posteriors zeroed once - the kernel
// writes the columns of a barcode's pool only, and pool membership does not change inside a call
static int begin_dense_pools(dmx_ctx *c)
{
    const std::vector<float> zeros((size_t)std::max(c->G, 1), 0.0f);
    DMX_TRY(ensure_options(c, 0, zeros.data()));
    const size_t bg = (size_t)c->B * c->G;
    HIP_TRY(hipMemsetAsync(c->d_post.p, 0, sizeof(float) * (bg ? bg : 1), c->stream));
    c->posteriors_dropped();  // (until the first dense E-step has run)
    return 0;
}

int dmx_estep_pools(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                    const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out,
                    float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass)
{
    DMX_TRY(bind(c));
    dmx::PoolsPlan plan;
    DMX_TRY(plan_pools(c, "dmx_estep_pools", false, false, {with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr},
                       {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    return dmx::run_estep_pools(c, plan);
}

int dmx_estep_pools_resident(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                             const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out,
                             float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass)
{
    DMX_TRY(bind(c));
    dmx::PoolsPlan plan;
    DMX_TRY(plan_pools(c, "dmx_estep_pools_resident", true, false, {with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr},
                       {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    DMX_TRY(begin_dense_pools(c));
    dmx::PoolsRunPtr run;
    DMX_TRY(dmx::prepare_estep_pools(c, plan, true, run));
    DMX_TRY(dmx::launch_estep_pools_pass(c, *run, 2.0f));  // (the floor of a squaring M-step; run_mstep rebuilds for another power)
    return dmx::read_back_estep_pools(c, *run);
}

// Ambient RNA fractions (ambient_profile.hip).  Everything is checked on the host (ambient_plan.h) before anything is uploaded or
// launched; the resident results of the last E-step are not touched.
int dmx_ambient_profile(dmx_ctx *c, float lo, float hi, int32_t n_alphas, const float *alphas, const int32_t *donor1, const int32_t *donor2,
                        const float *ambient, float *loglik, int32_t *best, float *ll_best, float *ll_zero, float *ambient_out)
{
    namespace ap = dmx::aplan;
    static_assert(ap::OK == DMX_OK && ap::INVALID == DMX_ERR_INVALID && ap::UNSUPPORTED == DMX_ERR_UNSUPPORTED, "ambient_plan.h restates the codes");
    static_assert(sizeof(int) == sizeof(int32_t), "");
    DMX_TRY(bind(c));
    const ap::Verdict verdict = ap::check(ambient_facts(c, c->have_probs), n_alphas, alphas, (const int *)donor1, (const int *)donor2, ambient);
    if (verdict.status != ap::OK) return refuse("dmx_ambient_profile", verdict.status, verdict.what, verdict.at);
    const dmx::AmbientPlan plan{lo, hi, (int)n_alphas, alphas, donor1, donor2, ambient, loglik, best, ll_best, ll_zero, ambient_out};
    return dmx::run_ambient_profile(c, plan);
}

// The pooled E-step under per-barcode ambient fractions (estep_ambient.hip).  ambient_scoring_plan.h refuses, on the host, before
// anything is uploaded or launched - the pools among the rest, once; what it has accepted is laid out as for dmx_estep_pools.
int dmx_estep_ambient(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                      const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out, float *probs_out,
                      int32_t *best_option, float *best_prob, double *doublet_mass, float lo, float hi, const float *alpha, const float *ambient,
                      float *ambient_out)
{
    namespace sp = dmx::asplan;
    DMX_TRY(bind(c));
    const sp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_estep_ambient", sp::check(ambient_facts(c, c->have_probs), pools, alpha, ambient), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::AmbientScoring scoring{lo, hi, alpha, ambient, ambient_out};
    return dmx::run_estep_ambient(c, plan, scoring);
}

// The pooled E-step with every option at its own best fraction of a grid (estep_ambient_grid.hip).  ambient_grid_plan.h refuses, on
// the host, before anything is uploaded or launched; what it has accepted is laid out as for dmx_estep_pools.
int dmx_estep_ambient_grid(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                           const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out, float *probs_out,
                           int32_t *best_option, float *best_prob, double *doublet_mass, float lo, float hi, int32_t n_alphas, const float *alphas,
                           const float *ambient, float *ambient_out, int32_t *alpha_index, int32_t *best_alpha_index, float *profile_out)
{
    namespace gp = dmx::agplan;
    DMX_TRY(bind(c));
    const gp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_estep_ambient_grid", gp::check(ambient_facts(c, c->have_probs), pools, n_alphas, alphas, ambient), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::AmbientGridScoring scoring{lo, hi, (int)n_alphas, alphas, ambient, ambient_out, alpha_index, best_alpha_index, profile_out,
                                          false, nullptr, nullptr, nullptr};
    return dmx::run_estep_ambient_grid(c, plan, scoring);
}

// The same pass with every option's logit the log of the weighted sum over the grid (estep_ambient_grid.hip: the MARGINAL forms).
// ambient_grid_plan.h's check_marginal refuses, on the host, before anything is uploaded or launched.
int dmx_estep_ambient_grid_marginal(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                                    const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out,
                                    float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass, float lo, float hi,
                                    int32_t n_alphas, const float *alphas, const float *ambient, float *ambient_out, int32_t *alpha_index,
                                    int32_t *best_alpha_index, const float *log_weights, float *alpha_mean, float *best_alpha_mean)
{
    namespace gp = dmx::agplan;
    DMX_TRY(bind(c));
    const gp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_estep_ambient_grid_marginal",
                         gp::check_marginal(ambient_facts(c, c->have_probs), pools, n_alphas, alphas, ambient, log_weights), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::AmbientGridScoring scoring{lo, hi, (int)n_alphas, alphas, ambient, ambient_out, alpha_index, best_alpha_index, nullptr,
                                          true, log_weights, alpha_mean, best_alpha_mean};
    return dmx::run_estep_ambient_grid(c, plan, scoring);
}

// The pooled E-step with every pair option summed over a grid of mixing shares (estep_pair_shares.hip).  pair_shares_plan.h refuses,
// on the host, before anything is uploaded or launched; what it has accepted is laid out as for dmx_estep_pools.
int dmx_estep_pair_shares(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                          const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out, float *probs_out,
                          int32_t *best_option, float *best_prob, double *doublet_mass, int32_t n_shares, const float *shares,
                          const float *log_weights, int32_t *share_index, float *share_mean, int32_t *best_share_index, float *best_share_mean)
{
    namespace ps = dmx::psplan;
    DMX_TRY(bind(c));
    const ps::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_estep_pair_shares", ps::check(ambient_facts(c, c->have_probs), pools, n_shares, shares, log_weights), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::PairSharesScoring scoring{(int)n_shares, shares, log_weights, share_index, share_mean, best_share_index, best_share_mean};
    return dmx::run_estep_pair_shares(c, plan, scoring);
}

int dmx_mstep(dmx_ctx *c, float power, float *addition_out)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem && c->have_post, "dmx_estep before dmx_mstep"));
    DMX_TRY(run_mstep(c, power));
    if (addition_out) DMX_TRY(ensure_full_addition(c));  // collective when sliced: all ranks pass it, or none does
    DMX_TRY(copy_out(c, addition_out, c->d_add.p, (size_t)c->V * c->G));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// demux.py:86: an EM call starts from a zero addition, which no kept state of an earlier M-step describes
static int begin_em_additions(dmx_ctx *c)
{
    const size_t vg = (size_t)c->V * c->G;
    HIP_TRY(hipMemsetAsync(c->d_add.p, 0, sizeof(float) * (vg ? vg : 1), c->stream));
    c->addition_zeroed();
    return 0;
}

int dmx_em(dmx_ctx *c, int n_iterations, float lo, float hi, int with_doublets, const float *penalties,
           const void *prior_logits, int prior_dtype, float power, float *logits_out, float *probs_out,
           float *addition_out)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem && c->have_betas, "dmx_set_problem + dmx_set_betas before dmx_em"));
    if (n_iterations < 1) return fail(DMX_ERR_INVALID, "n_iterations must be >= 1");
    if (!penalties) return fail(DMX_ERR_INVALID, "null penalties");
    DMX_TRY(ensure_options(c, with_doublets, penalties));
    DMX_TRY(upload_prior_logits(c, prior_logits, prior_dtype));
    DMX_TRY(begin_em_additions(c));
    const bool keep_last = c->logits_needed || logits_out != nullptr;  // (dmx_set_logits_needed)
    for (int it = 0; it < n_iterations; it++) {
        const bool kept = it + 1 == n_iterations && keep_last;  // somebody can read this E-step's logits
        DMX_TRY(run_pstep(c, lo, hi, true, !kept && it > 0 && ep::coarse_capable(estep_facts(c, with_doublets, false, kept), lo)));  // (iteration 0: the dictionary form)
        // (the E-step asks the plan of the M-step behind it for the codes' floor: msteps_ahead as that M-step will find it - 0 behind the
        // last E-step, whose M-step, if any, is a later call's)
        c->msteps_ahead = n_iterations - 1 - it;
        const int rc_e = run_estep(c, with_doublets, it == 0 && prior_logits != nullptr, prior_dtype, power, kept);
        const int rc_m = rc_e == 0 && it + 1 < n_iterations ? run_mstep(c, power) : rc_e;  // the M-step after the last yield is dead
        c->msteps_ahead = 0;
        if (rc_m) return rc_m;
    }
    const size_t bk = (size_t)c->B * c->K;
    DMX_TRY(copy_out(c, logits_out, c->d_logits.p, bk));
    DMX_TRY(copy_out(c, probs_out, c->d_post.p, bk));
    DMX_TRY(ensure_full_addition(c));  // (collective when sliced) the slices of the last M-step, on every rank
    DMX_TRY(copy_out(c, addition_out, c->d_add.p, (size_t)c->V * c->G));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The loop of an EM call whose E-step is a dense pooled pass (dmx_em_pools, dmx_em_ambient): P-step, estep_pass(), and between two
// iterations mstep(M-steps the call still has to do, this one included) - the M-step after the last yield is dead; then the addition
// the last E-step used goes to the caller.  The caller has begun the dense pass and the additions and prepared its run.
static int run_dense_em(dmx_ctx *c, int n_iterations, float lo, float hi, float *addition_out, const std::function<int()> &estep_pass,
                        const std::function<int(int)> &mstep)
{
    for (int it = 0; it < n_iterations; it++) {
        DMX_TRY(run_pstep(c, lo, hi, true, false));
        DMX_TRY(estep_pass());
        if (it + 1 < n_iterations) DMX_TRY(mstep(n_iterations - 1 - it));
    }
    return copy_out(c, addition_out, c->d_add.p, (size_t)c->V * c->G);
}

// dmx_em with the pooled E-step in place of the full-table one: P-step, dense pooled E-step, M-step, all on the device; the host
// round trip of the pools (lists, uploads, result buffers) is paid once, the read-back once after the last E-step.
int dmx_em_pools(dmx_ctx *c, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                 const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float power,
                 float *logits_out, float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass, float *addition_out)
{
    DMX_TRY(bind(c));
    dmx::PoolsPlan plan;
    DMX_TRY(plan_pools(c, "dmx_em_pools", true, true, {with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr},
                       {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    if (n_iterations < 1) return fail(DMX_ERR_INVALID, "dmx_em_pools: n_iterations must be >= 1");
    DMX_TRY(begin_dense_pools(c));
    DMX_TRY(begin_em_additions(c));
    dmx::PoolsRunPtr run;
    DMX_TRY(dmx::prepare_estep_pools(c, plan, true, run));
    DMX_TRY(run_dense_em(
        c, n_iterations, lo, hi, addition_out, [&] { return dmx::launch_estep_pools_pass(c, *run, power); },
        [&](int msteps_ahead) {  // run_mstep's plan (mstep_plan.h) weighs the M-steps still to come when it chooses a form that pays back
            c->msteps_ahead = msteps_ahead;
            const int rc_m = run_mstep(c, power);
            c->msteps_ahead = 0;
            return rc_m;
        }));
    return dmx::read_back_estep_pools(c, *run);
}

// Learning under per-barcode ambient fractions (estep_ambient.hip: the dense form; mstep_ambient.hip).  ambient_scoring_plan.h and
// ambient_learning_plan.h refuse, on the host, before anything is uploaded or launched.
int dmx_estep_ambient_resident(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                               const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out,
                               float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass, float lo, float hi,
                               const float *alpha, const float *ambient, float *ambient_out)
{
    namespace sp = dmx::asplan;
    DMX_TRY(bind(c));
    const sp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_estep_ambient_resident", sp::check(ambient_facts(c, c->have_probs), pools, alpha, ambient), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::AmbientScoring scoring{lo, hi, alpha, ambient, ambient_out, "dmx_estep_ambient_resident"};
    DMX_TRY(begin_dense_pools(c));
    dmx::AmbientRunPtr run;
    DMX_TRY(dmx::prepare_estep_ambient(c, plan, scoring, true, run));
    DMX_TRY(dmx::launch_estep_ambient_pass(c, *run, 2.0f));  // (the floor of a squaring M-step; the M-steps rebuild for another power)
    return dmx::read_back_estep_ambient(c, *run);
}

int dmx_mstep_ambient(dmx_ctx *c, float power, const float *alpha, const float *ambient, float lo, float hi, float *addition_out)
{
    namespace lp = dmx::alplan;
    DMX_TRY(bind(c));
    const lp::Verdict verdict = lp::check_mstep(ambient_facts(c, c->have_probs), c->have_post, power, alpha, ambient);
    if (verdict.status != lp::OK) return refuse("dmx_mstep_ambient", verdict.status, verdict.what, verdict.at, verdict.value);
    DMX_TRY(dmx::run_mstep_ambient_from_host(c, power, alpha, ambient, lo, hi));
    DMX_TRY(copy_out(c, addition_out, c->d_add.p, (size_t)c->V * c->G));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// dmx_em_pools with the E-step and the M-step under the fractions: P-step, dense ambient E-step, ambient M-step, all on the device; the
// round trip of the pools, the uploads, the profile and the soup's terms are paid once, the read-back once after the last E-step.
int dmx_em_ambient(dmx_ctx *c, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                   const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float power,
                   const float *alpha, const float *ambient, float *logits_out, float *probs_out, int32_t *best_option, float *best_prob,
                   double *doublet_mass, float *addition_out, float *ambient_out)
{
    namespace lp = dmx::alplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_em_ambient", lp::check_em(ambient_facts(c, c->have_betas), pools, n_iterations, power, alpha, ambient), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::AmbientScoring scoring{lo, hi, alpha, ambient, ambient_out, "dmx_em_ambient"};
    DMX_TRY(begin_dense_pools(c));
    DMX_TRY(begin_em_additions(c));
    dmx::AmbientRunPtr run;
    DMX_TRY(dmx::prepare_estep_ambient(c, plan, scoring, true, run));
    // msteps_ahead is not set around this M-step: run_mstep_ambient (mstep_ambient.hip) has one form, the float64 sums, asks no plan of
    // mstep_plan.h and never consults it
    DMX_TRY(run_dense_em(
        c, n_iterations, lo, hi, addition_out, [&] { return dmx::launch_estep_ambient_pass(c, *run, power); },
        [&](int) { return dmx::run_mstep_ambient(c, power, dmx::ambient_run_alpha(*run), dmx::ambient_run_soup(*run)); }));
    return dmx::read_back_estep_ambient(c, *run);
}

// Learning the soup's profile (mstep_soup.hip).  soup_learning_plan.h refuses, on the host, before anything is uploaded
// or launched.  The step writes its counts to scratch: the context's addition, posteriors and table stay as they are.
int dmx_mstep_soup(dmx_ctx *c, const float *alpha, const float *ambient, float pseudo_count, float lo, float hi, float *ambient_out,
                   float *counts_out)
{
    namespace lp = dmx::slplan;
    DMX_TRY(bind(c));
    const lp::Verdict verdict = lp::check_mstep(ambient_facts(c, c->have_probs), c->have_post, pseudo_count, alpha, ambient);
    if (verdict.status != lp::OK) return refuse("dmx_mstep_soup", verdict.status, verdict.what, verdict.at, verdict.value);
    return dmx::run_mstep_soup_from_host(c, alpha, ambient, pseudo_count, lo, hi, ambient_out, counts_out);
}

// dmx_em_ambient with the profile learnt: behind every E-step but the last the soup M-step and the ambient M-step, both with the
// profile that E-step read; the new profile takes the run's place for the next E-step, whose pass rebuilds the soup's terms.  The
// dense pass closes at the lower of the two M-steps' live floors - the soup step's 0 -, so no codes are rebuilt between the two.
int dmx_em_ambient_soup(dmx_ctx *c, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                        const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr,
                        float power, const float *alpha, const float *ambient, float pseudo_count, float *logits_out, float *probs_out,
                        int32_t *best_option, float *best_prob, double *doublet_mass, float *addition_out, float *ambient_out,
                        float *counts_out)
{
    namespace lp = dmx::slplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_em_ambient_soup",
                         lp::check_em(ambient_facts(c, c->have_betas), pools, n_iterations, power, pseudo_count, alpha, ambient), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::AmbientScoring scoring{lo, hi, alpha, ambient, ambient_out, "dmx_em_ambient_soup"};
    DMX_TRY(begin_dense_pools(c));
    DMX_TRY(begin_em_additions(c));
    dmx::AmbientRunPtr run;
    DMX_TRY(dmx::prepare_estep_ambient(c, plan, scoring, true, run));
    dmx::SoupRunPtr soup;
    DMX_TRY(dmx::prepare_soup_run(c, pseudo_count, lo, hi, soup));
    DMX_TRY(run_dense_em(
        c, n_iterations, lo, hi, addition_out, [&] { return dmx::launch_estep_ambient_pass(c, *run, lp::POWER); },
        [&](int) {
            DMX_TRY(dmx::run_mstep_soup(c, *soup, dmx::ambient_run_alpha(*run), dmx::ambient_run_soup(*run)));
            DMX_TRY(dmx::run_mstep_ambient(c, power, dmx::ambient_run_alpha(*run), dmx::ambient_run_soup(*run)));
            return dmx::ambient_run_replace_soup(c, *run, dmx::soup_run_profile(*soup));
        }));
    DMX_TRY(dmx::read_back_soup_counts(c, *soup, counts_out));
    return dmx::read_back_estep_ambient(c, *run);
}

// Learning from doublet posteriors (mstep_doublets.hip).  doublet_learning_plan.h refuses, on the host, before anything
// is uploaded or launched.  dmx_em_pools' loop with the live-pair list and the crediting M-step between two iterations; the round trip
// of the pools and the list's buffers are paid once, the read-back once after the last E-step.
int dmx_em_doublets(dmx_ctx *c, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                    const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float power,
                    float min_pair_posterior, float *logits_out, float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass,
                    float *addition_out)
{
    namespace lp = dmx::dlplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_em_doublets", lp::check_em(ambient_facts(c, c->have_betas), pools, n_iterations, power, min_pair_posterior), pools,
                         {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    DMX_TRY(begin_dense_pools(c));
    DMX_TRY(begin_em_additions(c));
    dmx::PoolsRunPtr run;
    DMX_TRY(dmx::prepare_estep_pools(c, plan, true, run));
    dmx::DoubletRunPtr credited;
    DMX_TRY(dmx::prepare_doublet_run(c, *run, lp::pair_options(c->B, pools), credited));
    // (msteps_ahead is not set around this M-step: run_mstep_doublets has one form, the float64 sums, and asks no plan of mstep_plan.h)
    DMX_TRY(run_dense_em(
        c, n_iterations, lo, hi, addition_out, [&] { return dmx::launch_estep_pools_pass(c, *run, power); },
        [&](int) { return dmx::run_mstep_doublets(c, power, min_pair_posterior, *credited); }));
    return dmx::read_back_estep_pools(c, *run);
}

int dmx_mstep_doublets(dmx_ctx *c, float power, float min_pair_posterior, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                       const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr,
                       const float *post_rows, int64_t n_rows, float *addition_out)
{
    namespace lp = dmx::dlplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_mstep_doublets",
                         lp::check_mstep(ambient_facts(c, c->have_probs), c->have_post, pools, power, min_pair_posterior, n_rows, post_rows), pools,
                         {nullptr, nullptr, nullptr, nullptr, nullptr}, plan));
    DMX_TRY(dmx::run_mstep_doublets_from_host(c, power, min_pair_posterior, plan, post_rows, lp::pair_options(c->B, pools)));
    DMX_TRY(copy_out(c, addition_out, c->d_add.p, (size_t)c->V * c->G));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Learning from doublets of unequal shares (estep_pair_shares.hip: the dense form; mstep_doublet_shares.hip).
// doublet_shares_learning_plan.h refuses, on the host, before anything is uploaded or launched.  dmx_em_doublets' loop with the
// grid-summed dense E-step and the share-weighted crediting M-step; share_mean stays on the device between the two.
int dmx_em_doublet_shares(dmx_ctx *c, int n_iterations, float lo, float hi, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                          const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr,
                          float power, float min_pair_posterior, int32_t n_shares, const float *shares, const float *log_weights,
                          float *logits_out, float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass, float *addition_out,
                          int32_t *share_index, float *share_mean, int32_t *best_share_index, float *best_share_mean)
{
    namespace lp = dmx::dslplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_em_doublet_shares",
                         lp::check_em(ambient_facts(c, c->have_betas), pools, n_shares, shares, log_weights, n_iterations, power, min_pair_posterior),
                         pools, {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::PairSharesScoring scoring{(int)n_shares, shares, log_weights, share_index, share_mean, best_share_index, best_share_mean};
    DMX_TRY(begin_dense_pools(c));
    DMX_TRY(begin_em_additions(c));
    dmx::PairSharesRunPtr run;
    DMX_TRY(dmx::prepare_pair_shares_run(c, plan, scoring, run));
    dmx::DoubletSharesRunPtr credited;
    DMX_TRY(dmx::prepare_doublet_shares_run(c, *run, lp::pair_options(c->B, pools), credited));
    // (msteps_ahead is not set around this M-step: run_mstep_doublet_shares has one form, the float64 sums, and asks no plan of mstep_plan.h)
    DMX_TRY(run_dense_em(
        c, n_iterations, lo, hi, addition_out, [&] { return dmx::launch_pair_shares_pass(c, *run, power); },
        [&](int) { return dmx::run_mstep_doublet_shares(c, power, min_pair_posterior, *credited); }));
    return dmx::read_back_pair_shares(c, *run);
}

int dmx_estep_pair_shares_resident(dmx_ctx *c, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                                   const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr, float *logits_out,
                                   float *probs_out, int32_t *best_option, float *best_prob, double *doublet_mass, int32_t n_shares,
                                   const float *shares, const float *log_weights, int32_t *share_index, float *share_mean,
                                   int32_t *best_share_index, float *best_share_mean)
{
    namespace lp = dmx::dslplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_estep_pair_shares_resident", lp::check_estep(ambient_facts(c, c->have_probs), pools, n_shares, shares, log_weights),
                         pools, {logits_out, probs_out, best_option, best_prob, doublet_mass}, plan));
    const dmx::PairSharesScoring scoring{(int)n_shares, shares, log_weights, share_index, share_mean, best_share_index, best_share_mean};
    DMX_TRY(begin_dense_pools(c));
    dmx::PairSharesRunPtr run;
    DMX_TRY(dmx::prepare_pair_shares_run(c, plan, scoring, run));
    DMX_TRY(dmx::launch_pair_shares_pass(c, *run, 2.0f));  // (the floor of a squaring M-step; the M-steps rebuild for another power)
    return dmx::read_back_pair_shares(c, *run);
}

int dmx_mstep_doublet_shares(dmx_ctx *c, float power, float min_pair_posterior, int with_doublets, int32_t n_pools, const int64_t *pool_start,
                             const int32_t *pool_donors, const float *pair_penalty, const int32_t *pool_of_barcode, const int64_t *row_ptr,
                             const float *post_rows, const float *share_rows, int64_t n_rows, float *addition_out)
{
    namespace lp = dmx::dslplan;
    DMX_TRY(bind(c));
    const lp::Pools pools{with_doublets, n_pools, pool_start, pool_donors, pair_penalty, pool_of_barcode, row_ptr};
    dmx::PoolsPlan plan;
    DMX_TRY(accept_pools("dmx_mstep_doublet_shares",
                         lp::check_mstep(ambient_facts(c, c->have_probs), c->have_post, pools, power, min_pair_posterior, n_rows, post_rows, share_rows),
                         pools, {nullptr, nullptr, nullptr, nullptr, nullptr}, plan));
    DMX_TRY(dmx::run_mstep_doublet_shares_from_host(c, power, min_pair_posterior, plan, post_rows, share_rows, lp::pair_options(c->B, pools)));
    DMX_TRY(copy_out(c, addition_out, c->d_add.p, (size_t)c->V * c->G));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_run_iterations(dmx_ctx *c, int n_iterations, float lo, float hi, float power)
{
    DMX_TRY(bind(c));
    DMX_TRY(need(c, c->have_problem && c->have_betas && c->have_post && c->K > 0,
                 "dmx_estep or dmx_em (to fix the options) before dmx_run_iterations"));
    if (n_iterations < 0) return fail(DMX_ERR_INVALID, "negative n_iterations");
    const int with_doublets = c->K != c->G;
    for (int it = 0; it < n_iterations; it++) {
        const bool kept = it + 1 == n_iterations && c->logits_needed;  // somebody can read this E-step's logits
        DMX_TRY(run_pstep(c, lo, hi, true, !kept && ep::coarse_capable(estep_facts(c, with_doublets, false, kept), lo)));
        c->msteps_ahead = n_iterations - it;  // (read by the E-step too: the plan of the M-step behind it, for the codes' floor)
        const int rc_e = run_estep(c, with_doublets, false, DMX_F32, power, kept);
        const int rc_m = rc_e == 0 ? run_mstep(c, power) : rc_e;
        c->msteps_ahead = 0;
        if (rc_m) return rc_m;
    }
    return 0;
}

}  // extern "C"
