// ctx_state.h -- which derived device data of a context is current, and every event that changes that (the flag x
// transition table and the invariants).  Host only: nothing of HIP, nothing of dmx_ctx, which derives from CtxState - every read stays
// c->flag, every write is one of the member functions below, named for what happened to a buffer and not for the flags it sets.
// No file but this one assigns a flag (tests/test_ctx_state_cpu.py reads the sources; tests/ctx_state_check.cpp walks the transitions).
// A transition writes exactly what its comment names, in the order the sites it replaced wrote them.
#pragma once

namespace dmx {

struct CtxState {
    // ---- the genotype table (d_prob) ----
    bool have_probs = false;
    float p_clip_lo = 0.0f;        // lower clip of the P-step that produced d_prob (0: a caller's table, dmx_set_probs)
    bool prob16_valid = false;     // d_prob16 holds the current d_prob
    bool dict_candidate = false;   // the current d_prob was computed without an addition, or set by the caller
    bool prob_prev_valid = false;  // d_prob_prev is what every rank holds of this slice
    bool emu_table_filled = false;  // emulated wire: the other ranks' slices of genotype_prob hold the table without addition
    // ---- the addition (d_add) ----
    bool add_is_zero = true;   // d_add holds zeros (no M-step / dmx_set_addition since the last reset)
    bool add_partial = false;  // only this rank's slice of d_add is current (sliced mode, after an M-step)
    bool incr_valid = false;   // the incremental M-step's device state may be trusted (else the state words are zeroed: a full pass)
    float incr_power = 0.0f;   // contribution power of the sums in d_acc64
    // ---- the posteriors and their codes (d_post, d_nz, d_first) ----
    bool have_post = false;
    bool have_post64 = false;       // d_logits64 / d_post64 hold the results of dmx_estep_snp
    bool post_gathered = false;     // variant-sharded M-step: the global tables hold the last E-step of every rank
    bool dense_stat_valid = false;  // d_dense_calls holds the last E-step's statistic
    float nz_floor = 0.0f;          // threshold the current d_nz / d_first were built with
    long long nz_rebuilds = 0;      // launches of k_rebuild_nz by the M-steps since dmx_reset_timings (the codes' floor did not fit the M-step's form)
    bool guard_ran = false;         // the last E-step evaluated the guard
    bool logits_readable = true;    // the last E-step's logits are the fine pass's / the exact kernel's (dmx_get_logits, dmx_get_block)

    // ---- the genotype table ----
    // d_prob is about to be written outside the sliced P-step (a caller's table, the float64 P-step on every rank), or d_prob_prev went
    // with its layout: what the ranks hold of each other's slices is no longer what they sent
    void sent_slice_forgotten() { prob_prev_valid = false; }
    // the first table of a layout (or the one behind a table somebody else wrote) was copied to d_prob_prev as it was sent
    void sent_slice_recorded() { prob_prev_valid = true; }
    // d_prob16 was allocated anew
    void half_table_reallocated() { prob16_valid = false; }
    // run_pstep is about to overwrite d_prob
    void pstep_begins() { prob16_valid = false; }
    // emulated wire: run_pstep filled the other ranks' slices once
    void emulated_slices_filled() { emu_table_filled = true; }
    // the P-step kernel wrote this rank's rows, as binary16 too where the whole table is its own (one rank, with_half)
    void pstep_launched(bool with_half) { prob16_valid = with_half; }
    // sliced P-step: the other ranks' changed rows were applied from their lists, as binary16 too where the table was valid before
    void changed_rows_applied(bool half_rows) { prob16_valid = half_rows; }
    // run_pstep is through, exchange included
    void table_written_by_pstep(float lo, bool with_addition)
    {
        have_probs = true;
        p_clip_lo = lo;
        dict_candidate = !with_addition || add_is_zero;
    }
    // dmx_set_probs accepted the table (entries may lie below binary16's normal range: no coarse pass)
    void table_written_by_caller()
    {
        have_probs = true;
        p_clip_lo = 0.0f;
        prob16_valid = false;
        dict_candidate = true;
    }
    // dmx_probs_from_betas_f64: computed from the caller's betas, no addition
    void table_written_from_f64_betas(float lo)
    {
        have_probs = true;
        p_clip_lo = lo;
        prob16_valid = false;
        dict_candidate = true;
    }
    // layout_exchange allocated / zeroed d_prob for another row layout
    void table_layout_changed()
    {
        have_probs = false;
        emu_table_filled = false;
    }
    // the guarded E-step converted d_prob to binary16 (kept: the conversion was not left to the device's choice)
    void half_table_converted(bool kept) { prob16_valid = kept; }

    // ---- the addition ----
    // an EM call starts from a zero addition, which no kept state of an earlier M-step describes
    void addition_zeroed()
    {
        incr_valid = false;
        add_is_zero = true;
        add_partial = false;
    }
    // dmx_set_addition uploaded a table (zeros: a null one)
    void addition_set_by_caller(bool zeros)
    {
        add_is_zero = zeros;
        add_partial = false;
    }
    // a form that keeps no sums (the table-weighted M-steps, the float64 M-step) writes the whole of d_add
    void addition_written_by_other_form()
    {
        add_is_zero = false;
        add_partial = false;
        incr_valid = false;
    }
    // run_mstep: ahead of the plan and the launches
    void mstep_begins() { add_is_zero = false; }
    // run_mstep: the combine and the exchange it named went through; a reduce-scatter leaves this rank's slice only
    void addition_written_by_mstep(bool slice_only, int nranks)
    {
        if (slice_only) add_partial = nranks > 1;
    }
    // ensure_full_addition all-gathered the slices
    void addition_gathered() { add_partial = false; }
    // layout_exchange is through: d_add is one table in the new layout
    void exchange_laid_out() { add_partial = false; }
    // the sums of d_acc64 no longer describe d_add, or what they were built with is gone (another form's M-step, a caller's addition,
    // the switch of dmx_set_mstep_incremental, the tiles' exponents, the state's first allocation or its release)
    void kept_sums_dropped() { incr_valid = false; }
    // the incremental M-step's state words were zeroed for a full pass at this power
    void kept_sums_started(float power)
    {
        incr_valid = true;
        incr_power = power;
    }

    // ---- the posteriors and their codes ----
    // run_estep, ahead of its launches (dense_stat: d_dense_calls was offered to the kernels; floor: what they build the codes with)
    void estep_begins(bool dense_stat, float floor)
    {
        post_gathered = false;
        dense_stat_valid = dense_stat;
        nz_floor = floor;
        guard_ran = false;
    }
    // the guarded step's fast kernels and its redo were launched
    void guard_evaluated() { guard_ran = true; }
    // run_estep, behind its launches (an E-step nobody was to read the logits of may have taken the coarse pass: the device's choice)
    void estep_done(bool logits_kept)
    {
        have_post = true;
        logits_readable = logits_kept;
    }
    // a dense pooled pass wrote d_post [B, G] and rebuilt the codes at `floor`: as run_estep leaves the context, without the
    // statistic of the dense calls and with nothing of this pass in d_logits
    void dense_pass_done(float floor)
    {
        post_gathered = false;
        dense_stat_valid = false;
        nz_floor = floor;
        guard_ran = false;
        have_post = true;
        logits_readable = false;
    }
    // k_rebuild_nz rewrote d_nz / d_first from the stored posteriors at another floor
    void codes_rebuilt(float floor)
    {
        nz_floor = floor;
        post_gathered = false;
        nz_rebuilds++;
    }
    // gather_posteriors went through
    void posteriors_gathered() { post_gathered = true; }
    // shard_mstep_by_variant allocated the global tables
    void gathered_tables_reset() { post_gathered = false; }
    // d_post was zeroed for a dense pooled call, or laid out for another K
    void posteriors_dropped() { have_post = false; }
    // dmx_estep_snp wrote d_logits64 / d_post64 (k_changed: the float32 tables and the bitmaps were laid out for the previous K)
    void float64_posteriors_written(bool k_changed)
    {
        if (k_changed) have_post = false;
        have_post64 = true;
    }
    // the float64 results were laid out for another K, or freed
    void float64_posteriors_dropped() { have_post64 = false; }
    // dmx_reset_timings
    void rebuild_count_reset() { nz_rebuilds = 0; }

    // ---- what the release_* helpers of dmx_runtime.cpp reset (nz_floor, logits_readable, p_clip_lo and incr_power stay as they are) ----
    void dictionary_released()
    {
        dict_candidate = false;
        add_is_zero = true;
    }
    void guard_released() { guard_ran = false; }
    void exchange_released()
    {
        prob_prev_valid = false;
        post_gathered = false;
        add_partial = false;
    }
    void problem_released()
    {
        prob16_valid = dense_stat_valid = false;
        have_probs = have_post = false;
    }
};

}  // namespace dmx
