// ctx_state_check.cpp -- walks demuxalot_amd/csrc/ctx_state.h on the CPU (tests/test_ctx_state_cpu.py builds it with AddressSanitizer +
// UndefinedBehaviorSanitizer and runs it as a plain program).
//   1. every transition from many states: the flags it names take the stated values, every other flag keeps its own;
//   2. three call sequences as the host code composes them, the flags after every step: the M-step of a rank that exchanges sums, a
//      fetch of the addition, another M-step; a foreign writer of the addition between two incremental M-steps; a caller's
//      table between two P-steps;
//   3. seeded random sequences of those compositions against a model of what the buffers hold: the invariants of DESIGN.md 4.15.
#include <functional>
#include <random>

#include "ctx_state.h"
#include "plan_check.h"

using dmx::CtxState;

static bool same(const CtxState &a, const CtxState &b)
{
    return a.have_probs == b.have_probs && a.p_clip_lo == b.p_clip_lo && a.prob16_valid == b.prob16_valid && a.dict_candidate == b.dict_candidate &&
           a.prob_prev_valid == b.prob_prev_valid && a.emu_table_filled == b.emu_table_filled && a.add_is_zero == b.add_is_zero &&
           a.add_partial == b.add_partial && a.incr_valid == b.incr_valid && a.incr_power == b.incr_power && a.have_post == b.have_post &&
           a.have_post64 == b.have_post64 && a.post_gathered == b.post_gathered && a.dense_stat_valid == b.dense_stat_valid &&
           a.nz_floor == b.nz_floor && a.nz_rebuilds == b.nz_rebuilds && a.guard_ran == b.guard_ran && a.logits_readable == b.logits_readable;
}
// (printed at the end; tests/test_ctx_state_cpu.py counts the header's flags, so one added there without a line in same() shows)
static const int FLAGS_COMPARED = 18;

static CtxState random_state(std::mt19937 &rng)
{
    const float values[4] = {0.0f, 0.01f, 2.0f, 1.5f};
    auto bit = [&] { return (rng() & 1u) != 0; };
    CtxState s;
    s.have_probs = bit(), s.prob16_valid = bit(), s.dict_candidate = bit(), s.prob_prev_valid = bit(), s.emu_table_filled = bit();
    s.add_is_zero = bit(), s.add_partial = bit(), s.incr_valid = bit(), s.have_post = bit(), s.have_post64 = bit();
    s.post_gathered = bit(), s.dense_stat_valid = bit(), s.guard_ran = bit(), s.logits_readable = bit();
    s.p_clip_lo = values[rng() % 4], s.incr_power = values[rng() % 4], s.nz_floor = values[rng() % 4];
    s.nz_rebuilds = (long long)(rng() % 5);
    return s;
}

// ---- 1. one transition: `apply` on the header's side, `stated` as this file says it, from the defaults and 64 random states ----
static void transition(const char *name, const std::function<void(CtxState &)> &apply, const std::function<void(CtxState &)> &stated)
{
    std::mt19937 rng(20240607u);
    std::vector<CtxState> starts(1);  // (the defaults)
    for (int i = 0; i < 64; i++) starts.push_back(random_state(rng));
    int bad = 0;
    for (const CtxState &from : starts) {
        CtxState got = from, want = from;
        apply(got);
        stated(want);
        if (!same(got, want)) bad++;
    }
    checks++;
    if (bad) {
        failures++;
        std::printf("%s: %d of %d start states end elsewhere than stated\n", name, bad, (int)starts.size());
    }
}
#define T(call, ...) transition(#call, [&](CtxState &s) { s.call; }, [&](CtxState &s) { __VA_ARGS__; })

static void every_transition()
{
    for (const bool b : {false, true}) {
        T(pstep_launched(b), s.prob16_valid = b);
        T(changed_rows_applied(b), s.prob16_valid = b);
        T(half_table_converted(b), s.prob16_valid = b);
        T(addition_set_by_caller(b), s.add_is_zero = b; s.add_partial = false);
        T(estep_done(b), s.have_post = true; s.logits_readable = b);
        T(float64_posteriors_written(b), if (b) s.have_post = false; s.have_post64 = true);
        for (const float x : {0.0f, 0.01f, 0.25f}) {
            T(table_written_by_pstep(x, b), s.have_probs = true; s.p_clip_lo = x; s.dict_candidate = !b || s.add_is_zero);
            T(estep_begins(b, x), s.post_gathered = false; s.dense_stat_valid = b; s.nz_floor = x; s.guard_ran = false);
        }
        for (const int n : {1, 2, 8}) T(addition_written_by_mstep(b, n), if (b) s.add_partial = n > 1);
    }
    for (const float x : {0.0f, 0.01f, 2.0f}) {
        T(table_written_from_f64_betas(x), s.have_probs = true; s.p_clip_lo = x; s.prob16_valid = false; s.dict_candidate = true);
        T(kept_sums_started(x), s.incr_valid = true; s.incr_power = x);
        T(dense_pass_done(x), s.post_gathered = false; s.dense_stat_valid = false; s.nz_floor = x; s.guard_ran = false; s.have_post = true; s.logits_readable = false);
        T(codes_rebuilt(x), s.nz_floor = x; s.post_gathered = false; s.nz_rebuilds += 1);
    }
    T(sent_slice_forgotten(), s.prob_prev_valid = false);
    T(sent_slice_recorded(), s.prob_prev_valid = true);
    T(half_table_reallocated(), s.prob16_valid = false);
    T(pstep_begins(), s.prob16_valid = false);
    T(emulated_slices_filled(), s.emu_table_filled = true);
    T(table_written_by_caller(), s.have_probs = true; s.p_clip_lo = 0.0f; s.prob16_valid = false; s.dict_candidate = true);
    T(table_layout_changed(), s.have_probs = false; s.emu_table_filled = false);
    T(addition_zeroed(), s.incr_valid = false; s.add_is_zero = true; s.add_partial = false);
    T(addition_written_by_other_form(), s.add_is_zero = false; s.add_partial = false; s.incr_valid = false);
    T(mstep_begins(), s.add_is_zero = false);
    T(addition_gathered(), s.add_partial = false);
    T(exchange_laid_out(), s.add_partial = false);
    T(kept_sums_dropped(), s.incr_valid = false);
    T(guard_evaluated(), s.guard_ran = true);
    T(posteriors_gathered(), s.post_gathered = true);
    T(gathered_tables_reset(), s.post_gathered = false);
    T(posteriors_dropped(), s.have_post = false);
    T(float64_posteriors_dropped(), s.have_post64 = false);
    T(rebuild_count_reset(), s.nz_rebuilds = 0);
    T(dictionary_released(), s.dict_candidate = false; s.add_is_zero = true);
    T(guard_released(), s.guard_ran = false);
    T(exchange_released(), s.prob_prev_valid = false; s.post_gathered = false; s.add_partial = false);
    T(problem_released(), s.prob16_valid = false; s.dense_stat_valid = false; s.have_probs = false; s.have_post = false);
}

// ---- the host code's compositions (dmx_steps.cpp, mstep_weighted.hip, dmx_runtime.cpp), with a model of what the buffers hold ----
struct Model {
    CtxState s;
    int nranks = 1;
    bool slice_only = false;       // the M-step's destination (a rank that reduce-scatters its sums)
    // what the buffers hold
    bool add_zero = true;          // d_add is all zeros
    bool add_whole = true;         // every slice of d_add is current
    bool add_is_kept_sums = false; // d_add is what the sums of d_acc64 round to
    float kept_power = -1.0f;      // the power d_acc64 was summed at
    bool table_without_addition = false;  // d_prob was formed from betas alone, from a zero addition, or by the caller
    bool half_current = false;     // d_prob16 was written from the current d_prob
    float codes_floor = 0.0f;      // the floor d_nz / d_first were built with
    bool gathered_current = false; // the global tables hold the codes as they are
    bool post_written = false;     // d_post holds an E-step's result
    long long full_passes = 0, delta_passes = 0;

    void pstep(float lo, bool with_addition, bool with_half)
    {
        s.pstep_begins();
        s.pstep_launched(with_half);
        s.table_written_by_pstep(lo, with_addition);
        table_without_addition = !with_addition || add_zero;
        half_current = with_half;
    }
    void set_probs()
    {
        s.sent_slice_forgotten();
        s.table_written_by_caller();
        table_without_addition = true;
        half_current = false;
    }
    void estep(float floor, bool guarded, bool logits_kept)
    {
        s.estep_begins(true, floor);
        if (guarded) s.guard_evaluated();
        s.estep_done(logits_kept);
        codes_floor = floor, gathered_current = false, post_written = true;
    }
    void dense_pooled_estep(float floor)
    {
        s.posteriors_dropped();
        post_written = false;
        s.dense_pass_done(floor);
        codes_floor = floor, gathered_current = false, post_written = true;
    }
    void rebuild(float floor)
    {
        s.codes_rebuilt(floor);
        codes_floor = floor, gathered_current = false;
    }
    void mstep(float power, bool incremental)  // run_mstep; the rebuilds as it decides them for the float64 floor 0
    {
        if (power != 2.0f && s.nz_floor != 0.0f) rebuild(0.0f);
        if (nranks > 1) s.posteriors_gathered(), gathered_current = true;
        s.mstep_begins();
        if (incremental) {
            const bool full = !s.incr_valid || s.incr_power != power;
            if (full) s.kept_sums_started(power), kept_power = power;
            (full ? full_passes : delta_passes)++;
            add_is_kept_sums = true;
        } else {
            s.kept_sums_dropped();
            add_is_kept_sums = false;
        }
        s.addition_written_by_mstep(slice_only, nranks);
        add_zero = false;
        if (slice_only) add_whole = nranks == 1;
    }
    void fetch_addition()  // ensure_full_addition
    {
        if (!s.add_partial) return;
        s.addition_gathered();
        add_whole = true;
    }
    void weighted_mstep(float floor)  // begin_weighted_mstep; the float64 M-step of aggregate_on_snps ends alike
    {
        if (s.nz_floor > floor) rebuild(floor);
        s.addition_written_by_other_form();
        add_zero = false, add_whole = true, add_is_kept_sums = false;
    }
    void set_addition(bool zeros)
    {
        s.kept_sums_dropped();
        s.addition_set_by_caller(zeros);
        add_zero = zeros, add_whole = true, add_is_kept_sums = false;
    }
    void em_begins()
    {
        s.addition_zeroed();
        add_zero = true, add_whole = true, add_is_kept_sums = false;
    }
    void switch_incremental() { s.kept_sums_dropped(), add_is_kept_sums = false; }
    void release_problem()
    {
        s.kept_sums_dropped();  // release_mstep_tiles, release_incremental
        s.dictionary_released();
        s.guard_released();
        s.exchange_released();
        s.float64_posteriors_dropped();
        s.problem_released();
        add_zero = true, add_whole = true, add_is_kept_sums = false, half_current = false, post_written = false, gathered_current = false;
        table_without_addition = false;
    }

    void invariants() const
    {
        EXPECT(!s.incr_valid || (add_is_kept_sums && s.incr_power == kept_power));  // the kept sums describe the addition, at their power
        EXPECT(!s.add_is_zero || add_zero);
        EXPECT(s.add_partial == !add_whole);
        EXPECT(!s.add_partial || nranks > 1);
        EXPECT(!s.dict_candidate || table_without_addition);
        EXPECT(!s.prob16_valid || half_current);
        EXPECT(!s.post_gathered || gathered_current);
        EXPECT(!s.have_post || post_written);
        EXPECT(!post_written || s.nz_floor == codes_floor);
        EXPECT(s.nz_rebuilds >= 0);
        EXPECT(!s.guard_ran || s.have_post);
    }
};

static void advice_sequence()
{
    Model m;
    m.nranks = 2, m.slice_only = true;
    m.em_begins();
    m.pstep(0.01f, true, false);
    m.estep(0.0f, false, true);
    m.mstep(2.0f, true);
    EXPECT(m.s.incr_valid && m.s.add_partial && !m.s.add_is_zero && m.full_passes == 1);
    m.fetch_addition();  // (the gather has a buffer of its own: the sums the next M-step builds on are untouched)
    EXPECT(m.s.incr_valid && !m.s.add_partial && !m.s.add_is_zero);
    m.invariants();
    m.pstep(0.01f, true, false);
    EXPECT(!m.s.dict_candidate);
    m.estep(0.0f, false, true);
    m.mstep(2.0f, true);
    EXPECT(m.s.incr_valid && m.s.add_partial && m.full_passes == 1 && m.delta_passes == 1);
    m.invariants();
}

static void foreign_writer_sequence()
{
    Model m;
    m.em_begins();
    for (int i = 0; i < 2; i++) m.pstep(0.01f, true, true), m.estep(2.0f, true, true), m.mstep(2.0f, true);
    EXPECT(m.s.incr_valid && m.s.incr_power == 2.0f && m.full_passes == 1 && m.delta_passes == 1 && m.s.nz_rebuilds == 0);
    m.pstep(0.01f, true, false);
    m.dense_pooled_estep(0.0f);
    EXPECT(m.s.have_post && !m.s.logits_readable && !m.s.dense_stat_valid && !m.s.guard_ran && m.s.incr_valid);
    m.weighted_mstep(0.0f);
    EXPECT(!m.s.incr_valid && !m.s.add_is_zero && !m.s.add_partial && m.s.nz_rebuilds == 0);
    m.invariants();
    m.pstep(0.01f, true, true), m.estep(2.0f, true, true), m.mstep(2.0f, true);
    EXPECT(m.s.incr_valid && m.full_passes == 2 && m.delta_passes == 1);
    m.pstep(0.01f, true, true), m.estep(2.0f, true, true);
    m.weighted_mstep(0.0f);  // behind an E-step that wrote the codes at a fixed-point floor: rebuilt
    EXPECT(m.s.nz_rebuilds == 1 && m.s.nz_floor == 0.0f && !m.s.incr_valid);
    m.estep(2.0f, true, true), m.mstep(2.0f, true);
    EXPECT(m.full_passes == 3 && m.delta_passes == 1);
    m.estep(2.0f, true, true), m.mstep(2.0f, true);
    EXPECT(m.full_passes == 3 && m.delta_passes == 2);
    m.invariants();
}

static void callers_table_sequence()
{
    Model m;
    m.pstep(0.01f, true, true);  // (no M-step yet: the addition is zero)
    EXPECT(m.s.have_probs && m.s.p_clip_lo == 0.01f && m.s.prob16_valid && m.s.dict_candidate);
    m.estep(0.0f, false, true), m.mstep(2.0f, false);
    m.pstep(0.01f, true, true);
    EXPECT(m.s.prob16_valid && !m.s.dict_candidate);
    m.s.sent_slice_recorded();
    m.set_probs();
    EXPECT(m.s.have_probs && m.s.p_clip_lo == 0.0f && !m.s.prob16_valid && m.s.dict_candidate && !m.s.prob_prev_valid);
    m.invariants();
    m.pstep(0.02f, true, false);
    EXPECT(m.s.p_clip_lo == 0.02f && !m.s.prob16_valid && !m.s.dict_candidate);
    m.pstep(0.02f, false, true);
    EXPECT(m.s.prob16_valid && m.s.dict_candidate);
    m.invariants();
}

static void random_sequences()
{
    std::mt19937 rng(7u);
    const float floors[2] = {0.0f, 2.0f}, powers[2] = {2.0f, 1.5f};
    for (int run = 0; run < 200; run++) {
        Model m;
        m.nranks = 1 + (int)(rng() % 3);
        m.slice_only = m.nranks > 1 && (rng() & 1u);
        for (int step = 0; step < 60; step++) {
            const unsigned r = rng();
            switch (r % 12) {
            case 0: m.pstep(0.01f, (r >> 8) & 1u, (r >> 9) & 1u); break;
            case 1: m.set_probs(); break;
            case 2: m.estep(floors[(r >> 8) & 1u], (r >> 9) & 1u, (r >> 10) & 1u); break;
            case 3: m.dense_pooled_estep(floors[(r >> 8) & 1u]); break;
            case 4: case 5: if (m.post_written) m.mstep(powers[(r >> 8) % 2], (r >> 9) % 4 != 0); break;
            case 6: m.fetch_addition(); break;
            case 7: if (m.post_written) m.weighted_mstep(0.0f); break;
            case 8: m.set_addition((r >> 8) & 1u); break;
            case 9: m.em_begins(); break;
            case 10: m.switch_incremental(); break;
            default: if ((r >> 8) % 8 == 0) m.release_problem(); break;
            }
            m.invariants();
        }
    }
}

int main()
{
    every_transition();
    advice_sequence();
    foreign_writer_sequence();
    callers_table_sequence();
    random_sequences();
    std::printf("ctx state: %d flags compared, %d checks, %d failures\n", FLAGS_COMPARED, checks, failures);
    return failures ? 1 : 0;
}
