// The M-step's policy (demuxalot_amd/csrc/mstep_plan.h) over the whole cross product of its fact space, on the CPU: the invariants every
// combination must keep, then the named rows of the decision table in DESIGN.md 2.7 one by one.  Built with -fsanitize=address,undefined
// and run by tests/test_mstep_plan_cpu.py; prints the number of combinations walked.
#include <cstdio>

#include "mstep_plan.h"

using namespace dmx::mplan;

static long long failures = 0;
static Facts failed;  // (a copy: the checked facts themselves never leave their registers, which keeps the walk quick under the sanitizers)
static void report(const char *what, int line)
{
    const Facts &f = failed;
    if (failures++ < 20)
        std::fprintf(stderr,
                     "line %d: %s\n  tiles %d incr %d exact %d G %d calls %d power %g | attached %d mshard %d sliced %d f64 %d | pairs %d item_variant %d shift_v %d "
                     "state %d slice_rec %d | n_mt %lld tried %d done %lld ahead %lld expected %lld heavy %d rows_total %lld\n",
                     line, what, f.mstep_tiles, f.mstep_incremental, f.exact_additions, f.G, f.has_calls, f.power, f.attached, f.mshard, f.sliced, f.reduce_f64,
                     f.has_call_pairs, f.has_item_variant, f.has_shift_v, f.has_incr_state, f.has_slice_rec, f.n_mt, f.mt_tried, f.msteps_done, f.msteps_ahead,
                     f.msteps_expected, f.incr_heavy, f.rows_total);
}
#define CHECK(cond) ((cond) ? (void)0 : (failed = f, report(#cond, __LINE__)))
#define IMPLIES(a, b) CHECK(!(a) || (b))

static const long long CUT[4] = {0, 10, 25, 40};  // three ranks' cuts of 40 variants; the facts' rank is 1

static inline void invariants(const Facts f)
{
    const Launch l = launch(f);
    const Dest d = destination(f);
    const bool eligible = !f.exact_additions && f.G <= 64 && f.has_calls && f.power > 0.0f;
    const bool incremental = l.incr != INCR_NONE, wanted = records_wanted(f), ready = tiles_ready(f), shifts = shifts_wanted(f), can = can_go_incremental(f);
    CHECK(l.form >= 1 && l.form <= 3);
    IMPLIES(f.exact_additions, l.form == 1 && !incremental);
    IMPLIES(incremental, l.form == 2 || l.form == 3);
    IMPLIES(l.incr == INCR_SHARDED, f.mshard && l.form == 2);
    IMPLIES(l.form == 2 || l.form == 3, f.G <= 64 && f.power > 0.0f && f.has_calls);
    IMPLIES(f.mstep_tiles == 0, l.form == 1);
    IMPLIES(f.mstep_tiles == 2 && eligible, wanted);
    IMPLIES(!eligible, !wanted && !shifts);
    // the forms and the kinds go together; what a kind builds on is there
    CHECK((l.form == 3) == (l.incr == INCR_WORK_ITEMS));
    CHECK((l.form == 2) == ready);
    IMPLIES(l.incr == INCR_OWN_RECORDS, l.form == 2 && !f.mshard);
    IMPLIES(incremental, f.mstep_incremental != 0 && f.has_shift_v);
    IMPLIES(incremental && l.incr != INCR_SHARDED, f.has_call_pairs && !f.mshard && (!f.attached || f.sliced));
    IMPLIES(l.incr == INCR_SHARDED, f.mstep_incremental == 1 && f.has_item_variant && f.rows_total > 0 && d.then == EXCH_NONE && !d.exchange_buffer);
    IMPLIES(f.attached && !f.mshard && !f.sliced, !incremental);  // the all-reduce sums in place: never incremental
    CHECK(l.row_variant == (incremental && l.incr != INCR_SHARDED && f.sliced));
    // the stages
    IMPLIES(build_due(f), wanted && !f.mt_tried && f.mstep_tiles != 0);
    IMPLIES(wanted && !f.mt_tried, build_due(f));
    // the horizon is the running call's or the announced one, whichever is longer; 8 M-steps seen count like 8 to come
    IMPLIES(f.mstep_tiles == 1 && eligible && !can && std::max({f.msteps_ahead, f.msteps_expected, f.msteps_done}) >= 8, wanted);
    IMPLIES(f.mstep_tiles == 1 && f.n_mt == 0 && std::max({f.msteps_ahead, f.msteps_expected, f.msteps_done}) < 8, !wanted);
    IMPLIES(ready, wanted && f.n_mt > 0);
    CHECK(!(ready && shifts));
    IMPLIES(shifts, f.mstep_tiles != 0 && f.mstep_incremental != 0 && f.has_item_variant);
    // the probe: only at M-steps 4, 16 and 64 of a context that can go incremental, is not yet heavy and has no records
    IMPLIES(probe_due(f), (f.msteps_done == 4 || f.msteps_done == 16 || f.msteps_done == 64) && can && !f.incr_heavy && f.n_mt == 0 &&
                              f.has_incr_state);
    IMPLIES(can, f.mstep_tiles == 1 && f.mstep_incremental != 0 && eligible && f.has_call_pairs && f.has_item_variant);
    // a context that can go incremental and is not heavy builds no records in auto mode, however long the run
    IMPLIES(can && !f.incr_heavy && f.n_mt == 0, !wanted);
    // the destination of the sums
    if (!f.attached || f.mshard) CHECK(!d.exchange_buffer && !d.f64 && d.then == EXCH_NONE);  // d_add float32, no prow
    else if (f.sliced) CHECK(d.exchange_buffer && d.f64 == f.reduce_f64 && d.then == EXCH_REDUCE_SCATTER);  // exchange buffer with prow in the reduce dtype
    else CHECK(!d.exchange_buffer && d.f64 == f.reduce_f64 && d.then == EXCH_ALL_REDUCE);  // d_add / d_add64 by dtype
    CHECK(d.slice_only == (f.attached && (f.mshard || f.sliced)));
    const Range r = variant_range(f, CUT, 1, 40);
    CHECK(f.mshard ? r.v0 == 10 && r.v1 == 25 : r.v0 == 0 && r.v1 == 40);
}

static long long walk()
{
    const int Gs[] = {8, 64, 65};
    const float powers[] = {2.0f, 1.5f, 0.0f};
    const long long dones[] = {0, 3, 4, 5, 8, 16, 64}, aheads[] = {0, 7, 8};
    long long n = 0;
    Facts f{};
    for (int bits = 0; bits < (1 << 14); bits++) {  // every boolean both ways
        const auto bit = [&](int i) { return ((bits >> i) & 1) != 0; };
        f.exact_additions = bit(0), f.has_calls = bit(1), f.attached = bit(2), f.mshard = bit(3), f.sliced = bit(4), f.reduce_f64 = bit(5);
        f.has_call_pairs = bit(6), f.has_item_variant = bit(7), f.has_shift_v = bit(8), f.has_incr_state = bit(9), f.has_slice_rec = bit(10);
        f.mt_tried = bit(11), f.incr_heavy = bit(12);
        f.n_mt = bit(13) ? 37 : 0;
        for (int tiles = 0; tiles <= 2; tiles++)
            for (int incr = 0; incr <= 2; incr++)
                for (int G : Gs)
                    for (float power : powers)
                        for (long long done : dones)
                            for (long long ahead : aheads)
                                for (long long expected : {0ll, 8ll})  // (dmx_set_msteps_expected)
                                    for (long long rows_total : {0ll, 4000ll}) {
                                        f.mstep_tiles = tiles, f.mstep_incremental = incr, f.G = G, f.power = power, f.msteps_done = done;
                                        f.msteps_ahead = ahead, f.msteps_expected = expected, f.rows_total = rows_total;
                                        invariants(f);
                                        n++;
                                    }
    }
    // incr_heavy after a probe: at the 4th M-step <=> three full passes, later <=> half of the M-steps
    for (long long done : {4ll, 16ll, 64ll})
        for (unsigned count = 0; count <= 70; count++) {
            f.msteps_done = done;
            CHECK(heavy_after_probe(f, count) == (done == 4 ? count >= 3 : 2 * (long long)count >= done));
        }
    return n;
}

// one context, all defaults, the repack's records there, nothing built yet: the first M-step of a call with `ahead` M-steps to come
static Facts one_context(long long ahead)
{
    Facts f{};
    f.mstep_tiles = 1, f.mstep_incremental = 1, f.exact_additions = false, f.G = 64, f.has_calls = true, f.power = 2.0f;
    f.has_call_pairs = f.has_item_variant = true;
    f.msteps_ahead = ahead;
    return f;
}

static void table_rows()
{
    {  // learn_genotypes' 5-iteration call (4 M-steps): no records, the work items with the tile cut's exponents, incremental on them
        Facts f = one_context(4);
        CHECK(!probe_due(f) && !records_wanted(f) && !build_due(f) && shifts_wanted(f));
        f.has_shift_v = true;  // (plan_mstep_shifts)
        CHECK(launch(f).form == 3 && launch(f).incr == INCR_WORK_ITEMS && !launch(f).row_variant);
        CHECK(!destination(f).exchange_buffer && !destination(f).f64 && destination(f).then == EXCH_NONE && !destination(f).slice_only);
        f.has_shift_v = false;  // (the problem does not take the tile cut: the float64 work items)
        CHECK(launch(f).form == 1 && launch(f).incr == INCR_NONE);
    }
    {  // a converging 25-iteration call starts the same way and stays there: the probe at its 4th M-step finds two full passes
        Facts f = one_context(24);
        CHECK(!records_wanted(f) && shifts_wanted(f));
        f.has_shift_v = f.has_incr_state = true, f.msteps_done = 4, f.msteps_ahead = 20;
        CHECK(probe_due(f) && !heavy_after_probe(f, 2));
        CHECK(!records_wanted(f) && launch(f).form == 3);
    }
    {  // a 25-iteration call on a heavy problem (three full passes in the first four M-steps): the records are built at once
        Facts f = one_context(20);
        f.has_shift_v = f.has_incr_state = true, f.msteps_done = 4;
        CHECK(probe_due(f) && heavy_after_probe(f, 3));
        f.incr_heavy = true;
        CHECK(!probe_due(f) && records_wanted(f) && build_due(f));
        f.n_mt = 37, f.mt_tried = true;  // (build_mstep_tiles)
        CHECK(!build_due(f) && !shifts_wanted(f) && launch(f).form == 2 && launch(f).incr == INCR_OWN_RECORDS);
        f.n_mt = 0;  // (the build left nothing: the work items again)
        CHECK(!build_due(f) && shifts_wanted(f) && launch(f).form == 3);
        f = one_context(24), f.incr_heavy = true;  // known heavy from an earlier call: at the first M-step
        CHECK(records_wanted(f) && build_due(f));
    }
    {  // dmx_set_mstep_incremental(0): records when 8 M-steps are to come or have been seen, else the float64 work items
        Facts f = one_context(8);
        f.mstep_incremental = 0;
        CHECK(records_wanted(f) && build_due(f));
        f.n_mt = 37, f.mt_tried = true;
        CHECK(launch(f).form == 2 && launch(f).incr == INCR_NONE);
        f = one_context(7), f.mstep_incremental = 0;
        CHECK(!records_wanted(f) && !shifts_wanted(f) && launch(f).form == 1);
        f.msteps_done = 8, f.msteps_ahead = 0;
        CHECK(records_wanted(f));
    }
    {  // exact additions: the float64 work items, whatever else is set
        Facts f = one_context(24);
        f.exact_additions = true, f.mstep_tiles = 2, f.n_mt = 37, f.has_shift_v = true;
        CHECK(!records_wanted(f) && !shifts_wanted(f) && launch(f).form == 1 && launch(f).incr == INCR_NONE);
    }
    for (int f64 = 0; f64 < 2; f64++) {  // a reduce-scatter rank: incremental on its own sums in the exchange buffer, padded rows brought back by row_variant
        Facts f = one_context(4);
        f.attached = f.sliced = true, f.reduce_f64 = f64 != 0, f.has_shift_v = true;
        CHECK(shifts_wanted(f) && launch(f).form == 3 && launch(f).incr == INCR_WORK_ITEMS && launch(f).row_variant);
        const Dest d = destination(f);
        CHECK(d.exchange_buffer && d.f64 == (f64 != 0) && d.then == EXCH_REDUCE_SCATTER && d.slice_only);
        f.mstep_tiles = 2, f.n_mt = 37, f.mt_tried = true;
        CHECK(launch(f).form == 2 && launch(f).incr == INCR_OWN_RECORDS && launch(f).row_variant);
        CHECK(variant_range(f, CUT, 1, 40).v0 == 0 && variant_range(f, CUT, 1, 40).v1 == 40);
    }
    {  // a variant-sharded rank: records when 8 M-steps are to come (its records are not its barcodes': no work-item start), then sharded incremental
        Facts f = one_context(7);
        f.attached = f.mshard = true, f.has_call_pairs = true, f.rows_total = 4000;
        CHECK(!can_go_incremental(f) && !records_wanted(f) && !shifts_wanted(f) && launch(f).form == 1 && launch(f).incr == INCR_NONE);
        f.msteps_ahead = 8;
        CHECK(records_wanted(f) && build_due(f));
        f.n_mt = 37, f.mt_tried = f.has_shift_v = true;
        CHECK(launch(f).form == 2 && launch(f).incr == INCR_SHARDED && !launch(f).row_variant && !sharded_by_row_index(f));  // the masked walk
        f.has_slice_rec = true;
        CHECK(launch(f).incr == INCR_SHARDED && sharded_by_row_index(f));  // the slice's records by barcode row
        const Dest d = destination(f);
        CHECK(!d.exchange_buffer && !d.f64 && d.then == EXCH_NONE && d.slice_only);
        CHECK(variant_range(f, CUT, 1, 40).v0 == 10 && variant_range(f, CUT, 1, 40).v1 == 25);
        f.mstep_incremental = 2;  // (the measurement path is one context's)
        CHECK(launch(f).form == 2 && launch(f).incr == INCR_NONE);
    }
    for (int f64 = 0; f64 < 2; f64++) {  // an all-reduce rank (scattered SNPs): never incremental, tiles when they pay, sums in d_add / d_add64
        Facts f = one_context(24);
        f.attached = true, f.reduce_f64 = f64 != 0, f.has_shift_v = true;
        CHECK(!can_go_incremental(f) && !shifts_wanted(f) && records_wanted(f));
        CHECK(launch(f).form == 1 && launch(f).incr == INCR_NONE);
        f.n_mt = 37, f.mt_tried = true;
        CHECK(launch(f).form == 2 && launch(f).incr == INCR_NONE);
        const Dest d = destination(f);
        CHECK(!d.exchange_buffer && d.f64 == (f64 != 0) && d.then == EXCH_ALL_REDUCE && !d.slice_only);
    }
}

int main()
{
    const long long n = walk();
    table_rows();
    std::printf("mstep plan: %lld combinations walked, %lld failures\n", n, failures);
    return failures ? 1 : 0;
}
