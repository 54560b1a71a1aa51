// The live floor of the fixed-point M-step forms (demuxalot_amd/csrc/kernels.h: live_floor_fixed; mstep_plan.h: sums_on_grid), on the CPU.
//   1. The plan asked AHEAD of an M-step (sums_on_grid, live_floor_on_grid) against the form launch() then yields, over the fact space: where
//      neither a record build nor a cut of the exponents is pending, "grid" <=> form 2 or 3 - never "grid" where form 1 sums in float64; a
//      pending build or cut may still leave nothing (that M-step rebuilds the codes), and behind it the answer is exact again.
//   2. The floor's proof by brute force, through the very conversion the kernels run (fixed_point.h: fixed_of): every float32 posterior in
//      [2^-27, 2^-25] x keep in {1, nextbelow(1), 0.75, 0.5, 1e-4} x shift 0 .. 50; p <= floor must give the integer 0.  And the floor is not
//      needlessly low: the codes' rule is live <=> p >= 2^-26, and no power of two above 2^-26 would do (2^-25 gives the integer 1 at keep 1,
//      shift 50).  The smallest p whose integer is not 0 there is printed: the exact edge lies between, at about 2^-25.5 (c 2^50 > 1/2).
// Built with -fsanitize=address,undefined and run by tests/test_live_floor_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "kernels.h"
#include "mstep_plan.h"

using namespace dmx::mplan;

static long long failures = 0;
#define CHECK(cond) ((cond) ? (void)0 : (void)(failures++ < 20 && std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond)))

static long long walk_plan()
{
    const int Gs[] = {8, 64, 65};
    const float powers[] = {2.0f, 1.5f, 0.0f};
    const long long dones[] = {0, 3, 4, 5, 8, 16, 64}, aheads[] = {0, 7, 8};
    long long n = 0;
    Facts f{};
    f.rows_total = 4000;
    for (int bits = 0; bits < (1 << 12); bits++) {  // every boolean the forms read, both ways
        const auto bit = [&](int i) { return ((bits >> i) & 1) != 0; };
        f.exact_additions = bit(0), f.has_calls = bit(1), f.attached = bit(2), f.mshard = bit(3), f.sliced = bit(4);
        f.has_call_pairs = bit(5), f.has_item_variant = bit(6), f.has_shift_v = bit(7), f.shift_tried = bit(8);
        f.mt_tried = bit(9), f.incr_heavy = bit(10);
        f.n_mt = bit(11) ? 37 : 0;
        for (int tiles = 0; tiles <= 2; tiles++)
            for (int incr = 0; incr <= 2; incr++)
                for (int G : Gs)
                    for (float power : powers)
                        for (long long done : dones)
                            for (long long ahead : aheads)
                                for (long long expected : {0ll, 8ll}) {
                                    f.mstep_tiles = tiles, f.mstep_incremental = incr, f.G = G, f.power = power, f.msteps_done = done;
                                    f.msteps_ahead = ahead, f.msteps_expected = expected;
                                    n++;
                                    const bool grid = sums_on_grid(f);
                                    const int form = launch(f).form;
                                    if (form != 1) CHECK(grid);  // a fixed-point M-step is always announced: no zero is added for nothing
                                    if (grid) CHECK(fixed_point_possible(f));
                                    if (live_floor_on_grid(f)) CHECK(grid && !f.attached);
                                    CHECK(grid_floor_admitted(launch(f)) == (form != 1));
                                    const bool build_pending = build_due(f);
                                    const bool cut_pending = shifts_wanted(f) && !f.has_shift_v && !f.shift_tried;
                                    if (!build_pending && !cut_pending) {
                                        CHECK(grid == (form != 1));  // settled: never "grid" where launch() then yields form 1
                                        continue;
                                    }
                                    // pending: whatever the build and the cut leave, the facts behind them are settled and answer exactly
                                    for (int left = 0; left < 4; left++) {
                                        Facts g = f;
                                        if (build_pending) g.mt_tried = true, g.n_mt = (left & 1) ? 37 : 0;
                                        if (shifts_wanted(g) && !g.has_shift_v && !g.shift_tried) g.shift_tried = true, g.has_shift_v = (left & 2) != 0;
                                        if (build_pending && g.n_mt > 0 && (left & 2)) g.has_shift_v = true;  // (the build uploads the exponents too)
                                        CHECK(!build_due(g));
                                        CHECK(sums_on_grid(g) == (launch(g).form != 1));
                                    }
                                }
    }
    return n;
}

static unsigned bits_of(float x)
{
    unsigned u;
    std::memcpy(&u, &x, 4);
    return u;
}
static float float_of(unsigned u)
{
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// the contribution as the kernels form it with contribution_power == 2: fl32(fl32(p keep)^2)
static float contribution(float p, float keep)
{
    volatile float t = p * keep;  // (one float32 rounding each, whatever the compiler would like to contract)
    volatile float c = t * t;
    return c;
}

int main()
{
    const long long walked = walk_plan();

    const float floor = dmx::live_floor_fixed(2.0f), edge = dmx::mincr_floor(2.0f);
    CHECK(edge == std::ldexp(1.0f, -26));
    CHECK(floor == std::nextafterf(edge, 0.0f));  // live <=> !(p <= floor) <=> p >= 2^-26: what mincr_differs looks at
    CHECK(dmx::live_floor_fixed(1.5f) == 0.0f && dmx::live_floor_fixed(3.0f) == 0.0f && dmx::live_floor_float64(1.5f) == 0.0f);
    CHECK(dmx::live_floor_float64(2.0f) == std::ldexp(1.0f, -80) && dmx::live_floor_float64(2.0f) < floor);
    CHECK(dmx::KEEP_MAX == 1.0f && dmx::FIXED_SHIFT_MAX == 50);

    const float keeps[5] = {1.0f, std::nextafterf(1.0f, 0.0f), 0.75f, 0.5f, 1e-4f};
    const unsigned lo = bits_of(std::ldexp(1.0f, -27)), hi = bits_of(std::ldexp(1.0f, -25));
    constexpr int THREADS = 8;
    std::vector<long long> bad(THREADS, 0), tried(THREADS, 0);
    std::vector<unsigned> first_nonzero(THREADS, 0xFFFFFFFFu);  // smallest p (bits) with a non-zero integer at keep 1, shift 50
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; t++)
        pool.emplace_back([&, t] {
            for (unsigned u = lo + (unsigned)t; u <= hi; u += THREADS) {
                const float p = float_of(u);
                for (int k = 0; k < 5; k++) {
                    const float c = contribution(p, keeps[k]);
                    unsigned long long any = 0ull;
                    for (int shift = 0; shift <= dmx::FIXED_SHIFT_MAX; shift++) any |= dmx::fixed_of(c, shift);
                    tried[t] += dmx::FIXED_SHIFT_MAX + 1;
                    if (p <= floor && any != 0ull) bad[t]++;
                    if (p == edge && any != 0ull) bad[t]++;  // (2^-26 itself, live by the rule, still adds 0)
                    if (k == 0 && dmx::fixed_of(c, dmx::FIXED_SHIFT_MAX) != 0ull && u < first_nonzero[t]) first_nonzero[t] = u;
                }
            }
        });
    for (auto &th : pool) th.join();
    long long n_bad = 0, n_tried = 0;
    unsigned first = 0xFFFFFFFFu;
    for (int t = 0; t < THREADS; t++) n_bad += bad[t], n_tried += tried[t], first = first < first_nonzero[t] ? first : first_nonzero[t];
    CHECK(n_bad == 0);
    CHECK(n_tried == (long long)(hi - lo + 1) * 5 * 51);
    // not needlessly low: the next power of two fails, and the first failing posterior is less than a factor of two above the floor
    CHECK(dmx::fixed_of(contribution(std::ldexp(1.0f, -25), 1.0f), 50) == 1ull);
    CHECK(first != 0xFFFFFFFFu && float_of(first) > edge && float_of(first) < std::ldexp(1.0f, -25));
    CHECK(dmx::fixed_of(contribution(std::nextafterf(float_of(first), 0.0f), 1.0f), 50) == 0ull);

    std::printf("live floor: %lld plan combinations walked, %lld conversions tried, first non-zero posterior %a (floor %a), %lld failures\n", walked, n_tried,
                (double)float_of(first), (double)floor, failures);
    return failures ? 1 : 0;
}
