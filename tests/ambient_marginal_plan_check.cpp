// ambient_marginal_plan_check.cpp -- walks check_marginal of demuxalot_amd/csrc/ambient_grid_plan.h on the CPU
// (tests/test_ambient_marginal_plan_cpu.py builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain
// program): what dmx_estep_ambient_grid_marginal refuses.  That is check() - tests/ambient_grid_plan_check.cpp walks it in depth; here
// every one of its refusals is met once, to see that it is asked at all, with its code and ahead of the weights - and the rule of the
// log weights: absent or every value finite, read only when everything else is in order, the first bad value reported.
#include <cmath>
#include <limits>

#include "ambient_grid_plan.h"
#include "plan_check.h"

using namespace dmx::agplan;

// the shared pooled call (plan_check.h) with a grid, a profile and the grid's log weights
namespace {  // (Pools is hidden from the library's exports; so is what derives from it)
struct Call : PooledCall<Pools> {
    std::vector<float> grid{0.0f, 0.5f, 1.0f, 0.25f, 0.5f};
    std::vector<float> soup{0.0f, 1.0f, 0.5f};
    std::vector<float> weights{0.0f, -1.5f, -30.0f, 2.0f, 0.0f};
    Verdict verdict(const Facts &f, bool with_soup = false, bool with_weights = true) const
    {
        return check_marginal(f, pools(), (long long)grid.size(), grid.data(), with_soup ? soup.data() : nullptr, with_weights ? weights.data() : nullptr);
    }
    Verdict plain(const Facts &f, bool with_soup = false) const { return check(f, pools(), (long long)grid.size(), grid.data(), with_soup ? soup.data() : nullptr); }
};
}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float largest = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
    const int G = 5;
    const long long B = 4, V = 3;
    const Facts good{true, true, false, 1, true, B, V, G};
    const Call ok;

    // a valid call: with and without weights, with and without a supplied profile, with and without doublets
    for (const bool soup : {false, true})
        for (const bool weights : {false, true}) EXPECT(ok.verdict(good, soup, weights).status == OK);
    {
        Call c;
        c.with_doublets = 0;
        c.row_ptr = {0, 3, 3, 5, 8};
        EXPECT(c.verdict(good).status == OK && c.verdict(good, true, false).status == OK);
    }

    // everything check() refuses is refused with check()'s verdict, whatever the weights are - good, bad or absent
    {
        std::vector<Call> calls;
        std::vector<Facts> facts;
        auto add = [&](const Call &c, const Facts &f) {
            calls.push_back(c);
            facts.push_back(f);
        };
        borrowed_refusals<Call>(good, G, INVALID, UNSUPPORTED, [&](const Call &c, const Facts &f, int) { add(c, f); });
        Call c;  // ... and check()'s own: the grid, the profile
        c.grid[2] = 1.5f;
        add(c, good);
        c = Call();
        c.grid[0] = nan;
        add(c, good);
        c = Call();
        c.soup[1] = -0.5f;
        add(c, good);
        for (size_t i = 0; i < calls.size(); i++) {
            const bool with_soup = i + 1 == calls.size();
            const Verdict want = calls[i].plain(facts[i], with_soup);
            EXPECT(want.status != OK);
            EXPECT(same(calls[i].verdict(facts[i], with_soup, false), want));
            EXPECT(same(calls[i].verdict(facts[i], with_soup, true), want));
            Call bad = calls[i];
            bad.weights[0] = nan;  // a bad weight behind another refusal: the other refusal
            EXPECT(same(bad.verdict(facts[i], with_soup, true), want));
        }
    }
    // the grid's length is refused before a weight is read: null weights, null grid
    for (const long long n : {0LL, -1LL, (long long)std::numeric_limits<int32_t>::min()}) {
        const Verdict verdict = check_marginal(good, ok.pools(), n, nullptr, nullptr, ok.weights.data());
        EXPECT(verdict.status == INVALID && verdict.at == n);
    }
    for (const long long n : {65LL, 1000LL, (long long)std::numeric_limits<int32_t>::max()}) {
        const Verdict verdict = check_marginal(good, ok.pools(), n, nullptr, nullptr, ok.weights.data());
        EXPECT(verdict.status == UNSUPPORTED && verdict.at == n);
    }
    EXPECT(check_marginal(good, ok.pools(), 5, nullptr, nullptr, ok.weights.data()).status == INVALID);  // null alphas
    // more than 1024 options in a pool, with weights
    for (const long long g : {44LL, 45LL}) {
        Facts f = good;
        f.G = 2000;
        f.B = 2;
        std::vector<int32_t> d((size_t)g);
        for (long long i = 0; i < g; i++) d[(size_t)i] = (int32_t)i;
        const long long options = g * (g + 1) / 2;
        const std::vector<int64_t> start{0, g}, rows{0, options, options};
        const std::vector<int32_t> pool_of{0, -1};
        const std::vector<float> pen{0.0f}, grid{0.5f}, w{-1.0f};
        const Pools p{1, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
        EXPECT(check_marginal(f, p, 1, grid.data(), nullptr, w.data()).status == (options <= 1024 ? OK : UNSUPPORTED));
    }

    // the weights' values: every finite value is in - both signs, zero of both signs, the largest, the smallest - at every place of a
    // grid of every length
    for (const float fine : {0.0f, -0.0f, 1.0f, -1.0f, largest, -largest, tiny, -tiny, -103.0f, 88.0f})
        for (const size_t n : {(size_t)1, (size_t)2, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.5f);
                c.weights.assign(n, -2.0f);
                c.weights[at] = fine;
                EXPECT(c.verdict(good).status == OK && c.verdict(good, true).status == OK);
            }
    // ... and nothing else: NaN and the infinities, with the index of the first one
    for (const float bad : {nan, -nan, inf, -inf})
        for (const size_t n : {(size_t)1, (size_t)2, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.5f);
                c.weights.assign(n, 0.0f);
                c.weights[at] = bad;
                const Verdict verdict = c.verdict(good);
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at && verdict.what[2] == 'l');
                EXPECT(c.verdict(good, true).status == INVALID);
                EXPECT(c.verdict(good, false, false).status == OK);  // (not supplied: not read)
                EXPECT(c.plain(good).status == OK);                  // (the max entry's check knows no weights)
                if (at > 0) {  // two bad values: the first one is reported
                    c.weights[0] = bad;
                    EXPECT(c.verdict(good).at == 0);
                }
            }
    // exactly n_alphas weights are read: a bad value behind the grid's end is nobody's
    {
        Call c;
        c.weights.push_back(nan);
        EXPECT(c.verdict(good).status == OK);
        c.grid.resize(1);
        c.weights = {0.0f, inf};
        EXPECT(c.verdict(good).status == OK);
    }
    // nobody in a pool, no barcodes: the weights are checked all the same
    {
        const std::vector<int64_t> zero{0};
        const std::vector<int32_t> none(4, -1);
        const std::vector<int64_t> zeros(5, 0);
        const Pools empty{1, 0, zero.data(), nullptr, nullptr, none.data(), zeros.data()};
        const std::vector<float> grid{0.5f}, fine{-3.0f}, bad{-inf};
        EXPECT(check_marginal(good, empty, 1, grid.data(), nullptr, fine.data()).status == OK);
        EXPECT(check_marginal(good, empty, 1, grid.data(), nullptr, bad.data()).status == INVALID);
        Facts nobody = good;
        nobody.B = 0;
        Pools p = ok.pools();
        p.pool_of_barcode = nullptr;
        p.row_ptr = zero.data();
        EXPECT(check_marginal(nobody, p, 1, grid.data(), nullptr, fine.data()).status == OK);
        EXPECT(check_marginal(nobody, p, 1, grid.data(), nullptr, bad.data()).status == INVALID);
        EXPECT(check_marginal(nobody, p, 1, grid.data(), nullptr, nullptr).status == OK);
    }

    return finish("ambient marginal plan");
}
