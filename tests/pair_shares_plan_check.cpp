// pair_shares_plan_check.cpp -- walks check of demuxalot_amd/csrc/pair_shares_plan.h on the CPU (tests/test_pair_shares_plan_cpu.py
// builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): what dmx_estep_pair_shares refuses.
// First what it borrows - the context and the pools, asplan::check_context_and_pools, met once each with its verdict and ahead of
// everything of the grid; then the grid's own rules in their order: the length below 1, null shares, a bad share with its index, a bad
// weight with its index, and last the length above 64.
#include <cmath>
#include <limits>

#include "pair_shares_plan.h"
#include "plan_check.h"

using namespace dmx::psplan;

// the shared pooled call (plan_check.h) with a grid of shares and its log weights
namespace {  // (Pools is hidden from the library's exports; so is what derives from it)
struct Call : PooledCall<Pools> {
    std::vector<float> grid{0.0f, 0.5f, 1.0f, 0.25f, 0.5f};
    std::vector<float> weights{0.0f, -1.5f, -30.0f, 2.0f, 0.0f};
    Verdict verdict(const Facts &f, bool with_weights = true) const
    {
        return check(f, pools(), (long long)grid.size(), grid.data(), with_weights ? weights.data() : nullptr);
    }
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

    // a valid call: with and without weights, with and without doublets
    EXPECT(ok.verdict(good, true).status == OK && ok.verdict(good, false).status == OK);
    {
        Call c;
        c.with_doublets = 0;
        c.row_ptr = {0, 3, 3, 5, 8};
        EXPECT(c.verdict(good).status == OK && c.verdict(good, false).status == OK);
    }

    // everything the pooled entries refuse of the context and the pools is refused with their verdict, whatever the grid is - good,
    // bad, too long or absent
    {
        std::vector<Call> calls;
        std::vector<Facts> facts;
        std::vector<int> codes;
        borrowed_refusals<Call>(good, G, INVALID, UNSUPPORTED, [&](const Call &c, const Facts &f, int code) {
            calls.push_back(c);
            facts.push_back(f);
            codes.push_back(code);
        });
        for (size_t i = 0; i < calls.size(); i++) {
            const Verdict want = dmx::asplan::check_context_and_pools(facts[i], calls[i].pools());
            EXPECT(want.status == codes[i]);
            EXPECT(same(calls[i].verdict(facts[i], false), want));
            EXPECT(same(calls[i].verdict(facts[i], true), want));
            Call bad = calls[i];
            bad.grid[0] = nan;  // a bad share and a bad weight behind another refusal: the other refusal
            bad.weights[1] = inf;
            EXPECT(same(bad.verdict(facts[i], true), want));
            EXPECT(same(check(facts[i], calls[i].pools(), 0, nullptr, nullptr), want));
            EXPECT(same(check(facts[i], calls[i].pools(), 65, nullptr, nullptr), want));
        }
        const Verdict communicator = check(facts[2], ok.pools(), 5, ok.grid.data(), nullptr);
        EXPECT(communicator.what[0] == 'a' && communicator.what[17] == 'c');  // "a context with a communicator ..."
        const Verdict padded = check(facts[4], ok.pools(), 5, ok.grid.data(), nullptr);
        EXPECT(padded.status == UNSUPPORTED && padded.what[4] == 'g');  // "the genotype table is in a padded exchange layout"
    }
    // more than 1024 options in a pool: 44 donors with doublets are the most, the count goes in front of the text
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
        const Verdict verdict = check(f, p, 1, grid.data(), w.data());
        EXPECT(verdict.status == (options <= 1024 ? OK : UNSUPPORTED));
        if (options > 1024) EXPECT(verdict.value == options && verdict.at == 0);
    }

    // the grid's length below 1: before the shares are looked at (they are null here)
    for (const long long n : {0LL, -1LL, (long long)std::numeric_limits<int32_t>::min()}) {
        const Verdict verdict = check(good, ok.pools(), n, nullptr, ok.weights.data());
        EXPECT(verdict.status == INVALID && verdict.at == n && verdict.what[4] == 'g');
        EXPECT(check(good, ok.pools(), n, ok.grid.data(), nullptr).status == INVALID);
    }
    // null shares: INVALID at every length, the ones above 64 included - what is invalid comes before what is unsupported
    for (const long long n : {1LL, 5LL, 64LL, 65LL, 1000LL, (long long)std::numeric_limits<int32_t>::max()}) {
        const Verdict verdict = check(good, ok.pools(), n, nullptr, nullptr);
        EXPECT(verdict.status == INVALID && verdict.what[0] == 'n');
    }
    // the lengths: 1 .. 64 are in, 65 and more are UNSUPPORTED when every value is in order
    for (const size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)66, (size_t)1000}) {
        Call c;
        c.grid.assign(n, 0.5f);
        c.weights.assign(n, -1.0f);
        for (const bool with_weights : {false, true}) {
            const Verdict verdict = c.verdict(good, with_weights);
            EXPECT(verdict.status == (n <= 64 ? OK : UNSUPPORTED));
            if (n > 64) EXPECT(verdict.at == (long long)n && verdict.what[23] == 'm');  // "... has more than 64 values"
        }
        if (n > 64) {  // a bad value in a grid that is too long: the bad value, with its index
            c.grid[n - 1] = 2.0f;
            Verdict verdict = c.verdict(good);
            EXPECT(verdict.status == INVALID && verdict.at == (long long)n - 1);
            c.grid[n - 1] = 0.5f;
            c.weights[64] = nan;
            verdict = c.verdict(good);
            EXPECT(verdict.status == INVALID && verdict.at == 64 && verdict.what[2] == 'l');
            EXPECT(c.verdict(good, false).status == UNSUPPORTED);
        }
    }

    // the shares' values: everything in [0, 1] is in - both ends, zero of both signs, the smallest positive, the value below 1 - at
    // every place of a grid of every length, duplicates and any order among them
    for (const float fine : {0.0f, -0.0f, 1.0f, 0.5f, tiny, std::nextafter(1.0f, 0.0f), 0.1f})
        for (const size_t n : {(size_t)1, (size_t)2, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.3f);
                c.weights.assign(n, -2.0f);
                c.grid[at] = fine;
                EXPECT(c.verdict(good).status == OK && c.verdict(good, false).status == OK);
            }
    // ... and nothing else, with the index of the first one; a bad share comes before a bad weight
    for (const float bad : {nan, -nan, inf, -inf, -tiny, std::nextafter(1.0f, 2.0f), -0.5f, 1.5f, largest})
        for (const size_t n : {(size_t)1, (size_t)2, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.3f);
                c.weights.assign(n, 0.0f);
                c.grid[at] = bad;
                Verdict verdict = c.verdict(good);
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at && verdict.what[2] == 's');
                EXPECT(same(c.verdict(good, false), verdict));
                c.weights[0] = nan;
                EXPECT(same(c.verdict(good), verdict));
                if (at > 0) {  // two bad values: the first one is reported
                    c.grid[0] = bad;
                    EXPECT(c.verdict(good).at == 0);
                }
            }

    // the weights' values: every finite value is in - both signs, zero of both signs, the largest, the smallest
    for (const float fine : {0.0f, -0.0f, 1.0f, -1.0f, largest, -largest, tiny, -tiny, -103.0f, 88.0f})
        for (const size_t n : {(size_t)1, (size_t)2, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.5f);
                c.weights.assign(n, -2.0f);
                c.weights[at] = fine;
                EXPECT(c.verdict(good).status == OK);
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
                EXPECT(c.verdict(good, false).status == OK);  // (not supplied: not read)
                if (at > 0) {
                    c.weights[0] = bad;
                    EXPECT(c.verdict(good).at == 0);
                }
            }
    // exactly n_shares values are read: a bad value behind the grid's end is nobody's
    {
        Call c;
        c.weights.push_back(nan);
        c.grid.push_back(7.0f);
        EXPECT(check(good, c.pools(), 5, c.grid.data(), c.weights.data()).status == OK);
        EXPECT(check(good, c.pools(), 6, c.grid.data(), c.weights.data()).status == INVALID);
    }
    // nobody in a pool, no barcodes: the grid is checked all the same
    {
        const std::vector<int64_t> zero{0};
        const std::vector<int32_t> none(4, -1);
        const std::vector<int64_t> zeros(5, 0);
        const Pools empty{1, 0, zero.data(), nullptr, nullptr, none.data(), zeros.data()};
        const std::vector<float> grid{0.5f}, off{1.5f}, fine{-3.0f}, bad{-inf};
        EXPECT(check(good, empty, 1, grid.data(), fine.data()).status == OK);
        EXPECT(check(good, empty, 1, grid.data(), bad.data()).status == INVALID);
        EXPECT(check(good, empty, 1, off.data(), fine.data()).status == INVALID);
        Facts nobody = good;
        nobody.B = 0;
        Pools p = ok.pools();
        p.pool_of_barcode = nullptr;
        p.row_ptr = zero.data();
        EXPECT(check(nobody, p, 1, grid.data(), fine.data()).status == OK);
        EXPECT(check(nobody, p, 1, grid.data(), bad.data()).status == INVALID);
        EXPECT(check(nobody, p, 1, off.data(), nullptr).status == INVALID);
        EXPECT(check(nobody, p, 1, grid.data(), nullptr).status == OK);
    }

    return finish("pair shares plan");
}
