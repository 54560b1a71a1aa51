// pools_plan_check.cpp -- walks demuxalot_amd/csrc/pools_plan.h on the CPU (tests/test_pools_plan_cpu.py builds it with
// AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of the pooled entries with its code
// and the index it speaks of, the order of the refusals, the boundaries of the option limit and of an option's 16-bit column, that
// nothing is read of what a call does not have, and the layout of the options, word for word.
#include <cstring>

#include "plan_check.h"
#include "pools_plan.h"

using namespace dmx::pplan;

using Call = PooledCall<Pools>;  // the shared pooled call (plan_check.h), as it is

static bool says(const Verdict &verdict, const char *word) { return std::strstr(verdict.what, word) != nullptr; }
static unsigned option(unsigned d1, unsigned d2) { return d1 | d2 << 16; }

int main()
{
    const int G = 5;
    const long long B = 4;
    const Call ok;

    // a valid call, with and without doublets: no index, no value
    {
        Verdict verdict = check(G, B, ok.pools());
        EXPECT(verdict.status == OK && verdict.at == -1 && verdict.value == -1);
        Call c;
        c.singlets_only();
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == OK && verdict.at == -1 && verdict.value == -1);
    }

    // the arguments themselves
    {
        Call c;
        c.with_doublets = 2;
        EXPECT(check(G, B, c.pools()).status == INVALID && says(check(G, B, c.pools()), "with_doublets"));
        c.with_doublets = -1;
        EXPECT(check(G, B, c.pools()).status == INVALID);
        const Pools base = ok.pools();
        Pools p = base;
        p.n_pools = -1;
        EXPECT(check(G, B, p).status == INVALID && says(check(G, B, p), "n_pools") && check(G, B, p).at == -1);
        p = base;
        p.pool_start = nullptr;
        EXPECT(check(G, B, p).status == INVALID && says(check(G, B, p), "null pool_start"));
        p = base;
        p.row_ptr = nullptr;
        EXPECT(check(G, B, p).status == INVALID && says(check(G, B, p), "row_ptr"));
        p = base;
        p.pool_donors = nullptr;
        EXPECT(check(G, B, p).status == INVALID && says(check(G, B, p), "null pool_donors"));
        p = base;
        p.pair_penalty = nullptr;
        EXPECT(check(G, B, p).status == INVALID && says(check(G, B, p), "pair_penalty"));
        p = base;
        p.pool_of_barcode = nullptr;
        EXPECT(check(G, B, p).status == INVALID && says(check(G, B, p), "null pool_of_barcode"));
        // the order: with_doublets before n_pools before the null pointers
        p = base;
        p.with_doublets = 3;
        p.n_pools = -1;
        p.pool_start = nullptr;
        EXPECT(says(check(G, B, p), "with_doublets"));
        p.with_doublets = 1;
        EXPECT(says(check(G, B, p), "n_pools"));
        // no barcodes: pool_of_barcode is not read; no pools: neither donors nor penalties
        const std::vector<int64_t> zero{0};
        p = base;
        p.pool_of_barcode = nullptr;
        p.row_ptr = zero.data();
        EXPECT(check(G, 0, p).status == OK);
        const std::vector<int32_t> none(4, -1);
        const std::vector<int64_t> zeros(5, 0);
        const Pools empty{1, 0, zero.data(), nullptr, nullptr, none.data(), zeros.data()};
        EXPECT(check(G, B, empty).status == OK);
        const Pools nothing{0, 0, zero.data(), nullptr, nullptr, nullptr, zero.data()};
        EXPECT(check(G, 0, nothing).status == OK);
        std::vector<long long> opt_ptr{7, 7};
        std::vector<unsigned> opts{9};
        std::vector<int> pool_size{3};
        layout(nothing, opt_ptr, opts, pool_size);  // reads nothing, leaves the layout of no pools
        EXPECT(opt_ptr == std::vector<long long>{0} && opts.empty() && pool_size.empty());
        // a barcode of a call without pools can only be in none
        std::vector<int32_t> somebody(4, -1);
        somebody[2] = 0;
        const Pools orphan{1, 0, zero.data(), nullptr, nullptr, somebody.data(), zeros.data()};
        EXPECT(check(G, B, orphan).status == INVALID && check(G, B, orphan).at == 2);
    }

    // the pools
    {
        Call c;
        c.pool_start[0] = 1;
        Verdict verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == -1 && says(verdict, "pool_start[0]"));
        c = Call();
        c.pool_start = {0, 5, 3};  // decreasing behind a pool that is out of order
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == 0 && says(verdict, "ascending"));
        c = Call();
        c.donors = {0, 1, 2, 3, 4};
        c.pool_start = {0, 5, 3};  // the first pool is fine, the second has -2 donors
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == 1 && says(verdict, "decreases"));
        c = Call();
        c.pool_start = {0, 3, 3};  // the second pool is empty
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == 1 && says(verdict, "empty"));
        c = Call();
        c.pool_start = {0, 0, 5};  // the first one is
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == 0 && says(verdict, "empty"));
        for (const int bad : {-1, G, G + 1, 70000}) {
            c = Call();
            c.donors[4] = bad;
            verdict = check(G, B, c.pools());
            EXPECT(verdict.status == INVALID && verdict.at == 1 && says(verdict, "outside") && verdict.value == -1);
            c = Call();
            c.donors[0] = bad;
            verdict = check(G, B, c.pools());
            EXPECT(verdict.status == INVALID && verdict.at == 0 && says(verdict, "outside"));
        }
        c = Call();
        c.donors = {0, 2, 2, 1, 3};  // not strictly ascending
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == 0 && says(verdict, "ascending"));
        c = Call();
        c.donors = {0, 2, 4, 3, 1};
        verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == 1 && says(verdict, "ascending"));
        c = Call();
        c.donors = {2, 0, 4, 1, 3};
        EXPECT(check(G, B, c.pools()).status == INVALID && check(G, B, c.pools()).at == 0);
        c = Call();  // a donor outside the table and out of order: outside is said first
        c.donors = {0, 4, -3, 1, 3};
        EXPECT(says(check(G, B, c.pools()), "outside"));
    }

    // the rows
    {
        Call c;
        c.row_ptr[0] = 1;
        Verdict verdict = check(G, B, c.pools());
        EXPECT(verdict.status == INVALID && verdict.at == -1 && says(verdict, "row_ptr[0]"));
        for (const int bad : {-2, 2, 100}) {
            c = Call();
            c.pool_of[3] = bad;
            verdict = check(G, B, c.pools());
            EXPECT(verdict.status == INVALID && verdict.at == 3 && verdict.what[0] == 'p' && says(verdict, "pool_of_barcode"));
        }
        for (size_t at = 1; at <= 4; at++)
            for (const int by : {-1, 1}) {
                c = Call();
                for (size_t i = at; i <= 4; i++) c.row_ptr[i] += by;  // barcode at - 1 gets one entry more or fewer
                verdict = check(G, B, c.pools());
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at - 1 && says(verdict, "row_ptr"));
            }
        c = Call();  // the rows of a run without doublets under with_doublets = 1, and the reverse
        c.row_ptr = {0, 3, 3, 5, 8};
        EXPECT(check(G, B, c.pools()).status == INVALID && check(G, B, c.pools()).at == 0);
        c = Call();
        c.with_doublets = 0;
        EXPECT(check(G, B, c.pools()).status == INVALID && check(G, B, c.pools()).at == 0);
        c = Call();  // a bad pool and bad rows: the pool is reported
        c.donors[1] = 0;
        c.row_ptr[4] = 99;
        EXPECT(says(check(G, B, c.pools()), "ascending"));
        c = Call();  // a barcode outside the pools and a wrong row ahead of it: the row, they are walked together
        c.pool_of[3] = 7;
        c.row_ptr[1] = 5;
        verdict = check(G, B, c.pools());
        EXPECT(verdict.at == 0 && says(verdict, "row_ptr"));
    }

    // the option limit: 44 donors with doublets are 990 options, 45 are 1035; 1024 without doublets, not 1025
    for (const int doublets : {0, 1})
        for (const long long g : {1LL, 44LL, 45LL, 1024LL, 1025LL}) {
            const long long options = options_of(g, doublets != 0);
            EXPECT(options == (doublets ? g * (g + 1) / 2 : g));
            std::vector<int32_t> d((size_t)g);
            for (long long i = 0; i < g; i++) d[(size_t)i] = (int32_t)i;
            const std::vector<int64_t> start{0, 1, 1 + g}, rows{0, options, options, options + 1};
            std::vector<int32_t> all{0};
            all.insert(all.end(), d.begin(), d.end());
            const std::vector<int32_t> pool_of{1, -1, 0};
            const std::vector<float> pen{0.0f, 0.0f};
            const Pools p{doublets, 2, start.data(), all.data(), pen.data(), pool_of.data(), rows.data()};
            const Verdict verdict = check(2000, 3, p);
            EXPECT(verdict.status == (options <= MAX_OPTIONS ? OK : UNSUPPORTED));
            if (verdict.status != OK) {
                EXPECT(verdict.at == 1 && verdict.value == options && says(verdict, "more than 1024 options"));
            } else {
                EXPECT(verdict.value == -1);
            }
        }
    EXPECT(options_of(44, true) == 990 && options_of(45, true) == 1035 && MAX_OPTIONS == 1024);

    // a column past 16 bits
    {
        const std::vector<int64_t> start{0, 2}, rows{0, 2};
        const std::vector<float> pen{0.0f};
        const std::vector<int32_t> pool_of{0};
        for (const int32_t last : {65535, 65536, 69999}) {
            const std::vector<int32_t> d{7, last};
            const Pools p{0, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
            const Verdict verdict = check(70000, 1, p);
            EXPECT(verdict.status == (last < MAX_COLUMN ? OK : UNSUPPORTED));
            if (verdict.status != OK) EXPECT(verdict.at == 0 && says(verdict, "16 bits"));
            if (verdict.status == OK) {
                std::vector<long long> opt_ptr;
                std::vector<unsigned> opts;
                std::vector<int> pool_size;
                layout(p, opt_ptr, opts, pool_size);
                EXPECT(opts == (std::vector<unsigned>{option(7, 7), option(65535, 65535)}));
            }
        }
    }

    // the layout: singlets in list order, then the pairs i < j, i-major
    {
        std::vector<long long> opt_ptr{5};
        std::vector<unsigned> opts{1, 2, 3};
        std::vector<int> pool_size{9, 9, 9};  // (what an earlier call left is dropped)
        layout(ok.pools(), opt_ptr, opts, pool_size);
        EXPECT(opts == (std::vector<unsigned>{option(0, 0), option(2, 2), option(4, 4), option(0, 2), option(0, 4), option(2, 4), option(1, 1), option(3, 3), option(1, 3)}));
        EXPECT(opts[3] == (0u | 2u << 16) && opts[8] == (1u | 3u << 16));
        EXPECT(opt_ptr == (std::vector<long long>{0, 6, 9}));
        EXPECT(pool_size == (std::vector<int>{3, 2}));
        Call c;
        c.singlets_only();
        layout(c.pools(), opt_ptr, opts, pool_size);
        EXPECT(opts == (std::vector<unsigned>{option(0, 0), option(2, 2), option(4, 4), option(1, 1), option(3, 3)}));
        EXPECT(opt_ptr == (std::vector<long long>{0, 3, 5}));
        EXPECT(pool_size == (std::vector<int>{3, 2}));
        // what check() compares row_ptr with is what layout() makes
        for (const int doublets : {0, 1}) {
            Call k;
            if (!doublets) k.singlets_only();
            layout(k.pools(), opt_ptr, opts, pool_size);
            for (size_t q = 0; q < 2; q++) EXPECT(opt_ptr[q + 1] - opt_ptr[q] == options_of(pool_size[q], doublets != 0));
        }
    }
    {
        // the widest pool with doublets: 44 donors, 990 options, the last one the pair of the last two donors
        std::vector<int32_t> d(44);
        for (int i = 0; i < 44; i++) d[(size_t)i] = i;
        const std::vector<int64_t> start{0, 44}, rows{0, 990};
        const std::vector<float> pen{0.0f};
        const std::vector<int32_t> pool_of{0};
        const Pools p{1, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
        EXPECT(check(44, 1, p).status == OK);
        std::vector<long long> opt_ptr;
        std::vector<unsigned> opts;
        std::vector<int> pool_size;
        layout(p, opt_ptr, opts, pool_size);
        EXPECT(opts.size() == 990 && opt_ptr == (std::vector<long long>{0, 990}) && pool_size == std::vector<int>{44});
        EXPECT(opts.back() == (42u | 43u << 16) && opts[43] == option(43, 43) && opts[44] == option(0, 1) && opts[44 + 43] == option(1, 2));
        bool ordered = true;  // i-major, j ascending: the words of the pairs ascend when read as (i, j)
        for (size_t k = 45; k < opts.size(); k++) {
            const unsigned i0 = opts[k - 1] & 0xFFFFu, j0 = opts[k - 1] >> 16, i1 = opts[k] & 0xFFFFu, j1 = opts[k] >> 16;
            ordered = ordered && i1 < j1 && (i1 > i0 || (i1 == i0 && j1 > j0));
        }
        EXPECT(ordered);
    }

    return finish("pools plan");
}
