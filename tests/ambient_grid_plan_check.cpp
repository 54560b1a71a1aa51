// ambient_grid_plan_check.cpp -- walks demuxalot_amd/csrc/ambient_grid_plan.h on the CPU (tests/test_ambient_grid_cpu.py builds it
// with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of dmx_estep_ambient_grid with
// its code - the grid's own, and that the two ends it borrows (ambient_scoring_plan.h: the contexts, the pools through pools_plan.h's
// check, the supplied profile; tests/ambient_scoring_plan_check.cpp and tests/pools_plan_check.cpp walk those in depth) are asked
// at all and in their place -, the boundaries of the grid's length and values, and the order of the checks.
#include <cmath>
#include <limits>

#include "ambient_grid_plan.h"
#include "plan_check.h"

using namespace dmx::agplan;

// the shared pooled call (plan_check.h) with a grid and a profile
namespace {  // (Pools is hidden from the library's exports; so is what derives from it)
struct Call : PooledCall<Pools> {
    std::vector<float> grid{0.0f, 0.5f, 1.0f, 0.25f, 0.5f};  // any order, duplicates allowed
    std::vector<float> soup{0.0f, 1.0f, 0.5f};
    Verdict verdict(const Facts &f, bool with_soup = false) const { return check(f, pools(), (long long)grid.size(), grid.data(), with_soup ? soup.data() : nullptr); }
};
}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int G = 5;
    const long long B = 4, V = 3;
    const Facts good{true, true, false, 1, true, B, V, G};
    const Call ok;

    // a valid call, with and without a supplied profile, with and without doublets
    EXPECT(ok.verdict(good).status == OK && ok.verdict(good, true).status == OK);
    {
        Call c;
        c.with_doublets = 0;
        c.row_ptr = {0, 3, 3, 5, 8};
        EXPECT(c.verdict(good).status == OK && c.verdict(good, true).status == OK);
    }

    // the borrowed front end: call order, communicator, layout, the pools
    for (int k = 0; k < 3; k++) {
        Facts f = good;
        f.have_problem = k == 1;
        f.have_table = k == 2;
        EXPECT(ok.verdict(f).status == INVALID);
    }
    {
        Facts f = good;
        f.attached = true;
        EXPECT(ok.verdict(f).status == UNSUPPORTED);
        f = good;
        f.nranks = 2;
        EXPECT(ok.verdict(f).status == UNSUPPORTED);
        f = good;
        f.dense_table = false;
        EXPECT(ok.verdict(f).status == UNSUPPORTED);
        f = good;  // a communicator and a bad grid: the communicator is reported
        f.attached = true;
        Call c;
        c.grid[0] = nan;
        EXPECT(c.verdict(f).status == UNSUPPORTED);
        c.grid.clear();
        EXPECT(c.verdict(f).status == UNSUPPORTED);
    }
    {
        Call c;
        c.with_doublets = 2;
        EXPECT(c.verdict(good).status == INVALID);
        c = Call();
        c.pool_start[0] = 1;
        EXPECT(c.verdict(good).status == INVALID);
        c = Call();
        c.pool_start = {0, 3, 3};  // the second pool is empty
        EXPECT(c.verdict(good).status == INVALID && c.verdict(good).at == 1);
        c = Call();
        c.donors = {0, 2, 2, 1, 3};  // not strictly ascending
        EXPECT(c.verdict(good).status == INVALID && c.verdict(good).at == 0);
        c = Call();
        c.donors[4] = G;
        EXPECT(c.verdict(good).status == INVALID && c.verdict(good).at == 1);
        c = Call();
        c.pool_of[3] = 2;
        EXPECT(c.verdict(good).status == INVALID && c.verdict(good).at == 3);
        c = Call();
        c.row_ptr[4] += 1;
        EXPECT(c.verdict(good).status == INVALID && c.verdict(good).at == 3);
        const Pools base = ok.pools();
        Pools p = base;
        p.row_ptr = nullptr;
        EXPECT(check(good, p, 1, ok.grid.data(), nullptr).status == INVALID);
        p = base;
        p.pool_of_barcode = nullptr;
        EXPECT(check(good, p, 1, ok.grid.data(), nullptr).status == INVALID);
        // a bad pool and a bad grid: the pool is reported
        c = Call();
        c.pool_of[0] = 9;
        c.grid[1] = 2.0f;
        const Verdict verdict = c.verdict(good);
        EXPECT(verdict.status == INVALID && verdict.at == 0 && verdict.what[0] == 'p');
    }
    // more than 1024 options in a pool: 44 donors with doublets are 990 options, 45 are 1035; 1024 without doublets, not 1025
    for (const int doublets : {0, 1})
        for (const long long g : {1LL, 44LL, 45LL, 1024LL, 1025LL}) {
            const long long options = doublets ? g * (g + 1) / 2 : g;
            Facts f = good;
            f.G = 2000;
            f.B = 2;
            std::vector<int32_t> d((size_t)g);
            for (long long i = 0; i < g; i++) d[(size_t)i] = (int32_t)i;
            const std::vector<int64_t> start{0, g}, rows{0, options, options};
            const std::vector<int32_t> pool_of{0, -1};
            const std::vector<float> pen{0.0f}, grid{0.5f};
            const Pools p{doublets, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
            const Verdict verdict = check(f, p, 1, grid.data(), nullptr);
            EXPECT(verdict.status == (options <= 1024 ? OK : UNSUPPORTED));
            if (verdict.status != OK) EXPECT(verdict.at == 0 && verdict.value == options);
        }

    // the grid's length: 1 .. 64; nothing is read of a grid whose length is refused
    {
        const std::vector<float> grid(65, 0.25f);
        for (const long long n : {1LL, 2LL, 63LL, 64LL}) EXPECT(check(good, ok.pools(), n, grid.data(), nullptr).status == OK);
        for (const long long n : {0LL, -1LL, -64LL, (long long)std::numeric_limits<int32_t>::min()}) {
            const Verdict verdict = check(good, ok.pools(), n, nullptr, nullptr);
            EXPECT(verdict.status == INVALID && verdict.at == n);
        }
        for (const long long n : {65LL, 66LL, 1000LL, (long long)std::numeric_limits<int32_t>::max()}) {
            const Verdict verdict = check(good, ok.pools(), n, nullptr, nullptr);
            EXPECT(verdict.status == UNSUPPORTED && verdict.at == n);
        }
        EXPECT(check(good, ok.pools(), 1, nullptr, nullptr).status == INVALID);   // null alphas
        EXPECT(check(good, ok.pools(), 64, nullptr, nullptr).status == INVALID);
        EXPECT(check(good, ok.pools(), 64, nullptr, ok.soup.data()).status == INVALID);
    }
    // the grid's values: the ends of [0, 1] are in, everything else is out, at every place of a grid of every length
    for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), std::numeric_limits<float>::denorm_min()})
        for (const size_t n : {(size_t)1, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.5f);
                c.grid[at] = fine;
                EXPECT(c.verdict(good).status == OK);
            }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -std::numeric_limits<float>::denorm_min(), 2.0f, -1.0f})
        for (const size_t n : {(size_t)1, (size_t)5, (size_t)64})
            for (const size_t at : {(size_t)0, n / 2, n - 1}) {
                Call c;
                c.grid.assign(n, 0.5f);
                c.grid[at] = bad;
                const Verdict verdict = c.verdict(good);
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at && verdict.what[2] == 'g');
                if (n > 1 && at > 0) {  // two bad values: the first one is reported
                    c.grid[0] = bad;
                    EXPECT(c.verdict(good).at == 0);
                }
            }
    {
        Call c;  // all values equal, all zero, descending: all fine
        c.grid.assign(64, 0.0f);
        EXPECT(c.verdict(good).status == OK);
        for (size_t j = 0; j < 64; j++) c.grid[j] = (float)(63 - j) / 63.0f;
        EXPECT(c.verdict(good).status == OK);
    }
    // nobody in a pool, no barcodes: the grid is checked all the same
    {
        const std::vector<int64_t> zero{0};
        const std::vector<int32_t> none(4, -1);
        const std::vector<int64_t> zeros(5, 0);
        const Pools empty{1, 0, zero.data(), nullptr, nullptr, none.data(), zeros.data()};
        const std::vector<float> fine{0.5f}, bad{1.5f};
        EXPECT(check(good, empty, 1, fine.data(), nullptr).status == OK);
        EXPECT(check(good, empty, 1, bad.data(), nullptr).status == INVALID);
        Facts nobody = good;
        nobody.B = 0;
        Pools p = ok.pools();
        p.pool_of_barcode = nullptr;
        p.row_ptr = zero.data();
        EXPECT(check(nobody, p, 1, fine.data(), nullptr).status == OK);
        EXPECT(check(nobody, p, 0, fine.data(), nullptr).status == INVALID);
    }

    // ambient values, behind the grid
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -1e-30f, 2.0f})
        for (long long at = 0; at < V; at++) {
            Call c;
            c.soup[(size_t)at] = bad;
            const Verdict verdict = c.verdict(good, true);
            EXPECT(verdict.status == INVALID && verdict.at == at && verdict.what[0] == 'a');
            EXPECT(c.verdict(good, false).status == OK);  // (not supplied: not read)
            c.grid[3] = bad;  // a bad grid value and a bad profile: the grid
            const Verdict first = c.verdict(good, true);
            EXPECT(first.status == INVALID && first.at == 3 && first.what[2] == 'g');
        }

    return finish("ambient grid plan");
}
