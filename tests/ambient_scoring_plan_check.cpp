// ambient_scoring_plan_check.cpp -- walks demuxalot_amd/csrc/ambient_scoring_plan.h on the CPU (tests/test_ambient_scoring_cpu.py
// builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of dmx_estep_ambient
// with its code - the contexts the pass does not run on, everything dmx_estep_pools refuses (pools_plan.h's check, composed here;
// tests/pools_plan_check.cpp walks it on its own), the fractions, the profile -, the boundaries of the option limit, the order of
// the checks, and that nothing is read of a barcode in no pool.
#include <cmath>
#include <limits>

#include "ambient_scoring_plan.h"
#include "plan_check.h"

using namespace dmx::asplan;

// the shared pooled call (plan_check.h) with the barcodes' fractions and a profile
namespace {  // (Pools is hidden from the library's exports; so is what derives from it)
struct Call : PooledCall<Pools> {
    std::vector<float> alpha{0.0f, 0.5f, 1.0f, 0.25f};
    std::vector<float> soup{0.0f, 1.0f, 0.5f};
};
}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int G = 5;
    const long long B = 4, V = 3;
    const Facts good{true, true, false, 1, true, B, V, G};
    const Call ok;
    auto status = [&](const Facts &f, const Call &c, bool with_soup = false) { return check(f, c.pools(), c.alpha.data(), with_soup ? c.soup.data() : nullptr).status; };

    // a valid call, with and without a supplied profile, with and without doublets
    EXPECT(status(good, ok) == OK && status(good, ok, true) == OK);
    {
        Call c;
        c.singlets_only();
        EXPECT(status(good, c) == OK && status(good, c, true) == OK);
    }

    // call order, communicator, layout; the call order is reported first
    for (int k = 0; k < 3; k++) {
        Facts f = good;
        f.have_problem = k == 1;
        f.have_table = k == 2;
        EXPECT(status(f, ok) == INVALID);
    }
    {
        Facts f = good;
        f.attached = true;
        EXPECT(status(f, ok) == UNSUPPORTED);
        f = good;
        f.nranks = 2;
        EXPECT(status(f, ok) == UNSUPPORTED);
        f = good;
        f.dense_table = false;
        EXPECT(status(f, ok) == UNSUPPORTED);
        f = good;
        f.attached = true;
        f.have_table = false;
        EXPECT(status(f, ok) == INVALID);
        f = good;  // a communicator and a bad argument: the communicator is reported
        f.attached = true;
        Call c;
        c.alpha[0] = nan;
        EXPECT(status(f, c) == UNSUPPORTED);
    }

    // what dmx_estep_pools refuses
    {
        Call c;
        c.with_doublets = 2;
        EXPECT(status(good, c) == INVALID);
        c.with_doublets = -1;
        EXPECT(status(good, c) == INVALID);
        const Pools base = ok.pools();
        Pools p = base;
        p.n_pools = -1;
        EXPECT(check(good, p, ok.alpha.data(), nullptr).status == INVALID);
        p = base;
        p.pool_start = nullptr;
        EXPECT(check(good, p, ok.alpha.data(), nullptr).status == INVALID);
        p = base;
        p.row_ptr = nullptr;
        EXPECT(check(good, p, ok.alpha.data(), nullptr).status == INVALID);
        p = base;
        p.pool_donors = nullptr;
        EXPECT(check(good, p, ok.alpha.data(), nullptr).status == INVALID);
        p = base;
        p.pair_penalty = nullptr;
        EXPECT(check(good, p, ok.alpha.data(), nullptr).status == INVALID);
        p = base;
        p.pool_of_barcode = nullptr;
        EXPECT(check(good, p, ok.alpha.data(), nullptr).status == INVALID);
        EXPECT(check(good, base, nullptr, nullptr).status == INVALID);  // null alpha with B > 0
        // no barcodes: neither pool_of_barcode nor alpha is read; no pools: neither donors nor penalties
        Facts nobody = good;
        nobody.B = 0;
        const std::vector<int64_t> zero{0};
        p = base;
        p.pool_of_barcode = nullptr;
        p.row_ptr = zero.data();
        EXPECT(check(nobody, p, nullptr, nullptr).status == OK);
        const std::vector<int32_t> none(4, -1);
        const std::vector<int64_t> zeros(5, 0);
        const Pools empty{1, 0, zero.data(), nullptr, nullptr, none.data(), zeros.data()};
        EXPECT(check(good, empty, ok.alpha.data(), nullptr).status == OK);
        const std::vector<float> wild(4, nan);  // (nobody is in a pool: no fraction is looked at)
        EXPECT(check(good, empty, wild.data(), nullptr).status == OK);
    }
    {
        Call c;
        c.pool_start[0] = 1;
        EXPECT(status(good, c) == INVALID);
        c = Call();
        c.pool_start = {0, 5, 3};  // decreasing
        Verdict verdict = check(good, c.pools(), c.alpha.data(), nullptr);
        EXPECT(verdict.status == INVALID);
        c = Call();
        c.pool_start = {0, 3, 3};  // the second pool is empty
        verdict = check(good, c.pools(), c.alpha.data(), nullptr);
        EXPECT(verdict.status == INVALID && verdict.at == 1);
        for (const int bad : {-1, G, G + 1, 70000}) {
            c = Call();
            c.donors[4] = bad;
            verdict = check(good, c.pools(), c.alpha.data(), nullptr);
            EXPECT(verdict.status == INVALID && verdict.at == 1);
        }
        c = Call();
        c.donors = {0, 2, 2, 1, 3};  // not strictly ascending
        verdict = check(good, c.pools(), c.alpha.data(), nullptr);
        EXPECT(verdict.status == INVALID && verdict.at == 0);
        c = Call();
        c.donors = {2, 0, 4, 1, 3};
        EXPECT(status(good, c) == INVALID);
        c = Call();
        c.row_ptr[0] = 1;
        EXPECT(status(good, c) == INVALID);
        for (const int bad : {-2, 2, 100}) {
            c = Call();
            c.pool_of[3] = bad;
            verdict = check(good, c.pools(), c.alpha.data(), nullptr);
            EXPECT(verdict.status == INVALID && verdict.at == 3);
        }
        for (size_t at = 1; at <= 4; at++)
            for (const int by : {-1, 1}) {
                c = Call();
                for (size_t i = at; i <= 4; i++) c.row_ptr[i] += by;  // barcode at - 1 gets one entry more or fewer
                verdict = check(good, c.pools(), c.alpha.data(), nullptr);
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at - 1);
            }
        c = Call();  // the rows of a run without doublets under with_doublets = 1
        c.row_ptr = {0, 3, 3, 5, 8};
        EXPECT(status(good, c) == INVALID);
    }

    // the option limit: 44 donors with doublets are 990 options, 45 are 1035; 1024 without doublets, not 1025; a column past 16 bits
    for (const int doublets : {0, 1})
        for (const long long g : {1LL, 44LL, 45LL, 1024LL, 1025LL}) {
            const long long options = options_of(g, doublets != 0);
            EXPECT(options == (doublets ? g * (g + 1) / 2 : g));
            Facts f = good;
            f.G = 2000;
            f.B = 2;
            std::vector<int32_t> d((size_t)g);
            for (long long i = 0; i < g; i++) d[(size_t)i] = (int32_t)i;
            const std::vector<int64_t> start{0, g}, rows{0, options, options};
            const std::vector<int32_t> pool_of{0, -1};
            const std::vector<float> pen{0.0f}, al{0.5f, nan};
            const Pools p{doublets, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
            const Verdict verdict = check(f, p, al.data(), nullptr);
            EXPECT(verdict.status == (options <= 1024 ? OK : UNSUPPORTED));
            if (verdict.status != OK) EXPECT(verdict.at == 0);
        }
    {
        Facts f = good;
        f.G = 70000;
        f.B = 1;
        const std::vector<int64_t> start{0, 2}, rows{0, 2};
        const std::vector<float> pen{0.0f}, al{0.5f};
        const std::vector<int32_t> pool_of{0};
        for (const int32_t last : {65535, 65536, 69999}) {
            const std::vector<int32_t> d{7, last};
            const Pools p{0, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
            EXPECT(check(f, p, al.data(), nullptr).status == (last < 65536 ? OK : UNSUPPORTED));
        }
    }

    // fractions: the ends of [0, 1] are in, everything else is out - for every pooled barcode; the barcode in no pool is not looked at
    for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), std::numeric_limits<float>::denorm_min()})
        for (size_t at = 0; at < 4; at++) {
            Call c;
            c.alpha[at] = fine;
            EXPECT(status(good, c) == OK);
        }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -std::numeric_limits<float>::denorm_min(), 2.0f, -1.0f})
        for (size_t at = 0; at < 4; at++) {
            Call c;
            c.alpha[at] = bad;
            const Verdict verdict = check(good, c.pools(), c.alpha.data(), nullptr);
            if (c.pool_of[at] < 0) {
                EXPECT(verdict.status == OK);
            } else {
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at);
            }
            c.singlets_only();
            EXPECT(status(good, c) == (c.pool_of[at] < 0 ? OK : INVALID));
        }

    // ambient values
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -1e-30f, 2.0f})
        for (long long at = 0; at < V; at++) {
            Call c;
            c.soup[(size_t)at] = bad;
            const Verdict verdict = check(good, c.pools(), c.alpha.data(), c.soup.data());
            EXPECT(verdict.status == INVALID && verdict.at == at);
            EXPECT(status(good, c, false) == OK);  // (not supplied: not read)
        }
    {
        Call c;  // a bad pool and a bad fraction: the pool is reported (the fractions of an unvalidated pool_of_barcode are not read)
        c.pool_of[0] = 9;
        c.alpha[0] = nan;
        const Verdict verdict = check(good, c.pools(), c.alpha.data(), nullptr);
        EXPECT(verdict.status == INVALID && verdict.at == 0 && verdict.what[0] == 'p');
        c = Call();  // a bad fraction and a bad profile: the fraction
        c.alpha[3] = 2.0f;
        c.soup[0] = nan;
        const Verdict second = check(good, c.pools(), c.alpha.data(), c.soup.data());
        EXPECT(second.status == INVALID && second.at == 3 && second.what[0] == 'a' && second.what[1] == 'l');
    }

    return finish("ambient scoring plan");
}
