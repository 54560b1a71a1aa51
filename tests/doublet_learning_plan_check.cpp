// doublet_learning_plan_check.cpp -- walks demuxalot_amd/csrc/doublet_learning_plan.h on the CPU (tests/test_doublet_learning_plan_cpu.py
// builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of dmx_em_doublets and
// dmx_mstep_doublets with its code - the iteration count, the contribution power, the threshold, the contexts the calls do not run on,
// what the pooled entries refuse of the pools (pplan::check, composed here; tests/pools_plan_check.cpp walks it on its own), the length
// and the values of the posterior rows -, the boundaries, the order of the checks, and the bound of the list's length.
#include <cmath>
#include <limits>

#include "doublet_learning_plan.h"
#include "plan_check.h"

using namespace dmx::dlplan;

// the shared pooled call (plan_check.h) with the posterior rows of its 15 options
namespace {  // (Pools is hidden from the library's exports; so is what derives from it)
struct Call : PooledCall<Pools> {
    std::vector<float> rows = std::vector<float>(15, 0.125f);
};
}  // namespace

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float tiny = std::numeric_limits<float>::denorm_min(), huge = std::numeric_limits<float>::max();
    const int G = 5;
    const long long B = 4, V = 3;
    const Facts good{true, true, false, 1, true, B, V, G};
    const Call ok;
    auto em = [&](const Facts &f, const Call &c, int n, float power, float threshold) { return check_em(f, c.pools(), n, power, threshold); };
    auto mstep = [&](const Facts &f, const Call &c, bool have_post, float power, float threshold) {
        return check_mstep(f, have_post, c.pools(), power, threshold, (long long)c.rows.size(), c.rows.data());
    };

    // valid calls: one iteration and many, the reference's power and others, thresholds from the smallest float to the largest
    for (const int n : {1, 2, 5, 1000000})
        for (const float power : {2.0f, 1.5f, 1.0f, tiny, huge, 0.25f})
            for (const float threshold : {1e-3f, 1e-6f, tiny, 1.0f, std::nextafter(1.0f, 2.0f), 2.0f, huge}) {
                EXPECT(em(good, ok, n, power, threshold).status == OK);
                EXPECT(mstep(good, ok, true, power, threshold).status == OK);
            }

    // the iteration count
    for (const int n : {0, -1, std::numeric_limits<int>::min()}) {
        const Verdict verdict = em(good, ok, n, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.what[0] == 'n' && verdict.at == -1);
    }

    // the power and the threshold: finite and above 0
    EXPECT(threshold_valid(1e-3f) && threshold_valid(tiny) && threshold_valid(huge) && !threshold_valid(0.0f) && !threshold_valid(-0.0f));
    for (const float bad : {0.0f, -0.0f, -tiny, -2.0f, nan, inf, -inf}) {
        EXPECT(!power_valid(bad) && !threshold_valid(bad));
        EXPECT(em(good, ok, 3, bad, 1e-3f).status == INVALID && em(good, ok, 3, bad, 1e-3f).what[0] == 't');
        EXPECT(mstep(good, ok, true, bad, 1e-3f).status == INVALID);
        EXPECT(em(good, ok, 3, 2.0f, bad).status == INVALID && em(good, ok, 3, 2.0f, bad).what[0] == 'm');
        EXPECT(mstep(good, ok, true, 2.0f, bad).status == INVALID && mstep(good, ok, true, 2.0f, bad).what[0] == 'm');
    }
    EXPECT(em(good, ok, 0, nan, nan).what[0] == 'n' && em(good, ok, 1, nan, nan).what[0] == 't');  // the order: count, power, threshold

    // call order: the M-step names what is missing, the problem first, then the table, then the posteriors
    {
        Facts f = good;
        f.have_problem = false;
        f.have_table = false;
        Verdict verdict = mstep(f, ok, false, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.what[14] == 'p');  // "call order: a problem ..."
        f.have_problem = true;
        verdict = mstep(f, ok, false, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.what[12] == 'g');  // "call order: genotype probabilities ..."
        f.have_table = true;
        verdict = mstep(f, ok, false, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.what[15] == 'E');  // "call order: an E-step ..."
        EXPECT(mstep(f, ok, true, 2.0f, 1e-3f).status == OK);
        for (int k = 0; k < 3; k++) {  // the loop: a problem and the prior betas
            Facts g = good;
            g.have_problem = k == 1;
            g.have_table = k == 2;
            EXPECT(em(g, ok, 3, 2.0f, 1e-3f).status == INVALID);
        }
    }

    // a communicator, several ranks, a padded table: UNSUPPORTED, behind the call order and the call's own numbers, ahead of the pools
    for (int k = 0; k < 3; k++) {
        Facts f = good;
        f.attached = k == 0;
        f.nranks = k == 1 ? 2 : 1;
        f.dense_table = k != 2;
        EXPECT(em(f, ok, 3, 2.0f, 1e-3f).status == UNSUPPORTED);
        EXPECT(mstep(f, ok, true, 2.0f, 1e-3f).status == UNSUPPORTED);
        Call c;
        c.donors = {0, 2, 2, 1, 3};
        c.rows[0] = nan;
        EXPECT(em(f, c, 3, 2.0f, 1e-3f).status == UNSUPPORTED);
        EXPECT(mstep(f, c, true, 2.0f, 1e-3f).status == UNSUPPORTED);
        EXPECT(em(f, ok, 0, 2.0f, 1e-3f).status == INVALID && em(f, ok, 3, 0.0f, 1e-3f).status == INVALID && em(f, ok, 3, 2.0f, 0.0f).status == INVALID);
        EXPECT(mstep(f, ok, true, 0.0f, 1e-3f).status == INVALID && mstep(f, ok, true, 2.0f, nan).status == INVALID);
        EXPECT(mstep(f, ok, false, 2.0f, 1e-3f).status == INVALID);
        f.have_table = false;
        EXPECT(em(f, ok, 3, 2.0f, 1e-3f).status == INVALID);
        EXPECT(mstep(f, ok, true, 2.0f, 1e-3f).status == INVALID);
    }

    // the pools, as the pooled entries refuse them
    {
        Call c;
        c.with_doublets = 2;
        EXPECT(em(good, c, 3, 2.0f, 1e-3f).status == INVALID && mstep(good, c, true, 2.0f, 1e-3f).status == INVALID);
        c = Call();
        c.donors = {0, 2, 2, 1, 3};
        Verdict verdict = em(good, c, 3, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.at == 0);
        verdict = mstep(good, c, true, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.at == 0);
        c = Call();
        c.donors[4] = 5;  // outside [0, G)
        EXPECT(em(good, c, 3, 2.0f, 1e-3f).status == INVALID && em(good, c, 3, 2.0f, 1e-3f).at == 1);
        c = Call();
        c.pool_of[3] = 2;
        verdict = em(good, c, 3, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.at == 3);
        EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == INVALID && mstep(good, c, true, 2.0f, 1e-3f).at == 3);
        c = Call();
        c.row_ptr[4] = 14;
        verdict = em(good, c, 3, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.at == 3);
        Facts wide = good;
        wide.G = 2000;
        wide.B = 1;
        std::vector<int32_t> d(45);
        for (int i = 0; i < 45; i++) d[(size_t)i] = i;
        const std::vector<int64_t> start{0, 45}, rows{0, 1035};
        const std::vector<int32_t> pool_of{0};
        const std::vector<float> pen{0.0f}, post(1035, 0.0f);
        const Pools p{1, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
        verdict = check_em(wide, p, 3, 2.0f, 1e-3f);
        EXPECT(verdict.status == UNSUPPORTED && verdict.value == 1035);
        EXPECT(check_mstep(wide, true, p, 2.0f, 1e-3f, 1035, post.data()).status == UNSUPPORTED);
        d.pop_back();  // 44 donors: 990 options, the most a pool holds with doublets
        const std::vector<int64_t> start44{0, 44}, rows44{0, 990};
        const Pools q{1, 1, start44.data(), d.data(), pen.data(), pool_of.data(), rows44.data()};
        EXPECT(check_em(wide, q, 3, 2.0f, 1e-3f).status == OK && check_mstep(wide, true, q, 2.0f, 1e-3f, 990, post.data()).status == OK);
        EXPECT(pair_options(1, q) == 990 - 44);
    }

    // the rows: their length is row_ptr[B]; no null rows of a length; every value finite and in [0, 1]
    {
        const Pools p = ok.pools();
        for (const long long n : {0ll, 14ll, 16ll, -1ll}) {
            const Verdict verdict = check_mstep(good, true, p, 2.0f, 1e-3f, n, ok.rows.data());
            EXPECT(verdict.status == INVALID && verdict.what[0] == 't' && verdict.at == -1);
        }
        EXPECT(check_mstep(good, true, p, 2.0f, 1e-3f, 15, nullptr).status == INVALID);
        Call nobody;  // every barcode in no pool: no rows, and null is theirs
        nobody.pool_of = {-1, -1, -1, -1};
        nobody.row_ptr = {0, 0, 0, 0, 0};
        EXPECT(check_mstep(good, true, nobody.pools(), 2.0f, 1e-3f, 0, nullptr).status == OK);
        EXPECT(pair_options(B, nobody.pools()) == 0);
        Facts none = good;
        none.B = 0;
        const std::vector<int64_t> empty_rows{0};
        const Pools e{1, 2, ok.pool_start.data(), ok.donors.data(), ok.penalty.data(), nullptr, empty_rows.data()};
        EXPECT(check_mstep(none, true, e, 2.0f, 1e-3f, 0, nullptr).status == OK && check_em(none, e, 1, 2.0f, 1e-3f).status == OK);
        EXPECT(pair_options(0, e) == 0);
    }
    for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), tiny})
        for (size_t at = 0; at < 15; at++) {
            Call c;
            c.rows[at] = fine;
            EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == OK);
        }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -tiny, 2.0f, -1.0f})
        for (size_t at = 0; at < 15; at++) {
            Call c;
            c.rows[at] = bad;
            const Verdict verdict = mstep(good, c, true, 2.0f, 1e-3f);
            EXPECT(verdict.status == INVALID && verdict.at == (long long)at && verdict.what[2] == 'p');  // "a posterior ..."
        }
    {
        Call c;  // bad pools and a bad row: the pools; a bad threshold and bad pools: the threshold
        c.rows[3] = nan;
        c.pool_of[0] = 7;
        EXPECT(mstep(good, c, true, 2.0f, 1e-3f).at == 0 && mstep(good, c, true, 2.0f, 1e-3f).what[0] == 'p');
        EXPECT(mstep(good, c, true, 2.0f, 0.0f).what[0] == 'm');
    }

    // the bound of the list: the pair options of the pooled barcodes
    EXPECT(pair_options(B, ok.pools()) == 3 + 0 + 1 + 3);
    {
        Call c;
        c.with_doublets = 0;
        c.row_ptr = {0, 3, 3, 5, 8};
        c.rows.assign(8, 0.5f);
        EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == OK && em(good, c, 2, 2.0f, 1e-3f).status == OK);
        EXPECT(pair_options(B, c.pools()) == 0);
    }

    return finish("doublet learning plan");
}
