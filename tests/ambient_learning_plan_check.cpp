// ambient_learning_plan_check.cpp -- walks demuxalot_amd/csrc/ambient_learning_plan.h on the CPU (tests/test_ambient_learning_plan_cpu.py
// builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of dmx_em_ambient and
// dmx_mstep_ambient with its code - the iteration count, the contribution power, the contexts the calls do not run on, what
// dmx_estep_ambient refuses (asplan::check, composed here; tests/ambient_scoring_plan_check.cpp walks it on its own), the fractions, the
// profile -, the boundaries, the order of the checks, and whose fraction is read.
#include <cmath>
#include <limits>

#include "ambient_learning_plan.h"
#include "plan_check.h"

using namespace dmx::alplan;

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
    const float tiny = std::numeric_limits<float>::denorm_min(), huge = std::numeric_limits<float>::max();
    const int G = 5;
    const long long B = 4, V = 3;
    const Facts good{true, true, false, 1, true, B, V, G};
    const Call ok;
    auto em = [&](const Facts &f, const Call &c, int n, float power, bool with_soup = false) {
        return check_em(f, c.pools(), n, power, c.alpha.data(), with_soup ? c.soup.data() : nullptr);
    };
    auto mstep = [&](const Facts &f, const Call &c, bool have_post, float power, bool with_soup = false) {
        return check_mstep(f, have_post, power, c.alpha.data(), with_soup ? c.soup.data() : nullptr);
    };

    // valid calls: one iteration and many, the reference's power and others, with and without a supplied profile
    for (const int n : {1, 2, 5, 1000000})
        for (const float power : {2.0f, 1.5f, 1.0f, tiny, huge, 0.25f})
            for (const bool with_soup : {false, true}) {
                EXPECT(em(good, ok, n, power, with_soup).status == OK);
                EXPECT(mstep(good, ok, true, power, with_soup).status == OK);
            }

    // the iteration count
    for (const int n : {0, -1, std::numeric_limits<int>::min()}) {
        const Verdict verdict = em(good, ok, n, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.what[0] == 'n' && verdict.at == -1);
    }

    // the power: finite and above 0
    EXPECT(power_valid(2.0f) && power_valid(tiny) && power_valid(huge) && !power_valid(0.0f) && !power_valid(-0.0f));
    for (const float bad : {0.0f, -0.0f, -tiny, -2.0f, nan, inf, -inf}) {
        EXPECT(!power_valid(bad));
        EXPECT(em(good, ok, 3, bad).status == INVALID);
        EXPECT(mstep(good, ok, true, bad).status == INVALID);
    }

    // call order: the M-step names what is missing, the problem first, then the table, then the posteriors
    {
        Facts f = good;
        f.have_problem = false;
        f.have_table = false;
        Verdict verdict = mstep(f, ok, false, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.what[14] == 'p');  // "call order: a problem ..."
        f.have_problem = true;
        verdict = mstep(f, ok, false, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.what[12] == 'g');  // "call order: genotype probabilities ..."
        f.have_table = true;
        verdict = mstep(f, ok, false, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.what[15] == 'E');  // "call order: an E-step ..."
        EXPECT(mstep(f, ok, true, 2.0f).status == OK);
        for (int k = 0; k < 3; k++) {  // the loop: a problem and the prior betas
            Facts g = good;
            g.have_problem = k == 1;
            g.have_table = k == 2;
            EXPECT(em(g, ok, 3, 2.0f).status == INVALID);
        }
    }

    // a communicator, several ranks, a padded table: UNSUPPORTED, behind the call order, ahead of the arguments' values
    for (int k = 0; k < 3; k++) {
        Facts f = good;
        f.attached = k == 0;
        f.nranks = k == 1 ? 2 : 1;
        f.dense_table = k != 2;
        EXPECT(em(f, ok, 3, 2.0f).status == UNSUPPORTED);
        EXPECT(mstep(f, ok, true, 2.0f).status == UNSUPPORTED);
        Call c;
        c.alpha[0] = nan;
        c.soup[0] = 7.0f;
        EXPECT(em(f, c, 3, 2.0f, true).status == UNSUPPORTED);
        EXPECT(mstep(f, c, true, 2.0f, true).status == UNSUPPORTED);
        f.have_table = false;
        EXPECT(em(f, ok, 3, 2.0f).status == INVALID);
        EXPECT(mstep(f, ok, true, 2.0f).status == INVALID);
        EXPECT(mstep(good, ok, false, 2.0f).status == INVALID);
    }
    {
        Facts f = good;  // the loop's own arguments come first of all
        f.attached = true;
        EXPECT(em(f, ok, 0, 2.0f).status == INVALID);
        EXPECT(em(f, ok, 3, 0.0f).status == INVALID);
        EXPECT(mstep(f, ok, true, 0.0f).status == UNSUPPORTED);  // (the M-step: the context first)
    }

    // the pools, as dmx_estep_ambient refuses them
    {
        Call c;
        c.with_doublets = 2;
        EXPECT(em(good, c, 3, 2.0f).status == INVALID);
        c = Call();
        c.donors = {0, 2, 2, 1, 3};
        Verdict verdict = em(good, c, 3, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.at == 0);
        c = Call();
        c.pool_of[3] = 2;
        verdict = em(good, c, 3, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.at == 3);
        c = Call();
        c.row_ptr[4] = 14;
        verdict = em(good, c, 3, 2.0f);
        EXPECT(verdict.status == INVALID && verdict.at == 3);
        Facts wide = good;
        wide.G = 2000;
        wide.B = 1;
        std::vector<int32_t> d(45);
        for (int i = 0; i < 45; i++) d[(size_t)i] = i;
        const std::vector<int64_t> start{0, 45}, rows{0, 1035};
        const std::vector<int32_t> pool_of{0};
        const std::vector<float> pen{0.0f}, al{0.5f};
        const Pools p{1, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
        EXPECT(check_em(wide, p, 3, 2.0f, al.data(), nullptr).status == UNSUPPORTED);
        EXPECT(check_em(good, ok.pools(), 3, 2.0f, nullptr, nullptr).status == INVALID);  // null alpha with B > 0
        EXPECT(check_mstep(good, true, 2.0f, nullptr, nullptr).status == INVALID);
        Facts nobody = good;
        nobody.B = 0;
        EXPECT(check_mstep(nobody, true, 2.0f, nullptr, nullptr).status == OK);
    }

    // fractions: the ends of [0, 1] are in, everything else is out.  The loop does not look at a barcode in no pool; the M-step has
    // no pools and reads every barcode's.
    for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), tiny})
        for (size_t at = 0; at < 4; at++) {
            Call c;
            c.alpha[at] = fine;
            EXPECT(em(good, c, 3, 2.0f).status == OK && mstep(good, c, true, 2.0f).status == OK);
        }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -tiny, 2.0f, -1.0f})
        for (size_t at = 0; at < 4; at++) {
            Call c;
            c.alpha[at] = bad;
            const Verdict loop = em(good, c, 3, 2.0f), step = mstep(good, c, true, 2.0f);
            if (c.pool_of[at] < 0) {
                EXPECT(loop.status == OK);
            } else {
                EXPECT(loop.status == INVALID && loop.at == (long long)at);
            }
            EXPECT(step.status == INVALID && step.at == (long long)at);
        }

    // ambient values; a profile that is not supplied is not read
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -1e-30f, 2.0f})
        for (long long at = 0; at < V; at++) {
            Call c;
            c.soup[(size_t)at] = bad;
            const Verdict loop = em(good, c, 3, 2.0f, true), step = mstep(good, c, true, 2.0f, true);
            EXPECT(loop.status == INVALID && loop.at == at);
            EXPECT(step.status == INVALID && step.at == at);
            EXPECT(em(good, c, 3, 2.0f).status == OK && mstep(good, c, true, 2.0f).status == OK);
        }
    {
        Call c;  // a bad fraction and a bad profile: the fraction
        c.alpha[3] = 2.0f;
        c.soup[0] = nan;
        const Verdict loop = em(good, c, 3, 2.0f, true), step = mstep(good, c, true, 2.0f, true);
        EXPECT(loop.status == INVALID && loop.at == 3 && loop.what[0] == 'a' && loop.what[1] == 'l');
        EXPECT(step.status == INVALID && step.at == 3 && step.what[0] == 'a' && step.what[1] == 'l');
        c = Call();  // a bad power and a bad fraction: the power
        c.alpha[0] = nan;
        EXPECT(em(good, c, 3, -1.0f).what[0] == 't' && mstep(good, c, true, -1.0f).what[0] == 't');
    }

    return finish("ambient learning plan");
}
