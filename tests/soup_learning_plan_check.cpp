// soup_learning_plan_check.cpp -- walks demuxalot_amd/csrc/soup_learning_plan.h on the CPU (tests/test_soup_learning_plan_cpu.py builds
// it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of dmx_em_ambient_soup and
// dmx_mstep_soup with its code - the pseudo-count, and everything dmx_em_ambient and dmx_mstep_ambient refuse, in their words
// (alplan::check_em / check_mstep, composed here; tests/ambient_learning_plan_check.cpp walks them on their own) -, the boundaries of
// the pseudo-count, the iteration count and the unit range, the order of the checks, and whose fraction is read.
#include <cmath>
#include <limits>

#include "plan_check.h"
#include "soup_learning_plan.h"

using namespace dmx::slplan;
namespace al = dmx::alplan;

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
    auto em = [&](const Facts &f, const Call &c, int n, float power, float pseudo, bool with_soup = false) {
        return check_em(f, c.pools(), n, power, pseudo, c.alpha.data(), with_soup ? c.soup.data() : nullptr);
    };
    auto mstep = [&](const Facts &f, const Call &c, bool have_post, float pseudo, bool with_soup = false) {
        return check_mstep(f, have_post, pseudo, c.alpha.data(), with_soup ? c.soup.data() : nullptr);
    };
    // what the entries without a pseudo-count say of the same call
    auto em_ambient = [&](const Facts &f, const Call &c, int n, float power, bool with_soup = false) {
        return al::check_em(f, c.pools(), n, power, c.alpha.data(), with_soup ? c.soup.data() : nullptr);
    };
    auto mstep_ambient = [&](const Facts &f, const Call &c, bool have_post, bool with_soup = false) {
        return al::check_mstep(f, have_post, POWER, c.alpha.data(), with_soup ? c.soup.data() : nullptr);
    };
    EXPECT(POWER == 1.0f && al::power_valid(POWER));

    // valid calls: one iteration and many, the reference's power and others, pseudo-counts over the whole range, with and without a profile
    for (const int n : {1, 2, 5, 1000000})
        for (const float power : {2.0f, 1.5f, 1.0f, tiny, huge})
            for (const float pseudo : {1.0f, tiny, huge, 0.5f, 1e-30f})
                for (const bool with_soup : {false, true}) {
                    EXPECT(em(good, ok, n, power, pseudo, with_soup).status == OK);
                    EXPECT(mstep(good, ok, true, pseudo, with_soup).status == OK);
                }

    // the pseudo-count: finite and above 0
    EXPECT(pseudo_count_valid(1.0f) && pseudo_count_valid(tiny) && pseudo_count_valid(huge) && !pseudo_count_valid(0.0f) && !pseudo_count_valid(-0.0f));
    for (const float bad : {0.0f, -0.0f, -tiny, -1.0f, nan, inf, -inf}) {
        EXPECT(!pseudo_count_valid(bad));
        const Verdict loop = em(good, ok, 3, 2.0f, bad), step = mstep(good, ok, true, bad);
        EXPECT(loop.status == INVALID && loop.at == -1 && loop.what[4] == 'p' && loop.what[5] == 's');  // "the pseudo-count ..."
        EXPECT(step.status == INVALID && step.at == -1 && same(step, loop));
    }

    // the iteration count and the power come first in the loop, in dmx_em_ambient's words; the pseudo-count behind them
    for (const int n : {0, -1, std::numeric_limits<int>::min()})
        for (const float pseudo : {1.0f, 0.0f, nan}) {
            const Verdict verdict = em(good, ok, n, 2.0f, pseudo);
            EXPECT(verdict.status == INVALID && verdict.what[0] == 'n' && same(verdict, em_ambient(good, ok, n, 2.0f)));
        }
    for (const float bad : {0.0f, -0.0f, -tiny, -2.0f, nan, inf, -inf})
        for (const float pseudo : {1.0f, 0.0f, nan}) {
            const Verdict verdict = em(good, ok, 3, bad, pseudo);
            EXPECT(verdict.status == INVALID && verdict.what[0] == 't' && verdict.what[4] == 'c' && same(verdict, em_ambient(good, ok, 3, bad)));
        }
    EXPECT(em(good, ok, 0, 0.0f, 0.0f).what[0] == 'n');

    // everything the entries without a pseudo-count refuse of the context and the pools: the same verdict, and ahead of a bad
    // pseudo-count where it is the context's (the M-step) - behind it where it is not one of the loop's own arguments
    {
        int walked = 0;
        borrowed_refusals<Call>(good, G, INVALID, UNSUPPORTED, [&](const Call &c, const Facts &f, int code) {
            const Verdict loop = em(f, c, 3, 2.0f, 1.0f);
            EXPECT(loop.status == code && same(loop, em_ambient(f, c, 3, 2.0f)));
            EXPECT(em(f, c, 3, 2.0f, 0.0f).what[4] == 'p');  // the loop's own arguments come first of all
            if (walked < 5) {  // the context's: the M-step has no pools
                const Verdict step = mstep(f, c, true, 1.0f);
                EXPECT(step.status == code && same(step, mstep_ambient(f, c, true)));
                EXPECT(same(mstep(f, c, true, 0.0f), step));  // (the M-step: the context first)
                EXPECT(same(mstep(f, c, true, nan, true), step));
            } else {
                EXPECT(mstep(f, c, true, 1.0f).status == OK);
            }
            walked++;
        });
        EXPECT(walked == 12);
    }

    // call order: the M-step names what is missing, the problem first, then the table, then the posteriors - whatever the pseudo-count
    for (const float pseudo : {1.0f, 0.0f}) {
        Facts f = good;
        f.have_problem = false;
        f.have_table = false;
        Verdict verdict = mstep(f, ok, false, pseudo);
        EXPECT(verdict.status == INVALID && verdict.what[14] == 'p');  // "call order: a problem ..."
        f.have_problem = true;
        verdict = mstep(f, ok, false, pseudo);
        EXPECT(verdict.status == INVALID && verdict.what[12] == 'g');  // "call order: genotype probabilities ..."
        f.have_table = true;
        verdict = mstep(f, ok, false, pseudo);
        EXPECT(verdict.status == INVALID && verdict.what[15] == 'E');  // "call order: an E-step ..."
        EXPECT(same(verdict, mstep_ambient(f, ok, false)));
        EXPECT(mstep(f, ok, true, 1.0f).status == OK);
        for (int k = 0; k < 3; k++) {  // the loop: a problem and the prior betas
            Facts g = good;
            g.have_problem = k == 1;
            g.have_table = k == 2;
            EXPECT(em(g, ok, 3, 2.0f, 1.0f).status == INVALID);
        }
    }

    // null fractions; a context without barcodes reads none
    {
        EXPECT(check_em(good, ok.pools(), 3, 2.0f, 1.0f, nullptr, nullptr).status == INVALID);
        EXPECT(check_mstep(good, true, 1.0f, nullptr, nullptr).status == INVALID);
        Facts nobody = good;
        nobody.B = 0;
        EXPECT(check_mstep(nobody, true, 1.0f, nullptr, nullptr).status == OK);
        EXPECT(check_mstep(nobody, true, 0.0f, nullptr, nullptr).status == INVALID);
    }

    // fractions: the ends of [0, 1] are in, everything else is out.  The loop does not look at a barcode in no pool; the M-step has
    // no pools and reads every barcode's.  A bad pseudo-count comes ahead of a bad fraction.
    for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), tiny})
        for (size_t at = 0; at < 4; at++) {
            Call c;
            c.alpha[at] = fine;
            EXPECT(em(good, c, 3, 2.0f, 1.0f).status == OK && mstep(good, c, true, 1.0f).status == OK);
        }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -tiny, 2.0f, -1.0f})
        for (size_t at = 0; at < 4; at++) {
            Call c;
            c.alpha[at] = bad;
            const Verdict loop = em(good, c, 3, 2.0f, 1.0f), step = mstep(good, c, true, 1.0f);
            if (c.pool_of[at] < 0) {
                EXPECT(loop.status == OK);
            } else {
                EXPECT(loop.status == INVALID && loop.at == (long long)at && same(loop, em_ambient(good, c, 3, 2.0f)));
            }
            EXPECT(step.status == INVALID && step.at == (long long)at && same(step, mstep_ambient(good, c, true)));
            EXPECT(em(good, c, 3, 2.0f, 0.0f).what[4] == 'p' && mstep(good, c, true, 0.0f).what[4] == 'p');
        }

    // ambient values; a profile that is not supplied is not read
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -1e-30f, 2.0f})
        for (long long at = 0; at < V; at++) {
            Call c;
            c.soup[(size_t)at] = bad;
            const Verdict loop = em(good, c, 3, 2.0f, 1.0f, true), step = mstep(good, c, true, 1.0f, true);
            EXPECT(loop.status == INVALID && loop.at == at && same(loop, em_ambient(good, c, 3, 2.0f, true)));
            EXPECT(step.status == INVALID && step.at == at && same(step, mstep_ambient(good, c, true, true)));
            EXPECT(em(good, c, 3, 2.0f, 1.0f).status == OK && mstep(good, c, true, 1.0f).status == OK);
        }
    {
        Call c;  // a bad fraction and a bad profile: the fraction
        c.alpha[3] = 2.0f;
        c.soup[0] = nan;
        const Verdict loop = em(good, c, 3, 2.0f, 1.0f, true), step = mstep(good, c, true, 1.0f, true);
        EXPECT(loop.status == INVALID && loop.at == 3 && loop.what[0] == 'a' && loop.what[1] == 'l');
        EXPECT(step.status == INVALID && step.at == 3 && step.what[0] == 'a' && step.what[1] == 'l');
    }

    return finish("soup learning plan");
}
