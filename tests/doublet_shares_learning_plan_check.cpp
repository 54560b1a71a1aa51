// doublet_shares_learning_plan_check.cpp -- walks demuxalot_amd/csrc/doublet_shares_learning_plan.h on the CPU
// (tests/test_doublet_shares_learning_plan_cpu.py builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain
// program): every refusal of dmx_em_doublet_shares, dmx_estep_pair_shares_resident and dmx_mstep_doublet_shares with its code - what
// pair_shares_plan.h refuses of the context, the pools and the grid, then what doublet_learning_plan.h refuses of the loop's and the
// M-step's own arguments, in that order and with their words -, the share rows of the M-step - present, every pair entry finite and in
// [0, 1] with its index, singlet entries not read -, and the boundaries.
#include <cmath>
#include <cstring>
#include <limits>

#include "doublet_shares_learning_plan.h"
#include "plan_check.h"

using namespace dmx::dslplan;

static bool says(const Verdict &verdict, const char *words) { return std::strstr(verdict.what, words) != nullptr; }

// the shared pooled call (plan_check.h) with the posterior and the share rows of its 15 options, a grid of shares and its log weights.
// The singlet entries of the share rows are NaN, as the E-step leaves them.
namespace {  // (Pools is hidden from the library's exports; so is what derives from it)
struct Call : PooledCall<Pools> {
    std::vector<float> rows = std::vector<float>(15, 0.125f);
    std::vector<float> shares = std::vector<float>(15, 0.75f);
    std::vector<float> grid{0.7f, 0.1f, 0.5f, 1.0f, 0.1f, 0.0f};
    std::vector<float> weights{-1.0f, 0.0f, 0.5f, -30.0f, 2.0f, -0.0f};
    Call()
    {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (const size_t k : singlets()) shares[k] = nan;
    }
    static std::vector<size_t> singlets() { return {0, 1, 2, 6, 7, 9, 10, 11}; }
    static std::vector<size_t> pairs() { return {3, 4, 5, 8, 12, 13, 14}; }
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
    auto em = [&](const Facts &f, const Call &c, int n, float power, float threshold) {
        return check_em(f, c.pools(), (long long)c.grid.size(), c.grid.data(), c.weights.data(), n, power, threshold);
    };
    auto estep = [&](const Facts &f, const Call &c) { return check_estep(f, c.pools(), (long long)c.grid.size(), c.grid.data(), c.weights.data()); };
    auto mstep = [&](const Facts &f, const Call &c, bool have_post, float power, float threshold) {
        return check_mstep(f, have_post, c.pools(), power, threshold, (long long)c.rows.size(), c.rows.data(), c.shares.data());
    };

    // valid calls
    for (const int n : {1, 2, 5, 1000000})
        for (const float power : {2.0f, 1.5f, 1.0f, tiny, huge, 0.25f})
            for (const float threshold : {1e-3f, 1e-6f, tiny, 1.0f, std::nextafter(1.0f, 2.0f), 2.0f, huge}) {
                EXPECT(em(good, ok, n, power, threshold).status == OK);
                EXPECT(mstep(good, ok, true, power, threshold).status == OK);
            }
    EXPECT(estep(good, ok).status == OK);
    EXPECT(check_em(good, ok.pools(), 1, ok.grid.data(), nullptr, 1, 2.0f, 1e-3f).status == OK);  // no weights: all 0
    EXPECT(check_estep(good, ok.pools(), 1, ok.grid.data(), nullptr).status == OK);

    // the loop's own arguments, with doublet_learning_plan.h's words
    for (const int n : {0, -1, std::numeric_limits<int>::min()}) {
        const Verdict verdict = em(good, ok, n, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && says(verdict, "n_iterations") && verdict.at == -1);
    }
    for (const float bad : {0.0f, -0.0f, -tiny, -2.0f, nan, inf, -inf}) {
        EXPECT(em(good, ok, 3, bad, 1e-3f).status == INVALID && says(em(good, ok, 3, bad, 1e-3f), "power"));
        EXPECT(em(good, ok, 3, 2.0f, bad).status == INVALID && says(em(good, ok, 3, 2.0f, bad), "min_pair_posterior"));
        EXPECT(mstep(good, ok, true, bad, 1e-3f).status == INVALID && says(mstep(good, ok, true, bad, 1e-3f), "power"));
        EXPECT(mstep(good, ok, true, 2.0f, bad).status == INVALID && says(mstep(good, ok, true, 2.0f, bad), "min_pair_posterior"));
    }
    EXPECT(says(em(good, ok, 0, nan, nan), "n_iterations") && says(em(good, ok, 1, nan, nan), "power"));  // the order: count, power, threshold

    // the grid, with pair_shares_plan.h's words and indices; ahead of the loop's own arguments
    {
        const Pools p = ok.pools();
        for (const long long n : {0ll, -1ll}) {
            const Verdict verdict = check_em(good, p, n, ok.grid.data(), ok.weights.data(), 0, nan, nan);
            EXPECT(verdict.status == INVALID && says(verdict, "at least one value"));
            EXPECT(check_estep(good, p, n, ok.grid.data(), ok.weights.data()).status == INVALID);
        }
        EXPECT(check_em(good, p, 6, nullptr, ok.weights.data(), 3, 2.0f, 1e-3f).status == INVALID);
        EXPECT(says(check_em(good, p, 6, nullptr, ok.weights.data(), 3, 2.0f, 1e-3f), "null shares"));
        for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -tiny, 2.0f})
            for (size_t at = 0; at < ok.grid.size(); at++) {
                Call c;
                c.grid[at] = bad;
                Verdict verdict = em(good, c, 0, nan, nan);  // (the grid is refused first)
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at && says(verdict, "a share is not finite"));
                verdict = estep(good, c);
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at);
                c = Call();
                if (bad >= -1.0f && bad <= 3.0f) continue;  // (a finite weight is any finite value)
                c.weights[at] = bad;
                verdict = em(good, c, 3, 2.0f, 1e-3f);
                EXPECT(verdict.status == INVALID && verdict.at == (long long)at && says(verdict, "log weight"));
            }
        for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), tiny}) {
            Call c;
            c.grid[2] = fine;
            EXPECT(em(good, c, 3, 2.0f, 1e-3f).status == OK && estep(good, c).status == OK);
        }
        std::vector<float> many(65, 0.5f), zeros(65, 0.0f);
        EXPECT(check_em(good, p, 64, many.data(), zeros.data(), 3, 2.0f, 1e-3f).status == OK);
        Verdict verdict = check_em(good, p, 65, many.data(), zeros.data(), 3, 2.0f, 1e-3f);
        EXPECT(verdict.status == UNSUPPORTED && verdict.at == 65);
        verdict = check_em(good, p, 65, many.data(), zeros.data(), 0, 2.0f, 1e-3f);  // (the unsupported length ahead of the count)
        EXPECT(verdict.status == UNSUPPORTED);
        many[64] = nan;
        EXPECT(check_em(good, p, 65, many.data(), zeros.data(), 3, 2.0f, 1e-3f).status == INVALID);  // (read in full first)
        EXPECT(check_estep(good, p, 65, many.data(), zeros.data()).status == INVALID);
    }

    // call order: the loop and the resident E-step name the problem and the table; the M-step names what is missing one by one
    {
        for (int k = 0; k < 3; k++) {
            Facts f = good;
            f.have_problem = k == 1;
            f.have_table = k == 2;
            EXPECT(em(f, ok, 3, 2.0f, 1e-3f).status == INVALID && says(em(f, ok, 3, 2.0f, 1e-3f), "call order"));
            EXPECT(estep(f, ok).status == INVALID && says(estep(f, ok), "call order"));
        }
        Facts f = good;
        f.have_problem = false;
        f.have_table = false;
        EXPECT(says(mstep(f, ok, false, 2.0f, 1e-3f), "a problem comes first"));
        f.have_problem = true;
        EXPECT(says(mstep(f, ok, false, 2.0f, 1e-3f), "genotype probabilities"));
        f.have_table = true;
        EXPECT(says(mstep(f, ok, false, 2.0f, 1e-3f), "an E-step comes first") && mstep(f, ok, false, 2.0f, 1e-3f).status == INVALID);
        EXPECT(mstep(f, ok, true, 2.0f, 1e-3f).status == OK);
    }

    // a communicator, several ranks, a padded table: UNSUPPORTED, ahead of the pools and the grid
    for (int k = 0; k < 3; k++) {
        Facts f = good;
        f.attached = k == 0;
        f.nranks = k == 1 ? 2 : 1;
        f.dense_table = k != 2;
        Call c;
        c.donors = {0, 2, 2, 1, 3};
        c.grid[0] = nan;
        c.shares[3] = nan;
        EXPECT(em(f, c, 3, 2.0f, 1e-3f).status == UNSUPPORTED && estep(f, c).status == UNSUPPORTED && mstep(f, c, true, 2.0f, 1e-3f).status == UNSUPPORTED);
        EXPECT(em(f, ok, 0, 2.0f, 1e-3f).status == UNSUPPORTED);  // (the context is the grid's check's first step)
        EXPECT(mstep(f, ok, true, 0.0f, 1e-3f).status == INVALID);  // (the M-step's own numbers come first: doublet_learning_plan.h)
    }

    // the pools, as the pooled entries refuse them
    {
        Call c;
        c.with_doublets = 2;
        EXPECT(em(good, c, 3, 2.0f, 1e-3f).status == INVALID && estep(good, c).status == INVALID && mstep(good, c, true, 2.0f, 1e-3f).status == INVALID);
        c = Call();
        c.donors = {0, 2, 2, 1, 3};
        EXPECT(em(good, c, 3, 2.0f, 1e-3f).status == INVALID && em(good, c, 3, 2.0f, 1e-3f).at == 0);
        EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == INVALID && mstep(good, c, true, 2.0f, 1e-3f).at == 0);
        c = Call();
        c.pool_of[3] = 2;
        EXPECT(em(good, c, 3, 2.0f, 1e-3f).at == 3 && estep(good, c).at == 3 && mstep(good, c, true, 2.0f, 1e-3f).at == 3);
        c.grid[1] = nan;  // bad pools and a bad grid: the pools
        EXPECT(em(good, c, 3, 2.0f, 1e-3f).at == 3 && !says(em(good, c, 3, 2.0f, 1e-3f), "share"));
        Facts wide = good;
        wide.G = 2000;
        wide.B = 1;
        std::vector<int32_t> d(45);
        for (int i = 0; i < 45; i++) d[(size_t)i] = i;
        const std::vector<int64_t> start{0, 45}, rows{0, 1035};
        const std::vector<int32_t> pool_of{0};
        const std::vector<float> pen{0.0f}, post(1035, 0.0f), mean(1035, 0.5f);
        const Pools p{1, 1, start.data(), d.data(), pen.data(), pool_of.data(), rows.data()};
        Verdict verdict = check_em(wide, p, 6, ok.grid.data(), nullptr, 3, 2.0f, 1e-3f);
        EXPECT(verdict.status == UNSUPPORTED && verdict.value == 1035);
        EXPECT(check_mstep(wide, true, p, 2.0f, 1e-3f, 1035, post.data(), mean.data()).status == UNSUPPORTED);
        d.pop_back();  // 44 donors: 990 options, the most a pool holds with doublets
        const std::vector<int64_t> start44{0, 44}, rows44{0, 990};
        const Pools q{1, 1, start44.data(), d.data(), pen.data(), pool_of.data(), rows44.data()};
        EXPECT(check_em(wide, q, 6, ok.grid.data(), nullptr, 3, 2.0f, 1e-3f).status == OK);
        EXPECT(check_mstep(wide, true, q, 2.0f, 1e-3f, 990, post.data(), mean.data()).status == OK);
        EXPECT(pair_options(1, q) == 990 - 44);
        std::vector<float> last = mean;
        last[989] = nan;
        verdict = check_mstep(wide, true, q, 2.0f, 1e-3f, 990, post.data(), last.data());
        EXPECT(verdict.status == INVALID && verdict.at == 989);
        last[989] = 0.5f;
        last[43] = nan;  // the last singlet entry: not read
        EXPECT(check_mstep(wide, true, q, 2.0f, 1e-3f, 990, post.data(), last.data()).status == OK);
        last[44] = inf;  // the first pair entry
        EXPECT(check_mstep(wide, true, q, 2.0f, 1e-3f, 990, post.data(), last.data()).at == 44);
    }

    // the posterior rows: dmx_mstep_doublets' refusals, ahead of the share rows
    {
        const Pools p = ok.pools();
        for (const long long n : {0ll, 14ll, 16ll, -1ll}) {
            const Verdict verdict = check_mstep(good, true, p, 2.0f, 1e-3f, n, ok.rows.data(), ok.shares.data());
            EXPECT(verdict.status == INVALID && says(verdict, "another length") && verdict.at == -1);
        }
        EXPECT(says(check_mstep(good, true, p, 2.0f, 1e-3f, 15, nullptr, ok.shares.data()), "null posterior rows"));
        Call c;
        c.rows[4] = nan;
        c.shares[3] = nan;
        Verdict verdict = mstep(good, c, true, 2.0f, 1e-3f);
        EXPECT(verdict.status == INVALID && verdict.at == 4 && says(verdict, "a posterior of the rows"));
    }

    // the share rows: present; every pair entry finite and in [0, 1]; a singlet's entry is not read
    {
        const Pools p = ok.pools();
        const Verdict verdict = check_mstep(good, true, p, 2.0f, 1e-3f, 15, ok.rows.data(), nullptr);
        EXPECT(verdict.status == INVALID && says(verdict, "null share rows") && verdict.at == -1);
        Call nobody;  // every barcode in no pool: no rows - null posterior rows are theirs, null share rows are still refused
        nobody.pool_of = {-1, -1, -1, -1};
        nobody.row_ptr = {0, 0, 0, 0, 0};
        const float none_held = 0.0f;
        EXPECT(check_mstep(good, true, nobody.pools(), 2.0f, 1e-3f, 0, nullptr, &none_held).status == OK);
        const Verdict null_rows = check_mstep(good, true, nobody.pools(), 2.0f, 1e-3f, 0, nullptr, nullptr);
        EXPECT(null_rows.status == INVALID && says(null_rows, "null share rows"));
        Facts none = good;
        none.B = 0;
        const std::vector<int64_t> empty_rows{0};
        const Pools e{1, 2, ok.pool_start.data(), ok.donors.data(), ok.penalty.data(), nullptr, empty_rows.data()};
        EXPECT(check_mstep(none, true, e, 2.0f, 1e-3f, 0, nullptr, &none_held).status == OK);
        EXPECT(check_mstep(none, true, e, 2.0f, 1e-3f, 0, nullptr, nullptr).status == INVALID);
        EXPECT(check_em(none, e, 6, ok.grid.data(), nullptr, 1, 2.0f, 1e-3f).status == OK);
    }
    for (const float fine : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), tiny, 0.5f})
        for (const size_t at : Call::pairs()) {
            Call c;
            c.shares[at] = fine;
            EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == OK);
        }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -tiny, 2.0f, -1.0f}) {
        for (const size_t at : Call::pairs()) {
            Call c;
            c.shares[at] = bad;
            const Verdict verdict = mstep(good, c, true, 2.0f, 1e-3f);
            EXPECT(verdict.status == INVALID && verdict.at == (long long)at && says(verdict, "a pair's share of the rows"));
        }
        for (const size_t at : Call::singlets()) {
            Call c;
            c.shares[at] = bad;
            EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == OK);
        }
        Call c;  // two bad entries: the first
        c.shares[13] = bad;
        c.shares[5] = bad;
        EXPECT(mstep(good, c, true, 2.0f, 1e-3f).at == 5);
    }
    {
        Call c;  // without doublets a row has no pair entry: nothing of the share rows is read
        c.with_doublets = 0;
        c.row_ptr = {0, 3, 3, 5, 8};
        c.rows.assign(8, 0.5f);
        c.shares.assign(8, nan);
        EXPECT(mstep(good, c, true, 2.0f, 1e-3f).status == OK && em(good, c, 2, 2.0f, 1e-3f).status == OK && estep(good, c).status == OK);
        EXPECT(pair_options(B, c.pools()) == 0);
    }
    EXPECT(pair_options(B, ok.pools()) == 3 + 0 + 1 + 3);

    return finish("doublet shares learning plan");
}
