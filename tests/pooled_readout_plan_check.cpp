// pooled_readout_plan_check.cpp -- walks demuxalot_amd/csrc/pooled_readout_plan.h on the CPU (tests/test_pooled_readout_plan_cpu.py
// builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): what the entries over the resident
// pooled result refuse - the upload's pools (pools_plan.h's check, met refusal by refusal, and the rows), the allowed lists, the
// ranges of dmx_pooled_get / _get_pool, k of the top options - and the layouts they derive: marg_ptr, the pools' barcode lists, the
// slab bounds of the option sums.
#include <cstring>

#include "plan_check.h"
#include "pooled_readout_plan.h"

using namespace dmx::prplan;

// one upload's arrays, owned: pools {0, 2, 4} and {1, 3} of G = 5 and a third, {2}, without barcodes; five barcodes, the second and
// the last in no pool
struct Upload {
    int G = 5;
    int with_doublets = 1;
    std::vector<int64_t> pool_start{0, 3, 5, 6};
    std::vector<int32_t> donors{0, 2, 4, 1, 3, 2};
    std::vector<int32_t> pool_of{0, -1, 1, 0, -1};
    std::vector<int64_t> row_ptr{0, 6, 6, 9, 15, 15};
    std::vector<float> probs = std::vector<float>(15, 0.125f);
    bool with_probs = true;
    long long B() const { return (long long)pool_of.size(); }
    Verdict verdict() const
    {
        return check_upload(G, B(), with_doublets, (long long)pool_start.size() - 1, pool_start.data(), donors.data(), pool_of.data(), row_ptr.data(),
                            with_probs ? probs.data() : nullptr);
    }
};

static bool refused(const Verdict &v, int status, const char *word, long long at = -2)
{
    return v.status == status && std::strstr(v.what, word) != nullptr && (at == -2 || v.at == at);
}

int main()
{
    // ---- dmx_pooled_upload ------------------------------------------------------------------------------------------------
    const Upload ok;
    EXPECT(ok.verdict().status == OK);
    {
        Upload u;  // without doublets: rows of g entries
        u.with_doublets = 0;
        u.row_ptr = {0, 3, 3, 5, 8, 8};
        u.probs.assign(8, 0.5f);
        EXPECT(u.verdict().status == OK);
        u.row_ptr = ok.row_ptr;
        EXPECT(refused(u.verdict(), INVALID, "row_ptr gives", 0));
    }
    {
        Upload u;
        u.with_doublets = 2;
        EXPECT(refused(u.verdict(), INVALID, "with_doublets"));
        u = Upload();
        u.G = -1;
        EXPECT(refused(u.verdict(), INVALID, "negative G"));
        EXPECT(refused(check_upload(5, -1, 1, 3, ok.pool_start.data(), ok.donors.data(), ok.pool_of.data(), ok.row_ptr.data(), ok.probs.data()), INVALID, "negative B"));
        EXPECT(refused(check_upload(5, 5, 1, -1, ok.pool_start.data(), ok.donors.data(), ok.pool_of.data(), ok.row_ptr.data(), ok.probs.data()), INVALID, "negative n_pools"));
        EXPECT(refused(check_upload(5, 5, 1, 3, nullptr, ok.donors.data(), ok.pool_of.data(), ok.row_ptr.data(), ok.probs.data()), INVALID, "null pool_start"));
        EXPECT(refused(check_upload(5, 5, 1, 3, ok.pool_start.data(), ok.donors.data(), ok.pool_of.data(), nullptr, ok.probs.data()), INVALID, "null pool_start / row_ptr"));
        EXPECT(refused(check_upload(5, 5, 1, 3, ok.pool_start.data(), nullptr, ok.pool_of.data(), ok.row_ptr.data(), ok.probs.data()), INVALID, "null pool_donors"));
        EXPECT(refused(check_upload(5, 5, 1, 3, ok.pool_start.data(), ok.donors.data(), nullptr, ok.row_ptr.data(), ok.probs.data()), INVALID, "null pool_of_barcode"));
    }
    {
        Upload u;
        u.pool_start[0] = 1;
        EXPECT(refused(u.verdict(), INVALID, "pool_start[0]"));
        u = Upload();
        u.pool_start = {0, 3, 2, 6};
        EXPECT(refused(u.verdict(), INVALID, "decreases", 1));
        u = Upload();
        u.pool_start = {0, 3, 3, 6};
        EXPECT(refused(u.verdict(), INVALID, "empty", 1));
        u = Upload();
        u.donors[4] = 5;  // == G
        EXPECT(refused(u.verdict(), INVALID, "outside [0, G)", 1));
        u.donors[4] = 4;
        EXPECT(u.verdict().status == OK);  // G - 1: the last column
        u = Upload();
        u.donors[0] = -1;
        EXPECT(refused(u.verdict(), INVALID, "outside [0, G)", 0));
        u = Upload();
        u.donors[1] = 0;  // a duplicate
        EXPECT(refused(u.verdict(), INVALID, "strictly ascending", 0));
        u = Upload();
        u.donors[1] = 4, u.donors[2] = 2;
        EXPECT(refused(u.verdict(), INVALID, "strictly ascending", 0));
    }
    {
        Upload u;
        u.row_ptr[0] = 1;
        EXPECT(refused(u.verdict(), INVALID, "row_ptr[0]"));
        u = Upload();
        u.pool_of[1] = -2;
        EXPECT(refused(u.verdict(), INVALID, "outside [-1, n_pools)", 1));
        u = Upload();
        u.pool_of[1] = 3;  // == n_pools
        EXPECT(refused(u.verdict(), INVALID, "outside [-1, n_pools)", 1));
        u = Upload();
        u.row_ptr = {0, 6, 7, 10, 16, 16};  // an entry for a barcode in no pool
        EXPECT(refused(u.verdict(), INVALID, "row_ptr gives", 1));
        u = Upload();
        u.with_probs = false;
        EXPECT(refused(u.verdict(), INVALID, "null probs"));
        u.pool_of.assign(5, -1);  // nobody in a pool: no rows, probs may be absent
        u.row_ptr.assign(6, 0);
        EXPECT(u.verdict().status == OK);
    }
    {
        // the widest pools: 44 donors with doublets (990 options) and 1024 without pass, one more is unsupported
        for (const int with_doublets : {1, 0})
            for (const int over : {0, 1}) {
                const int g = (with_doublets ? 44 : 1024) + over;
                std::vector<int64_t> start{0, g};
                std::vector<int32_t> donors((size_t)g);
                for (int i = 0; i < g; i++) donors[(size_t)i] = i;
                const int32_t pool_of[1] = {0};
                const int64_t row_ptr[2] = {0, with_doublets ? (int64_t)g * (g + 1) / 2 : g};
                const float probs[1] = {0.0f};
                const Verdict v = check_upload(2000, 1, with_doublets, 1, start.data(), donors.data(), pool_of, row_ptr, probs);
                EXPECT(over ? refused(v, UNSUPPORTED, "more than 1024 options", 0) : v.status == OK);
                if (over) EXPECT(v.value == (with_doublets ? 1035 : 1025));
            }
        std::vector<int64_t> start{0, 1};
        std::vector<int32_t> donors{65536};
        const int32_t pool_of[1] = {0};
        const int64_t row_ptr[2] = {0, 1};
        const float probs[1] = {1.0f};
        EXPECT(refused(check_upload(70000, 1, 0, 1, start.data(), donors.data(), pool_of, row_ptr, probs), UNSUPPORTED, "16 bits", 0));
        donors[0] = 65535;
        EXPECT(check_upload(70000, 1, 0, 1, start.data(), donors.data(), pool_of, row_ptr, probs).status == OK);
    }
    {
        // B == 0: no barcode arrays are read
        const int64_t start[2] = {0, 2}, row_ptr[1] = {0};
        const int32_t donors[2] = {0, 1};
        EXPECT(check_upload(2, 0, 1, 1, start, donors, nullptr, row_ptr, nullptr).status == OK);
        EXPECT(check_upload(0, 0, 0, 0, row_ptr, nullptr, nullptr, row_ptr, nullptr).status == OK);
    }

    // ---- dmx_pooled_allowed_mass -------------------------------------------------------------------------------------------
    {
        const long long B = ok.B();
        const int32_t *pool_of = ok.pool_of.data();
        const int64_t *row_ptr = ok.row_ptr.data();
        std::vector<int64_t> start{0, 2, 2, 5, 6, 6};
        std::vector<int32_t> options{5, 5, 0, 2, 1, 0};  // a duplicate, the last option of a row of 6, of a row of 3
        EXPECT(check_allowed(B, pool_of, row_ptr, start.data(), options.data()).status == OK);
        EXPECT(refused(check_allowed(B, pool_of, row_ptr, nullptr, options.data()), INVALID, "null allowed_start"));
        EXPECT(refused(check_allowed(B, pool_of, row_ptr, start.data(), nullptr), INVALID, "null allowed_options"));
        const std::vector<int64_t> none(6, 0);
        EXPECT(check_allowed(B, pool_of, row_ptr, none.data(), nullptr).status == OK);  // every list empty: no options are read
        auto with_start = [&](std::vector<int64_t> s) { return check_allowed(B, pool_of, row_ptr, s.data(), options.data()); };
        EXPECT(refused(with_start({1, 2, 2, 5, 6, 6}), INVALID, "allowed_start[0]"));
        EXPECT(with_start({1, 2, 2, 5, 6, 6}).value == 1);
        EXPECT(refused(with_start({0, 2, 1, 5, 6, 6}), INVALID, "decreases", 1));
        EXPECT(refused(with_start({0, 2, 2, 5, 6, 5}), INVALID, "decreases", 4));
        EXPECT(refused(with_start({0, 2, 3, 5, 6, 6}), INVALID, "in no pool", 1));
        EXPECT(refused(with_start({0, 2, 2, 5, 5, 6}), INVALID, "in no pool", 4));
        auto with_option = [&](size_t j, int32_t k) {
            std::vector<int32_t> o = options;
            o[j] = k;
            return check_allowed(B, pool_of, row_ptr, start.data(), o.data());
        };
        EXPECT(refused(with_option(0, 6), INVALID, "outside its barcode's row", 0));   // K = 6
        EXPECT(refused(with_option(1, -1), INVALID, "outside its barcode's row", 1));
        EXPECT(refused(with_option(3, 3), INVALID, "outside its barcode's row", 3));   // K = 3
        EXPECT(with_option(3, 3).value == 3);
        EXPECT(with_option(4, 0).status == OK && with_option(5, 5).status == OK);
        EXPECT(check_allowed(0, nullptr, none.data(), none.data(), nullptr).status == OK);
    }

    // ---- dmx_pooled_get / dmx_pooled_get_pool / dmx_pooled_top_options ------------------------------------------------------
    {
        const bool all[N_WHAT] = {true, true, true, true}, plain[N_WHAT] = {false, true, false, false};
        for (int what = 0; what < N_WHAT; what++) {
            EXPECT(check_get(5, what, all, 0, 5).status == OK);
            EXPECT(check_get_pool(3, what, all, 2).status == OK);
            EXPECT((check_get(5, what, plain, 0, 5).status == OK) == (what == PROBS));
            EXPECT((check_get_pool(3, what, plain, 0).status == OK) == (what == PROBS));
        }
        EXPECT(refused(check_get(5, LOGITS, plain, 0, 5), INVALID, "does not hold"));
        EXPECT(refused(check_get(5, -1, all, 0, 5), INVALID, "what is not") && refused(check_get(5, N_WHAT, all, 0, 5), INVALID, "what is not"));
        EXPECT(refused(check_get_pool(3, -1, all, 0), INVALID, "what is not") && refused(check_get_pool(3, N_WHAT, all, 0), INVALID, "what is not"));
        EXPECT(check_get(5, PROBS, all, 0, 0).status == OK && check_get(5, PROBS, all, 5, 5).status == OK && check_get(5, PROBS, all, 2, 3).status == OK);
        EXPECT(refused(check_get(5, PROBS, all, -1, 3), INVALID, "range"));
        EXPECT(refused(check_get(5, PROBS, all, 3, 2), INVALID, "range"));
        EXPECT(refused(check_get(5, PROBS, all, 0, 6), INVALID, "range"));
        EXPECT(check_get(0, PROBS, all, 0, 0).status == OK);
        EXPECT(refused(check_get_pool(3, PROBS, all, -1), INVALID, "outside [0, n_pools)"));
        EXPECT(refused(check_get_pool(3, PROBS, all, 3), INVALID, "outside [0, n_pools)"));
        EXPECT(refused(check_get_pool(0, PROBS, all, 0), INVALID, "outside [0, n_pools)"));
        for (int k = -1; k <= 6; k++) EXPECT((check_top(k).status == OK) == (k >= 1 && k <= TOP_MAX));
        EXPECT(refused(check_top(5), INVALID, "k is outside"));
    }

    // ---- marg_ptr and the pools' lists --------------------------------------------------------------------------------------
    {
        const std::vector<int> pool_size{3, 2, 1};
        std::vector<int64_t> m;
        marg_ptr(ok.B(), ok.pool_of.data(), pool_size.data(), m);
        EXPECT((m == std::vector<int64_t>{0, 3, 3, 5, 8, 8}));
        marg_ptr(0, nullptr, pool_size.data(), m);
        EXPECT((m == std::vector<int64_t>{0}));
        std::vector<int64_t> list_ptr;
        std::vector<int32_t> list;
        pool_lists(ok.B(), 3, ok.pool_of.data(), list_ptr, list);
        EXPECT((list_ptr == std::vector<int64_t>{0, 2, 3, 3}));  // the third pool has no barcodes
        EXPECT((list == std::vector<int32_t>{0, 3, 2}));
        pool_lists(0, 3, nullptr, list_ptr, list);
        EXPECT((list_ptr == std::vector<int64_t>{0, 0, 0, 0}) && list.empty());
        pool_lists(0, 0, nullptr, list_ptr, list);
        EXPECT((list_ptr == std::vector<int64_t>{0}) && list.empty());
        // interleaved pools: every list ascending, every pooled barcode listed once
        std::vector<int32_t> pool_of(1000);
        for (size_t b = 0; b < pool_of.size(); b++) pool_of[b] = (int32_t)((b * 7) % 5) - 1;
        pool_lists((long long)pool_of.size(), 4, pool_of.data(), list_ptr, list);
        EXPECT(list_ptr[4] == 800 && list.size() == 800);
        bool ordered = true;
        for (int p = 0; p < 4; p++)
            for (int64_t i = list_ptr[(size_t)p]; i < list_ptr[(size_t)p + 1]; i++) {
                ordered = ordered && pool_of[(size_t)list[(size_t)i]] == p;
                ordered = ordered && (i == list_ptr[(size_t)p] || list[(size_t)i - 1] < list[(size_t)i]);
            }
        EXPECT(ordered);
    }

    // ---- the slabs of the option sums ---------------------------------------------------------------------------------------
    for (const long long n : {0LL, 1LL, 2LL, 511LL, 512LL, 513LL, 1023LL, 1024LL, 1025LL, 1300LL, 100000LL, (1LL << 33) + 5}) {
        const long long per = slab_rows(n);
        EXPECT(per == (n + 511) / 512 && per * SUM_SLABS >= n && (n == 0 || (per - 1) * SUM_SLABS < n));
        long long covered = 0, next = 0;
        bool tiled = true;
        for (int j = 0; j < SUM_SLABS; j++) {
            const Slab s = slab(n, j);
            // k_option_partial's own bounds: [j per, min(j per + per, n)), empty when it starts past the list
            const long long b0 = (long long)j * per, b1 = b0 + per < n ? b0 + per : n;
            tiled = tiled && s.first <= s.last && s.last <= n && s.last - s.first <= per;
            tiled = tiled && (b1 > b0 ? (s.first == b0 && s.last == b1) : s.first == s.last);
            tiled = tiled && (s.first == s.last || s.first == next);
            if (s.last > s.first) next = s.last;
            covered += s.last - s.first;
        }
        EXPECT(tiled);
        EXPECT(covered == n);
    }
    EXPECT(slab(513, 0).last == 2 && slab(513, 256).first == 512 && slab(513, 256).last == 513 && slab(513, 257).first == slab(513, 257).last);
    EXPECT(slab(512, 511).first == 511 && slab(512, 511).last == 512);
    EXPECT(slab(1300, 433).first == 1299 && slab(1300, 433).last == 1300 && slab(1300, 434).first == 1300);

    return finish("pooled readout plan");
}
