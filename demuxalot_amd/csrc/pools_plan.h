// pools_plan.h -- what the pooled entries (dmx_estep_pools, dmx_estep_pools_resident, dmx_em_pools, dmx_estep_ambient)
// refuse of their pool arguments and how they lay a pool's options out, as pure functions of plain values.  Host only: nothing of
// HIP, nothing of dmx_ctx.  dmx_steps.cpp: plan_pools asks check() before anything is uploaded or launched, accept_pools layout() for
// what was accepted; ambient_scoring_plan.h puts its own refusals around the same check(); tests/pools_plan_check.cpp walks both on the CPU.
#pragma once
#include <cstdint>
#include <vector>

namespace dmx {
namespace pplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

constexpr int OK = 0, INVALID = -1, UNSUPPORTED = -5;  // DMX_OK, DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED (dmx_steps.cpp asserts the values)
constexpr long long MAX_OPTIONS = 1024;  // the register-resident row of the exact epilogue (estep_epilogue.h: reg_row_sum)
constexpr long long MAX_COLUMN = 65536;  // an option holds its two table columns in 16 bits each

struct Verdict {
    int status;            // OK, INVALID, UNSUPPORTED
    const char *what;      // static text
    long long at;          // index the text speaks of, or -1
    long long value = -1;  // a number that goes in front of the text, or -1
};

// the pool arguments of the dmx_estep_pools family, as the caller passed them
struct Pools {
    int with_doublets;
    long long n_pools;
    const int64_t *pool_start;       // [n_pools + 1]
    const int32_t *pool_donors;
    const float *pair_penalty;       // [n_pools]
    const int32_t *pool_of_barcode;  // [B]
    const int64_t *row_ptr;          // [B + 1]
};

// options of a pool of g donors
inline long long options_of(long long g, bool with_doublets) { return with_doublets ? g * (g + 1) / 2 : g; }

// G: columns of the genotype table, B: barcodes.  The order is the order of the refusals.
inline Verdict check(int G, long long B, const Pools &p)
{
    if (p.with_doublets != 0 && p.with_doublets != 1) return {INVALID, "with_doublets must be 0 or 1", -1};
    if (p.n_pools < 0) return {INVALID, "negative n_pools", -1};
    if (!p.pool_start || !p.row_ptr) return {INVALID, "null pool_start / row_ptr", -1};
    if (p.n_pools > 0 && (!p.pool_donors || !p.pair_penalty)) return {INVALID, "null pool_donors / pair_penalty", -1};
    if (B > 0 && !p.pool_of_barcode) return {INVALID, "null pool_of_barcode", -1};
    if (p.pool_start[0] != 0) return {INVALID, "pool_start[0] is not 0", -1};
    for (long long q = 0; q < p.n_pools; q++) {
        const long long first = p.pool_start[q], g = p.pool_start[q + 1] - first;
        if (g < 0) return {INVALID, "pool_start decreases at a pool", q};
        if (g == 0) return {INVALID, "a pool is empty", q};
        for (long long i = 0; i < g; i++) {
            const long long d = p.pool_donors[first + i];
            if (d < 0 || d >= G) return {INVALID, "a donor of a pool is outside [0, G)", q};
            if (i > 0 && d <= p.pool_donors[first + i - 1]) return {INVALID, "the donors of a pool are not strictly ascending", q};
            if (d >= MAX_COLUMN) return {UNSUPPORTED, "a donor index of a pool does not fit the 16 bits of an option's column", q};
        }
        // (the one text that is read behind its verdict's value: "1035 options in a pool, more than 1024 options ...")
        static_assert(MAX_OPTIONS == 1024, "the text below spells the limit out");
        const long long options = options_of(g, p.with_doublets != 0);
        if (options > MAX_OPTIONS) return {UNSUPPORTED, "options in a pool, more than 1024 options (44 donors with doublets, 1024 without)", q, options};
    }
    if (p.row_ptr[0] != 0) return {INVALID, "row_ptr[0] is not 0", -1};
    for (long long b = 0; b < B; b++) {
        const long long q = p.pool_of_barcode[b];
        if (q < -1 || q >= p.n_pools) return {INVALID, "pool_of_barcode of a barcode is outside [-1, n_pools)", b};
        const long long options = q < 0 ? 0 : options_of(p.pool_start[q + 1] - p.pool_start[q], p.with_doublets != 0);
        if (p.row_ptr[b + 1] - p.row_ptr[b] != options) return {INVALID, "row_ptr gives a barcode other entries than its pool has options", b};
    }
    return {OK, "", -1};
}

// The options of every pool that check() has accepted, d1 | d2 << 16 (table columns; a singlet: d1 == d2), in the reference's order
// for the pool's genotype list (demux.py:175-191): singlets in list order, then the pairs i < j, i-major.
inline void layout(const Pools &p, std::vector<long long> &opt_ptr, std::vector<unsigned> &opts, std::vector<int> &pool_size)
{
    opt_ptr.assign(1, 0);
    opts.clear();
    pool_size.clear();
    for (long long q = 0; q < p.n_pools; q++) {
        const int32_t *d = p.pool_donors + p.pool_start[q];
        const long long g = p.pool_start[q + 1] - p.pool_start[q];
        for (long long i = 0; i < g; i++) opts.push_back((unsigned)d[i] | (unsigned)d[i] << 16);
        if (p.with_doublets)
            for (long long i = 0; i < g; i++)
                for (long long j = i + 1; j < g; j++) opts.push_back((unsigned)d[i] | (unsigned)d[j] << 16);
        pool_size.push_back((int)g);
        opt_ptr.push_back((long long)opts.size());
    }
}

}  // namespace pplan
}  // namespace dmx
