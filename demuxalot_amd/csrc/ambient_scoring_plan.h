// ambient_scoring_plan.h -- what dmx_estep_ambient (estep_ambient.hip) refuses, as one pure function of plain values:
// everything dmx_estep_pools refuses of the pools, the per-barcode fractions, the soup's profile, and the contexts the pass does not
// run on.  Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp: dmx_estep_ambient asks check() before anything is uploaded
// or launched; tests/ambient_scoring_plan_check.cpp walks it on the CPU.
#pragma once
#include <cstdint>

#include "ambient_plan.h"

namespace dmx {
namespace asplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using aplan::Facts;
using aplan::Verdict;
using aplan::INVALID;
using aplan::OK;
using aplan::UNSUPPORTED;

constexpr long long MAX_OPTIONS = 1024;     // POOL_MAX_OPTIONS (estep_pools.h; estep_ambient.hip asserts the value)
constexpr long long MAX_COLUMN = 65536;     // an option holds its two table columns in 16 bits each

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

// The order is the order of the refusals: the context, the pools as dmx_estep_pools walks them, the fractions, the profile.
// alpha[b] of a barcode in no pool is not looked at.
inline Verdict check(const Facts &f, const Pools &p, const float *alpha, const float *ambient)
{
    if (!f.have_problem || !f.have_table) return {INVALID, "call order: a problem and genotype probabilities (dmx_probs_from_betas / dmx_set_probs) come first", -1};
    if (f.attached || f.nranks > 1) return {UNSUPPORTED, "a context with a communicator attached is not supported", -1};
    if (!f.dense_table) return {UNSUPPORTED, "the genotype table is in a padded exchange layout", -1};
    if (p.with_doublets != 0 && p.with_doublets != 1) return {INVALID, "with_doublets must be 0 or 1", -1};
    if (p.n_pools < 0) return {INVALID, "negative n_pools", -1};
    if (!p.pool_start || !p.row_ptr) return {INVALID, "null pool_start / row_ptr", -1};
    if (p.n_pools > 0 && (!p.pool_donors || !p.pair_penalty)) return {INVALID, "null pool_donors / pair_penalty", -1};
    if (f.B > 0 && !p.pool_of_barcode) return {INVALID, "null pool_of_barcode", -1};
    if (f.B > 0 && !alpha) return {INVALID, "null alpha", -1};
    if (p.pool_start[0] != 0) return {INVALID, "pool_start[0] is not 0", -1};
    for (long long q = 0; q < p.n_pools; q++) {
        const long long first = p.pool_start[q], g = p.pool_start[q + 1] - first;
        if (g < 0) return {INVALID, "pool_start decreases at a pool", q};
        if (g == 0) return {INVALID, "a pool is empty", q};
        for (long long i = 0; i < g; i++) {
            const long long d = p.pool_donors[first + i];
            if (d < 0 || d >= f.G) return {INVALID, "a donor of a pool is outside [0, G)", q};
            if (i > 0 && d <= p.pool_donors[first + i - 1]) return {INVALID, "the donors of a pool are not strictly ascending", q};
            if (d >= MAX_COLUMN) return {UNSUPPORTED, "a donor index of a pool does not fit the 16 bits of an option's column", q};
        }
        if (options_of(g, p.with_doublets != 0) > MAX_OPTIONS)
            return {UNSUPPORTED, "a pool has more than 1024 options (44 donors with doublets, 1024 without)", q};
    }
    if (p.row_ptr[0] != 0) return {INVALID, "row_ptr[0] is not 0", -1};
    for (long long b = 0; b < f.B; b++) {
        const long long q = p.pool_of_barcode[b];
        if (q < -1 || q >= p.n_pools) return {INVALID, "pool_of_barcode of a barcode is outside [-1, n_pools)", b};
        const long long options = q < 0 ? 0 : options_of(p.pool_start[q + 1] - p.pool_start[q], p.with_doublets != 0);
        if (p.row_ptr[b + 1] - p.row_ptr[b] != options) return {INVALID, "row_ptr gives a barcode other entries than its pool has options", b};
    }
    for (long long b = 0; b < f.B; b++)
        if (p.pool_of_barcode[b] >= 0 && !aplan::unit_range(alpha[b])) return {INVALID, "alpha of a barcode is not finite or outside [0, 1]", b};
    if (ambient)
        for (long long v = 0; v < f.V; v++)
            if (!aplan::unit_range(ambient[v])) return {INVALID, "an ambient value is not finite or outside [0, 1]", v};
    return {OK, "", -1};
}

}  // namespace asplan
}  // namespace dmx
