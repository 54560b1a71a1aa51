// pooled_readout_plan.h -- what the entries over the resident compact result (the "pooled slot": dmx_pooled_upload, dmx_pooled_get,
// dmx_pooled_get_pool, dmx_pooled_readout, dmx_pooled_option_sums, dmx_pooled_allowed_mass) refuse of their
// arguments, and the small layouts they derive on the host, as pure functions of plain values.  Host only: nothing of HIP, nothing of
// dmx_ctx.  csrc/pooled_readout.hip asks them before anything is uploaded or launched; tests/pooled_readout_plan_check.cpp walks
// them on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "pools_plan.h"

namespace dmx {
namespace prplan __attribute__((visibility("hidden"))) {

using pplan::INVALID;
using pplan::OK;
using pplan::UNSUPPORTED;
using pplan::Verdict;

constexpr int SUM_SLABS = 512;  // results.hip: the slabs of k_option_partial
constexpr int TOP_MAX = 4;      // results.hip: dmx_get_top_options

// the matrices of the slot, as dmx_pooled_get / dmx_pooled_get_pool name them
enum What { LOGITS = 0, PROBS = 1, ALPHA_INDEX = 2, ALPHA_MEAN = 3, N_WHAT = 4 };

// dmx_pooled_upload: pools_plan.h's check() of the pool arguments (the entry has no pair penalties: none is read), then the rows
inline Verdict check_upload(int G, long long B, int with_doublets, long long n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                            const int32_t *pool_of_barcode, const int64_t *row_ptr, const float *probs)
{
    if (G < 0) return {INVALID, "negative G", -1};
    if (B < 0) return {INVALID, "negative B", -1};
    static const float no_penalty = 0.0f;  // (check() asks that there be penalties, and reads none)
    const pplan::Pools pools{with_doublets, n_pools, pool_start, pool_donors, &no_penalty, pool_of_barcode, row_ptr};
    const Verdict v = pplan::check(G, B, pools);
    if (v.status != OK) return v;
    if (row_ptr[B] > 0 && !probs) return {INVALID, "null probs with rows to hold", -1};
    return {OK, "", -1};
}

// options of barcode b's row: row_ptr says it (check() has tied it to the pool)
inline long long row_options(const int64_t *row_ptr, long long b) { return row_ptr[b + 1] - row_ptr[b]; }

// dmx_pooled_allowed_mass: the CSR lists of pool-local options
inline Verdict check_allowed(long long B, const int32_t *pool_of_barcode, const int64_t *row_ptr, const int64_t *allowed_start,
                             const int32_t *allowed_options)
{
    if (!allowed_start) return {INVALID, "null allowed_start", -1};
    if (allowed_start[0] != 0) return {INVALID, "allowed_start[0] is not 0", -1, (long long)allowed_start[0]};
    for (long long b = 0; b < B; b++)
        if (allowed_start[b + 1] < allowed_start[b]) return {INVALID, "allowed_start decreases at a barcode", b};
    if (allowed_start[B] > 0 && !allowed_options) return {INVALID, "null allowed_options", -1};
    for (long long b = 0; b < B; b++) {
        if (allowed_start[b + 1] == allowed_start[b]) continue;
        if (pool_of_barcode[b] < 0) return {INVALID, "a barcode in no pool has allowed options", b};
        const long long K = row_options(row_ptr, b);
        for (long long j = allowed_start[b]; j < allowed_start[b + 1]; j++)
            if (allowed_options[j] < 0 || allowed_options[j] >= K) return {INVALID, "an allowed option is outside its barcode's row", j, (long long)allowed_options[j]};
    }
    return {OK, "", -1};
}

// dmx_pooled_get: barcodes [b0, b1) of matrix `what`
inline Verdict check_get(long long B, int what, const bool (&present)[N_WHAT], long long b0, long long b1)
{
    if (what < 0 || what >= N_WHAT) return {INVALID, "what is not 0 (logits), 1 (probs), 2 (alpha_index) or 3 (alpha_mean)", -1, what};
    if (!present[what]) return {INVALID, "the kept result does not hold that matrix", -1, what};
    if (b0 < 0 || b1 < b0 || b1 > B) return {INVALID, "the barcode range is not inside [0, B]", -1};
    return {OK, "", -1};
}

inline Verdict check_get_pool(long long n_pools, int what, const bool (&present)[N_WHAT], long long pool)
{
    if (what < 0 || what >= N_WHAT) return {INVALID, "what is not 0 (logits), 1 (probs), 2 (alpha_index) or 3 (alpha_mean)", -1, what};
    if (!present[what]) return {INVALID, "the kept result does not hold that matrix", -1, what};
    if (pool < 0 || pool >= n_pools) return {INVALID, "the pool is outside [0, n_pools)", -1, pool};
    return {OK, "", -1};
}

inline Verdict check_top(int k)
{
    if (k < 1 || k > TOP_MAX) return {INVALID, "k is outside 1..4", -1, k};
    return {OK, "", -1};
}

// first marginal of every barcode: g_p entries for a barcode of pool p, none for a barcode in no pool
inline void marg_ptr(long long B, const int32_t *pool_of_barcode, const int *pool_size, std::vector<int64_t> &out)
{
    out.assign((size_t)B + 1, 0);
    for (long long b = 0; b < B; b++) out[(size_t)b + 1] = out[(size_t)b] + (pool_of_barcode[b] < 0 ? 0 : pool_size[pool_of_barcode[b]]);
}

// every pool's barcodes in ascending barcode order (a counting sort: stable)
inline void pool_lists(long long B, long long n_pools, const int32_t *pool_of_barcode, std::vector<int64_t> &list_ptr, std::vector<int32_t> &list)
{
    list_ptr.assign((size_t)n_pools + 1, 0);
    for (long long b = 0; b < B; b++)
        if (pool_of_barcode[b] >= 0) list_ptr[(size_t)pool_of_barcode[b] + 1]++;
    for (long long p = 0; p < n_pools; p++) list_ptr[(size_t)p + 1] += list_ptr[(size_t)p];
    list.assign((size_t)list_ptr[(size_t)n_pools], 0);
    std::vector<int64_t> next(list_ptr.begin(), list_ptr.end() - 1);
    for (long long b = 0; b < B; b++)
        if (pool_of_barcode[b] >= 0) list[(size_t)next[(size_t)pool_of_barcode[b]]++] = (int32_t)b;
}

// slab j of a list of n positions: [first, last), as k_option_partial cuts B rows (results.hip); the kernel restates it
struct Slab {
    long long first, last;
};
inline long long slab_rows(long long n) { return (n + SUM_SLABS - 1) / SUM_SLABS; }
inline Slab slab(long long n, int j)
{
    const long long per = slab_rows(n);
    const long long first = (long long)j * per < n ? (long long)j * per : n;  // (a slab past the list is empty at its end)
    return {first, first + per < n ? first + per : n};
}

}  // namespace prplan
}  // namespace dmx
