// estep_ambient.h -- the pooled E-step under per-barcode ambient RNA fractions (estep_ambient.hip; dmx_steps.cpp: dmx_estep_ambient;
// DESIGN.md 4.7): every option of a barcode's pool is scored with the mixture q (1 - alpha[b]) + ambient[v] alpha[b] in place of the
// option's own term q.  The walk is k_estep_pools', a call's term is k_ambient_profile's.
#pragma once
#include <hip/hip_runtime.h>

#include "estep_pools.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_estep_ambient: k_estep_pools' (its `dense` is not used) and what the mixture adds
struct AmbientEstepArgs {
    PoolEstepArgs pools;
    const float *alpha;       // [B] the barcode's fraction
    const float2 *soup_term;  // [n_pairs] beside the records: f32(ambient[row] * alpha[b]) of a record's two calls (k_soup_terms)
};

// argument block of k_soup_terms: one wavefront per barcode of `order`, a call per lane
struct SoupTermArgs {
    const long long *pair_ptr;  // [B + 1]
    const CallPair *pairs;
    const int *order;           // [B] barcodes by decreasing row length
    long long B;
    const int *pool_of;         // [B] -1: in no pool - nothing is read of alpha[b], nothing is written
    const float *alpha;         // [B]
    const float *ambient;       // [V + 1] the soup's allele profile per table row
    unsigned row_shift, row_inverse;  // aplan::row_divide(4 G)
    float *soup_term;           // [2 n_pairs]
};
hipError_t launch_soup_terms(hipStream_t st, const SoupTermArgs &a);
hipError_t launch_estep_ambient(hipStream_t st, const AmbientEstepArgs &a, int slots, bool pairs);

// what dmx_estep_ambient passes on beside the pools' plan: host pointers
struct AmbientScoring {
    float lo, hi;          // the clip of a derived profile
    const float *alpha;    // [B]
    const float *ambient;  // nullable [V]: derived from the resident calls
    float *ambient_out;    // nullable [V]
};
// prepare_estep_pools, the profile (given or derived), the two kernels (counted in DMX_T_ESTEP), read_back_estep_pools
int run_estep_ambient(dmx_ctx *c, const PoolsPlan &plan, const AmbientScoring &scoring);

}  // namespace dmx
