// ambient_profile.h -- per-barcode ambient RNA fractions (ambient_profile.hip; dmx_steps.cpp: dmx_ambient_profile):
// the log-likelihood of every barcode's calls under its assigned donor(s) mixed with the soup's allele profile, on a grid of
// contamination fractions, in one pass over the resident call records and the resident genotype table.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "ambient_plan.h"
#include "kernels.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_ambient_profile: one wavefront per barcode of `order`, lane j = grid point j
struct AmbientArgs {
    const long long *pair_ptr;  // [B + 1] the resident problem's records, as EstepArgs has them (read by vector loads, a call per lane)
    const CallPair *pairs;
    const int *order;           // [B] barcodes by decreasing row length
    long long B;
    const float *prob;          // [V, G]
    const float *ambient;       // [V + 1] the soup's allele profile per table row
    unsigned row_shift, row_inverse;  // aplan::row_divide(4 G): a record's row offset -> its table row
    const float *alphas;        // [A]
    int A;                      // 1 .. 64
    int zero_column;            // aplan::zero_column, -1: the grid has no 0
    const int *donor1, *donor2; // [B] table columns: (-1, .) skipped, (d, -1) a singlet, d1 < d2 a pair
    float *loglik;              // nullable [B, A]
    int *best;                  // [B]
    float *ll_best, *ll_zero;   // [B]
};
hipError_t launch_ambient_profile(hipStream_t st, const AmbientArgs &a);

// what dmx_ambient_profile has validated (aplan::check): host pointers, outputs nullable
struct AmbientPlan {
    float lo, hi;  // the clip of a derived profile
    int n_alphas;
    const float *alphas;
    const int32_t *donor1, *donor2;
    const float *ambient;  // nullable: derived from the resident calls
    float *loglik;
    int32_t *best;
    float *ll_best, *ll_zero, *ambient_out;
};
// uploads, the profile (given or derived), the pass (counted in DMX_T_ESTEP), the read-back; temporaries go back on return.
// DMX_ERR_UNSUPPORTED where a variant has 2^24 calls or more (the derived profile's counts are float32).
int run_ambient_profile(dmx_ctx *c, const AmbientPlan &plan);

namespace scratch {
struct Scratch;
}
// The soup's profile on the device, [V + 1] floats of `sc` (one entry past the variants, 0: what a padding record's row may find):
// the caller's `ambient`, or, for NULL, the one derived from the resident calls as dmx_ambient_profile defines it.  Shared by
// dmx_ambient_profile and dmx_estep_ambient (estep_ambient.hip); `who` names the entry point in a refusal.
int soup_profile(dmx_ctx *c, scratch::Scratch &sc, const char *who, const float *ambient, float lo, float hi, float **soup);

}  // namespace dmx
