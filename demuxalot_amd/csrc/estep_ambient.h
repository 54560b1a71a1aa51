// estep_ambient.h -- the pooled E-step under per-barcode ambient RNA fractions (estep_ambient.hip; dmx_steps.cpp: dmx_estep_ambient;
// DESIGN.md 4.7): every option of a barcode's pool is scored with the mixture q (1 - alpha[b]) + ambient[v] alpha[b] in place of the
// option's own term q.  The walk is k_estep_pools', a call's term is k_ambient_profile's.
#pragma once
#include <hip/hip_runtime.h>

#include "estep_pools.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_estep_ambient: k_estep_pools' (its `dense`: the DENSE form only) and what the mixture adds
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
// the block over the context's records and the pools of `view`; device pointers: the fractions [B], the profile [V + 1], the stream
SoupTermArgs soup_term_args(const dmx_ctx *c, const PoolsLaunchView &view, const float *d_alpha, const float *d_soup, float *d_terms);
// dense: the form that also leaves the singlet posteriors in a.pools.dense (learning under ambient fractions: the M-step's input)
hipError_t launch_estep_ambient(hipStream_t st, const AmbientEstepArgs &a, int slots, bool pairs, bool dense = false);

// what dmx_estep_ambient passes on beside the pools' plan: host pointers
struct AmbientScoring {
    float lo, hi;          // the clip of a derived profile
    const float *alpha;    // [B]
    const float *ambient;  // nullable [V]: derived from the resident calls
    float *ambient_out;    // nullable [V]
    const char *who = "dmx_estep_ambient";  // the entry point a refusal of the derived profile names
};
// The device half in three parts, as the pooled pass has them (estep_pools.h), so that a call of several E-steps (dmx_em_ambient)
// pays the pools' round trip, the uploads, the profile and the soup's terms once.
//   prepare    prepare_estep_pools, the profile (given or derived), the fractions, the stream of the soup's terms; `plan` and the
//              arrays of `scoring` outlive the run
//   launch     k_soup_terms in the first pass of a run, then one launch per non-empty bucket (counted in DMX_T_ESTEP).  A dense run
//              writes the singlet posteriors into the context's d_post as [B, G] and leaves the context as the dense pooled pass does
//   read back  the profile, then read_back_estep_pools
// The run holds its temporaries (device_scratch.h) until it is destroyed.
struct AmbientRun;
struct AmbientRunDeleter {
    void operator()(AmbientRun *run) const;
};
typedef std::unique_ptr<AmbientRun, AmbientRunDeleter> AmbientRunPtr;
int prepare_estep_ambient(dmx_ctx *c, const PoolsPlan &plan, const AmbientScoring &scoring, bool dense, AmbientRunPtr &run);
int launch_estep_ambient_pass(dmx_ctx *c, AmbientRun &run, float power);
int read_back_estep_ambient(dmx_ctx *c, AmbientRun &run);
// what the M-step under the same fractions reads of a run (mstep_ambient.hip): device pointers, [B] and [V + 1]
const float *ambient_run_alpha(const AmbientRun &run);
const float *ambient_run_soup(const AmbientRun &run);
// A call that learns the profile (mstep_soup.hip) replaces the run's: d_profile [V + 1], device memory, copied on the stream behind
// whatever still reads the old one; the next pass rebuilds the stream of the soup's terms.  ambient_out then gets the new profile.
int ambient_run_replace_soup(dmx_ctx *c, AmbientRun &run, const float *d_profile);
// the three in a row without the dense form: dmx_estep_ambient
int run_estep_ambient(dmx_ctx *c, const PoolsPlan &plan, const AmbientScoring &scoring);

}  // namespace dmx
