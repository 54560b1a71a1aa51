// mstep_ambient.h -- the M-step under per-barcode ambient RNA fractions (mstep_ambient.hip; dmx_steps.cpp: dmx_mstep_ambient,
// dmx_em_ambient): every call's contribution is weighted by the probability that the call came from the donor and
// not from the soup, r = own / (own + ambient[v] alpha[b]) with own = prob[v, g] (1 - alpha[b]).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_mstep_ambient, k_mcombine_ambient and k_mredo_ambient: the work items, the records, the posteriors and the
// bitmap of MstepArgs (float64 form: partial, item_variant, item_ptr, out32, redo_cap; nothing of the fixed-point or tile forms),
// and what the weight reads
struct AmbientMstepArgs {
    MstepArgs m;
    const float *prob;          // [V, G] the genotype table the E-step of these posteriors read
    const float *ambient;       // [V + 1] the soup's allele profile per variant
    const float *alpha;         // [B] the barcode's fraction
    long long V;
    unsigned long long *redo;   // [m.redo_cap] (variant << 16 | genotype) of the sums to be redone in call order
    unsigned *n_redo;           // [2] their number, and 0 (the context's two counters, zeroed by the launcher: dmx_get_redo_count adds them)
};
// k_mstep_ambient over every (work item, 64-column word), k_mcombine_ambient over [V, G], k_mredo_ambient over the queue
hipError_t launch_mstep_ambient(hipStream_t st, const AmbientMstepArgs &a);
hipError_t launch_mcombine_ambient(hipStream_t st, const AmbientMstepArgs &a);

// The M-step of the context's posteriors (d_post, singlet columns; d_nz) and table (d_prob) into d_add, on the stream: the codes
// are rebuilt first when they were written above live_floor_float64(power); the walk is counted in DMX_T_MSTEP, the combining pass
// and the redo in DMX_T_MCOMBINE.  d_alpha [B], d_soup [V + 1]: device memory.  Leaves the context as run_mstep's float64 form does.
int run_mstep_ambient(dmx_ctx *c, float power, const float *d_alpha, const float *d_soup);
// dmx_mstep_ambient's device half: the uploads, the profile (given or derived), run_mstep_ambient; temporaries go back on return
int run_mstep_ambient_from_host(dmx_ctx *c, float power, const float *alpha, const float *ambient, float lo, float hi);

}  // namespace dmx
