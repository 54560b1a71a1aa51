// mstep_ambient.h -- the M-step under per-barcode ambient RNA fractions (mstep_ambient.hip; dmx_steps.cpp: dmx_mstep_ambient,
// dmx_em_ambient): every call's contribution is weighted by the probability that the call came from the donor and
// not from the soup, r = own / (own + ambient[v] alpha[b]) with own = prob[v, g] (1 - alpha[b]).
#pragma once
#include <hip/hip_runtime.h>

#include "mstep_weighted.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_mstep_ambient and k_mredo_ambient: the shared block (mstep_weighted.h) and what the weight reads
struct AmbientMstepArgs {
    WeightedMstepArgs w;
    const float *ambient;       // [V + 1] the soup's allele profile per variant
    const float *alpha;         // [B] the barcode's fraction
};

// The M-step of the context's posteriors and table into d_add, on the stream: begin_weighted_mstep and run_weighted_mstep
// (mstep_weighted.h) around k_mstep_ambient over every (work item, 64-column word) and k_mredo_ambient over the queue
// k_mcombine_weighted left.  d_alpha [B], d_soup [V + 1]: device memory.
int run_mstep_ambient(dmx_ctx *c, float power, const float *d_alpha, const float *d_soup);
// dmx_mstep_ambient's device half: the uploads, the profile (given or derived), run_mstep_ambient; temporaries go back on return
int run_mstep_ambient_from_host(dmx_ctx *c, float power, const float *alpha, const float *ambient, float lo, float hi);

}  // namespace dmx
