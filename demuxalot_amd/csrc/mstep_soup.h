// mstep_soup.h -- the M-step of the soup's allele profile (mstep_soup.hip; dmx_steps.cpp: dmx_mstep_soup, dmx_em_ambient_soup;
// DESIGN.md 4.18): every call counts for the soup with the probability that it came from there and not from the donor,
// s = amb / (own + amb) with amb = ambient[v] alpha[b] and own = prob[v, g] (1 - alpha[b]) - the complement of mstep_ambient.h's r.
#pragma once
#include <memory>

#include <hip/hip_runtime.h>

#include "mstep_weighted.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_mstep_soup and k_mredo_soup: the shared block (mstep_weighted.h) and what the weight reads
struct SoupMstepArgs {
    WeightedMstepArgs w;
    const float *ambient;       // [V + 1] the soup's allele profile the E-step of these posteriors read
    const float *alpha;         // [B] the barcode's fraction
};

// What a call that learns the profile keeps on the device (device_scratch.h: held until the run is destroyed): the counts [V, G],
// their totals [V] (zeros until a step has run), the betas [V] and the profile the last step formed [V + 1].
struct SoupRun;
struct SoupRunDeleter {
    void operator()(SoupRun *run) const;
};
typedef std::unique_ptr<SoupRun, SoupRunDeleter> SoupRunPtr;
int prepare_soup_run(dmx_ctx *c, float pseudo_count, float lo, float hi, SoupRunPtr &run);
// One step on the context's posteriors and table, on the stream: begin_weighted_mstep with the run's counts as the output (the
// context's addition and its flags stay as they are; the codes are rebuilt at floor 0 when they were written above it) and
// run_weighted_mstep around k_mstep_soup and k_mredo_soup, then k_soup_totals and the P-step's formula on the one column of betas.
// d_alpha [B], d_soup [V + 1]: device memory, the fractions and the profile the E-step read.
int run_mstep_soup(dmx_ctx *c, SoupRun &run, const float *d_alpha, const float *d_soup);
// the profile the last step formed: device memory, [V + 1]
const float *soup_run_profile(const SoupRun &run);
// the totals of the last step to the host (asynchronous: the caller synchronises); nullable
int read_back_soup_counts(dmx_ctx *c, SoupRun &run, float *counts_out);
// dmx_mstep_soup's device half: the uploads, the profile (given or derived), one step, the read-back; temporaries go back on return
int run_mstep_soup_from_host(dmx_ctx *c, const float *alpha, const float *ambient, float pseudo_count, float lo, float hi, float *ambient_out,
                             float *counts_out);

}  // namespace dmx
