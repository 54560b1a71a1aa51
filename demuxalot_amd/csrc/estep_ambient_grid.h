// estep_ambient_grid.h -- the pooled E-step with every option scored at its own best ambient fraction (estep_ambient_grid.hip;
// dmx_steps.cpp: dmx_estep_ambient_grid): dmx_estep_ambient's term on a grid of fractions, the maximum over the grid
// per option, one softmax over those maxima.  The walk is k_estep_ambient's with the grid inside it.
// dmx_estep_ambient_grid_marginal: the same pass with the log of the weighted sum over the grid in place of the maximum.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "estep_pools.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_estep_ambient_grid: k_estep_pools' (its `dense` is not used) and what the grid adds
struct AmbientGridArgs {
    PoolEstepArgs pools;
    const float2 *soup;   // [n_pairs] beside the records: ambient[row] of a record's two calls (k_soup_terms with a fraction of 1)
    const float *alphas;  // [n_alphas]
    int n_alphas;         // 1 .. 64
    int *alpha_index;     // compact like the logits: the grid point of an option's first maximum, -1: every value NaN
    float *profile;       // the PROFILE form only: [row_ptr[B], n_alphas] every option's logit at every grid point
    const float *log_weights;  // the MARGINAL forms only: [n_alphas] the log of a prior over the grid
    float *alpha_mean;         // the MARGINAL forms only: compact like the logits: an option's posterior mean fraction, NaN: every value NaN
};
// profile: the form that also stores a.profile; marginal (never with profile): the grid summed, a.alpha_index its
// first maximum of lambda + log_weights
hipError_t launch_estep_ambient_grid(hipStream_t st, const AmbientGridArgs &a, int slots, bool pairs, bool profile, bool marginal);

// what dmx_estep_ambient_grid passes on beside the pools' plan: host pointers
struct AmbientGridScoring {
    float lo, hi;               // the clip of a derived profile
    int n_alphas;
    const float *alphas;        // [n_alphas]
    const float *ambient;       // nullable [V]: derived from the resident calls
    float *ambient_out;         // nullable [V]
    int32_t *alpha_index;       // nullable [row_ptr[B]]
    int32_t *best_alpha_index;  // nullable [B]
    float *profile_out;         // nullable [row_ptr[B], n_alphas]; not looked at under `marginal`
    bool marginal;              // dmx_estep_ambient_grid_marginal: the sum over the grid in place of its maximum
    const float *log_weights;   // marginal: nullable [n_alphas], absent: all 0
    float *alpha_mean;          // marginal: nullable [row_ptr[B]]
    float *best_alpha_mean;     // marginal: nullable [B]
};
// prepare_estep_pools, the profile (given or derived), the kernels (estep_grid.h: run_grid_estep), read_back_estep_pools
int run_estep_ambient_grid(dmx_ctx *c, const PoolsPlan &plan, const AmbientGridScoring &scoring);

}  // namespace dmx
