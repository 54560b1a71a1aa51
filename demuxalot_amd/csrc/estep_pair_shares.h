// estep_pair_shares.h -- the pooled E-step with every pair option summed over a grid of mixing shares (estep_pair_shares.hip;
// dmx_steps.cpp: dmx_estep_pair_shares): a pair's term is p1 w + p2 (1 - w) in place of (p1 + p2) / 2, its logit the
// log of the weighted sum over the grid of w, in dmx_estep_ambient_grid_marginal's order; singlet options are dmx_estep_pools' own.
// The walk is k_estep_pools' with the grid inside it.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "estep_pools.h"

struct dmx_ctx;

namespace dmx {

// argument block of k_estep_pair_shares: k_estep_pools' (its `dense` is not used) and what the grid adds
struct PairSharesArgs {
    PoolEstepArgs pools;
    const float *shares;       // [n_shares] the share of a pair's first donor
    const float *log_weights;  // [n_shares] the log of a prior over the grid
    int n_shares;              // 1 .. 64
    int *share_index;          // compact like the logits: the grid point of a pair's largest term; -1: a singlet, or every value NaN
    float *share_mean;         // compact like the logits: a pair's posterior mean share; NaN: a singlet, or every value NaN
};
// the pools of a launch have pair options (with_doublets): there is no form for singlets alone - that is k_estep_pools
hipError_t launch_estep_pair_shares(hipStream_t st, const PairSharesArgs &a, int slots);

// what dmx_estep_pair_shares passes on beside the pools' plan: host pointers
struct PairSharesScoring {
    int n_shares;
    const float *shares;        // [n_shares]
    const float *log_weights;   // nullable [n_shares], absent: all 0
    int32_t *share_index;       // nullable [row_ptr[B]]
    float *share_mean;          // nullable [row_ptr[B]]
    int32_t *best_share_index;  // nullable [B]
    float *best_share_mean;     // nullable [B]
};
// prepare_estep_pools, the kernels (estep_grid.h: run_grid_estep), read_back_estep_pools.  Without doublets: the pooled pass itself, the
// share outputs filled with -1 / NaN on the host, no grid kernel.  The context's pooled slot (dmx_set_keep_pooled) is left alone.
int run_estep_pair_shares(dmx_ctx *c, const PoolsPlan &plan, const PairSharesScoring &scoring);

}  // namespace dmx
