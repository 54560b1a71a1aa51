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

// argument block of k_estep_pair_shares: k_estep_pools' (its `dense` is written by the DENSE form alone) and what the grid adds
struct PairSharesArgs {
    PoolEstepArgs pools;
    const float *shares;       // [n_shares] the share of a pair's first donor
    const float *log_weights;  // [n_shares] the log of a prior over the grid
    int n_shares;              // 1 .. 64
    int *share_index;          // compact like the logits: the grid point of a pair's largest term; -1: a singlet, or every value NaN
    float *share_mean;         // compact like the logits: a pair's posterior mean share; NaN: a singlet, or every value NaN
};
// the pools of a launch have pair options (with_doublets): there is no form for singlets alone - that is k_estep_pools
// dense: the form that also leaves the singlet posteriors in a.pools.dense (learning under shares: the M-step's input)
hipError_t launch_estep_pair_shares(hipStream_t st, const PairSharesArgs &a, int slots, bool dense = false);

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

// The dense pass in three parts, as estep_ambient.h has its own, so that a call of several E-steps (dmx_em_doublet_shares) pays the host
// round trip once and share_mean stays on the device for the M-step between two of them (mstep_doublet_shares.h).
//   prepare    prepare_estep_pools (dense), the grid and the prior uploaded, the four grid outputs; `plan` outlives the run
//   launch     the DENSE kernels into the context's own d_post as [B, G] (the caller has begun the dense pass: dmx_steps.cpp),
//              the best option's entries, close_dense_pools_pass with the floor of `power`.  Without doublets: the dense pooled
//              pass itself, no grid kernel
//   read back  the share outputs (-1 / NaN on the host without doublets), then read_back_estep_pools
struct PairSharesRun;
struct PairSharesRunDeleter {
    void operator()(PairSharesRun *run) const;
};
typedef std::unique_ptr<PairSharesRun, PairSharesRunDeleter> PairSharesRunPtr;
int prepare_pair_shares_run(dmx_ctx *c, const PoolsPlan &plan, const PairSharesScoring &scoring, PairSharesRunPtr &run);
int launch_pair_shares_pass(dmx_ctx *c, PairSharesRun &run, float power);
int read_back_pair_shares(dmx_ctx *c, PairSharesRun &run);
// the prepared pooled run inside it, and the compact share_mean on the device (null without doublets)
const PoolsRun &pair_shares_run_pools(const PairSharesRun &run);
const float *pair_shares_run_mean(const PairSharesRun &run);

}  // namespace dmx
