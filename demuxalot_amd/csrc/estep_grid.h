// estep_grid.h -- the host frame of the pooled E-steps over a grid (estep_grid.hip; the forms: estep_ambient_grid.h, estep_pair_shares.h;
// DESIGN.md 4.16): the prior over the grid on the device, the four outputs a grid adds to a pooled pass, and the launches of one pass
// around a form's own.  The kernels' shared device code is estep_grid_device.h.
#pragma once
#include <functional>

#include <hip/hip_runtime.h>

#include "device_scratch.h"
#include "estep_pools.h"

namespace dmx {

// [n] the log of a prior over the grid, from the caller's array; absent means all 0, which adds nothing anywhere (x + 0.0f is x in
// every comparison and sum of the fold)
int upload_log_weights(scratch::Scratch &sc, float **out, const float *log_weights, int n, hipStream_t st);

// What a grid adds to a pooled pass, on the device: per option (compact like the logits) the grid point a form reports and, in the
// forms that sum the grid, the posterior mean over it; per barcode the two entries of its best option, -1 / NaN where there is none.
struct GridOutputs {
    int *index = nullptr, *best_index = nullptr;
    float *mean = nullptr, *best_mean = nullptr;  // null: a pass without means
    int get(scratch::Scratch &sc, size_t n_values, size_t B, bool with_mean);
    // into the caller's arrays, each nullable (a mean of a pass without means is not asked for)
    int download(hipStream_t st, size_t n_values, size_t B, int32_t *index_out, float *mean_out, int32_t *best_index_out, float *best_mean_out) const;
};

// One pass on the context's stream, in one span of DMX_T_ESTEP: `before` (may be empty), `launch` once per bucket of the prepared run
// with the pools' block filled for that bucket and its option slots, then the gather of the best option's entries into out.best_*
int run_grid_estep(dmx_ctx *c, const PoolsLaunchView &view, const GridOutputs &out, const std::function<hipError_t(hipStream_t)> &before,
                   const std::function<hipError_t(hipStream_t, const PoolEstepArgs &, int slots)> &launch);

}  // namespace dmx
