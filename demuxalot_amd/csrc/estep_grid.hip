// estep_grid.hip -- what the pooled E-steps over a grid share outside their kernels (estep_grid.h):
//   k_best_of_grid   the best option's entry of a compact int32 and, WITH_MEAN, a compact float32 array, whatever they hold: a thread
//                    per barcode, -1 / NaN where best[b] is -1 or the barcode is in no pool
// and the host steps around a form's launches: the prior over the grid, the four outputs, the bucket loop inside the timer's span.
#include "estep_grid.h"

namespace dmx {

namespace {

template <bool WITH_MEAN>
__global__ __launch_bounds__(256) void k_best_of_grid(long long B, const int *__restrict__ pool_of, const long long *__restrict__ row_ptr,
                                                      const int *__restrict__ best, const int *__restrict__ index, const float *__restrict__ mean,
                                                      int *__restrict__ best_index, float *__restrict__ best_mean)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int j = -1;
    float m = __builtin_nanf("");
    if (pool_of[b] >= 0) {  // (nothing has written best[b] of a barcode in no pool)
        const int k = best[b];
        if (k >= 0) {
            j = index[row_ptr[b] + k];
            if (WITH_MEAN) m = mean[row_ptr[b] + k];
        }
    }
    best_index[b] = j;
    if (WITH_MEAN) best_mean[b] = m;
}

}  // namespace

int upload_log_weights(scratch::Scratch &sc, float **out, const float *log_weights, int n, hipStream_t st)
{
    if (log_weights) return scratch::upload(sc, out, log_weights, (size_t)n, st);
    DMX_TRY(sc.get(out, (size_t)n));
    HIP_TRY(hipMemsetAsync(*out, 0, sizeof(float) * (size_t)n, st));  // (all bits 0: +0.0f)
    return 0;
}

int GridOutputs::get(scratch::Scratch &sc, size_t n_values, size_t B, bool with_mean)
{
    DMX_TRY(sc.get(&index, n_values));
    DMX_TRY(sc.get(&best_index, B));
    if (!with_mean) return 0;
    DMX_TRY(sc.get(&mean, n_values));
    return sc.get(&best_mean, B);
}

int GridOutputs::download(hipStream_t st, size_t n_values, size_t B, int32_t *index_out, float *mean_out, int32_t *best_index_out, float *best_mean_out) const
{
    if (index_out && n_values) HIP_TRY(hipMemcpyAsync(index_out, index, sizeof(int) * n_values, hipMemcpyDeviceToHost, st));
    if (mean_out && n_values) HIP_TRY(hipMemcpyAsync(mean_out, mean, sizeof(float) * n_values, hipMemcpyDeviceToHost, st));
    if (best_index_out && B) HIP_TRY(hipMemcpyAsync(best_index_out, best_index, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    if (best_mean_out && B) HIP_TRY(hipMemcpyAsync(best_mean_out, best_mean, sizeof(float) * B, hipMemcpyDeviceToHost, st));
    return 0;
}

int run_grid_estep(dmx_ctx *c, const PoolsLaunchView &view, const GridOutputs &out, const std::function<hipError_t(hipStream_t)> &before,
                   const std::function<hipError_t(hipStream_t, const PoolEstepArgs &, int slots)> &launch)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    PoolEstepArgs pools = view.args;
    pools.dense = nullptr;
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);
    if (before) HIP_TRY(before(st));
    for (int k = 0; k < POOL_BUCKETS; k++) {
        pools.list = view.lists[k];
        pools.n_list = view.n_lists[k];
        HIP_TRY(launch(st, pools, pool_bucket_slots(k)));
    }
    if (c->B > 0) {
        const dim3 grid(scratch::grid_for(c->B)), block(256);
        hipLaunchKernelGGL(out.mean ? k_best_of_grid<true> : k_best_of_grid<false>, grid, block, 0, st, c->B, pools.pool_of, pools.row_ptr, pools.best,
                           out.index, out.mean, out.best_index, out.best_mean);
        HIP_TRY(hipGetLastError());
    }
    timer_end(c, DMX_T_ESTEP, ev);
    return 0;
}

}  // namespace dmx
