// mstep_weighted.hip -- what the M-steps with a table-dependent weight share outside their kernels (mstep_weighted.h):
//   k_mcombine_weighted   the variants of several work items: the partial sums added in item order, accepted when no float32 rounding
//                         boundary lies within 4 n u S of the total (the rule of kernels.hip: k_mcombine), else queued for the form's redo
// and the host steps around the form's launches: the codes at the float64 floor, the argument block, the context's flags, the timer spans.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dmx_host.h"
#include "mstep_weighted.h"

namespace dmx {

namespace {

// k_mcombine (kernels.hip) for the float64 partials of a weighted walk, always with the redo queue: a thread per (variant, column)
__global__ __launch_bounds__(256) void k_mcombine_weighted(WeightedMstepArgs x)
{
    const MstepArgs &a = x.m;
    const long long total = x.V * a.G;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long v = i / a.G;
        const int g = (int)(i - v * a.G);
        const long long it0 = a.item_ptr[v], it1 = a.item_ptr[v + 1];
        if (it1 - it0 == 1) continue;  // written by the item's own wavefront
        double s = 0.0;
        for (long long it = it0; it < it1; it++) s += a.partial[(size_t)it * a.G + g];
        a.out32[i] = (float)s;  // (a variant without calls: +0; a NaN stands: no order of the additions removes it)
        if (it1 - it0 > 1 && s > 0.0) {
            const long long n = a.item_start[it1 - 1] + a.item_len[it1 - 1] - a.item_start[it0];
            const double bound = 4.0 * (double)n * 1.1102230246251565e-16 * s;
            const float f = (float)s;
            const double lo = 0.5 * ((double)f + (double)nextafterf(f, 0.0f));  // rounding boundary towards zero
            const double hi = 0.5 * ((double)f + (double)nextafterf(f, __builtin_inff()));
            if (!(s - bound > lo && s + bound < hi)) {
                const unsigned at = atomicAdd(&x.n_redo[0], 1u);
                if (at < a.redo_cap) x.redo[at] = ((unsigned long long)v << 16) | (unsigned long long)g;
            }
        }
    }
}

}  // namespace

hipError_t launch_mcombine_weighted(hipStream_t st, const WeightedMstepArgs &a)
{
    const long long total = a.V * a.m.G;
    if (total <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.n_redo, 0, 2 * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(k_mcombine_weighted, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

int begin_weighted_mstep(dmx_ctx *c, float power, WeightedMstepArgs &a, float *out)
{
    // the codes and the bitmap at the floor of a float64 sum (a fixed-point M-step may have asked the E-step for a higher one)
    const float floor = live_floor_float64(power);
    if (c->nz_floor > floor) {
        HIP_TRY(launch_rebuild_nz(c->stream, c->d_post.p, c->B, c->K, c->G, floor, c->d_nz.p, c->G <= 64 ? c->d_first.p : nullptr));
        c->codes_rebuilt(floor);
    }
    a = {};
    a.m.order = c->d_item_order.p;
    a.m.item_start = c->d_item_start.p;
    a.m.item_len = c->d_item_len.p;
    a.m.calls = c->d_csc.p;
    a.m.post = c->d_post.p;
    a.m.nz = c->d_nz.p;
    a.m.K = c->K;
    a.m.post_bytes = (unsigned long long)c->B * (unsigned long long)c->K * 4ull;
    a.m.partial = c->d_partial.p;
    a.m.item_variant = c->d_item_variant.p;
    a.m.item_ptr = c->d_item_ptr.p;
    a.m.out32 = out ? out : c->d_add.p;
    a.m.n_items = c->n_items;
    a.m.G = c->G;
    a.m.square = (power == 2.0f);
    a.m.power = power;
    a.m.redo_cap = c->d_redo.n;
    a.prob = c->d_prob.p;
    a.V = c->V;
    a.redo = c->d_redo.p;
    a.n_redo = c->d_n_redo.p;
    if (!out) c->addition_written_by_other_form();
    return 0;
}

int run_weighted_mstep(dmx_ctx *c, const WeightedMstepArgs &a, const std::function<hipError_t(hipStream_t)> &walk,
                       const std::function<hipError_t(hipStream_t)> &redo)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_MSTEP, &ev);
    HIP_TRY(walk(st));
    c->mstep_form = 1;
    timer_end(c, DMX_T_MSTEP, ev);
    timer_begin(c, DMX_T_MCOMBINE, &ev);
    HIP_TRY(launch_mcombine_weighted(st, a));
    if (a.V * a.m.G > 0) HIP_TRY(redo(st));  // (no sum, no queue)
    timer_end(c, DMX_T_MCOMBINE, ev);
    return 0;
}

}  // namespace dmx
