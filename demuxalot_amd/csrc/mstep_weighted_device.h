// mstep_weighted_device.h -- device inlines of the M-steps with a table-dependent weight (mstep_ambient.hip, mstep_doublets.hip,
// mstep_doublet_shares.hip, mstep_soup.hip): the broadcast of a lane's value, the power of a contribution, the ends of a walk - which (work item, word) a
// wavefront has, where its sums go - and the redo of the queued sums around a form's weight object.  The walks' chunk loops are the forms'.
#pragma once
#include <hip/hip_runtime.h>

#include "mstep_weighted.h"

namespace dmx {

__device__ __forceinline__ float lane_value(float x, int i) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), i)); }
__device__ __forceinline__ unsigned long long lane_value(unsigned long long x, int i)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), i);
    return ((unsigned long long)hi << 32) | lo;
}

// The reference's power of 2 is one float32 product.  Another power is f32(pow(f64(c), f64(power))): a float32 `**` is libm's powf or a
// vector library's in numpy, whichever the host has, and the device's powf is a third (tests/test_gpu_parity.py compares dmx_mstep's
// other powers to float32 accuracy for that reason) - the float64 pow rounded once is what all of them approximate, and what the
// restatements can state.
template <bool SQUARE>
__device__ __forceinline__ float power_weight(float c, float power)
{
    return SQUARE ? c * c : (float)pow((double)c, (double)power);
}

// what a wavefront of a walk has: item `item` of a.m.order, of variant v with n records at `calls`, and word w of the G columns; lane l
// owns the float64 accumulator of column g = 64 w + l, and prob_row is the table's row of v
struct WalkSlot {
    long long item, v;
    int w, n, g;
    const uint2 *__restrict__ calls;
    const float *__restrict__ prob_row;
};

// The slot of this wavefront, four wavefronts to a block, and the number of slots: a wavefront whose slot is not below it has none
// and returns.  (The kernel makes that comparison itself: with the return inside walk_slot the compiler kept a second comparison and
// a second exit, and the walks' code was no longer the code they had before they shared this header.)
__device__ __forceinline__ long long wave_slot() { return (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ long long walk_slots(const WeightedMstepArgs &x) { return x.m.n_items * ((x.m.G + 63) >> 6); }
__device__ __forceinline__ WalkSlot walk_slot(const WeightedMstepArgs &x, long long slot)
{
    const MstepArgs &a = x.m;
    const int lane = threadIdx.x & 63;
    const int W = (a.G + 63) >> 6;
    WalkSlot s;
    const long long islot = slot / W;
    s.w = (int)(slot - islot * W);
    s.item = a.order[islot];
    s.n = a.item_len[s.item];
    s.v = a.item_variant[s.item];
    s.calls = a.calls + a.item_start[s.item];
    s.g = lane + 64 * s.w;
    s.prob_row = x.prob + (size_t)s.v * a.G;
    return s;
}

// the lane's sum: in the addition when the variant has this item only, else in the item's partial row for the combining pass
__device__ __forceinline__ void walk_store(const WeightedMstepArgs &x, const WalkSlot &s, double acc)
{
    const MstepArgs &a = x.m;
    if (s.g >= a.G) return;
    if (a.item_ptr[s.v + 1] - a.item_ptr[s.v] == 1) a.out32[(size_t)s.v * a.G + s.g] = (float)acc;  // (what the combining pass would form: 0.0 + acc)
    else a.partial[(size_t)s.item * a.G + s.g] = acc;
}

// The queued sums as the reference forms them.  A wavefront per (variant, column): 64 calls at a time, a call per lane, then the live
// contributions added in call order into one accumulator that every lane carries.  make(v, g) gives the weight object of a queue
// entry - what the form reads once per sum -, and weight.call<SQUARE>(record, bit, c) says whether the call contributes and leaves its
// contribution in c; bit: the posterior of (barcode, g) is live in the bitmap.
template <bool SQUARE, class MakeWeight>
__device__ __forceinline__ void mredo_weighted(const WeightedMstepArgs &x, MakeWeight make)
{
    const MstepArgs &a = x.m;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int W = (a.G + 63) >> 6;
    const unsigned long long queued = x.n_redo[0];
    const unsigned long long count = queued < a.redo_cap ? queued : a.redo_cap;
    for (unsigned long long e = (unsigned long long)blockIdx.x * 4 + wave; e < count; e += (unsigned long long)gridDim.x * 4) {
        const unsigned long long entry = x.redo[e];
        const long long v = (long long)(entry >> 16);
        const int g = (int)(entry & 0xFFFFull);
        const long long it0 = a.item_ptr[v], it1 = a.item_ptr[v + 1];
        const long long first = a.item_start[it0];
        const long long n = a.item_start[it1 - 1] + a.item_len[it1 - 1] - first;
        const uint2 *__restrict__ calls = a.calls + first;
        const auto weight = make(v, g);
        double acc = 0.0;
        for (long long c0 = 0; c0 < n; c0 += 64) {
            float c = 0.0f;
            bool live = false;
            if (c0 + lane < n) {
                const uint2 d = calls[c0 + lane];
                const bool bit = (a.nz[(size_t)d.x * W + (g >> 6)] >> (g & 63)) & 1ull;
                live = weight.template call<SQUARE>(d, bit, c);
            }
            unsigned long long pending = __ballot(live);
            while (pending) {
                const int i = __builtin_ctzll(pending);
                pending &= pending - 1ull;
                acc += (double)lane_value(c, i);
            }
        }
        if (lane == 0) a.out32[(size_t)v * a.G + g] = (float)acc;
    }
}

// a form's kernel for the reference's power of 2 or for another power: the launch of the one the argument block asks for
template <class Args>
inline hipError_t launch_by_power(hipStream_t st, dim3 grid, void (*squaring)(Args), void (*raising)(Args), const Args &a)
{
    void (*const kernel)(Args) = a.w.m.square ? squaring : raising;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// a form's walk: a wavefront per (work item, 64-column word), four to a block; no slot: nothing to launch; more than a grid holds: refused
template <class Args>
inline hipError_t launch_walk(hipStream_t st, void (*squaring)(Args), void (*raising)(Args), const Args &a)
{
    const long long slots = a.w.m.n_items * ((a.w.m.G + 63) / 64);
    if (slots == 0) return hipSuccess;
    if (slots > 4ll * 0x7FFFFFFF) return hipErrorInvalidValue;
    return launch_by_power(st, dim3((unsigned)((slots + 3) / 4)), squaring, raising, a);
}

}  // namespace dmx
