// mstep_ambient.hip -- the M-step under per-barcode ambient RNA fractions (include/demux_hip_debug.h: dmx_mstep_ambient,
// dmx_em_ambient).  For variant v, donor column g and the calls c of v in stored variant-major order, b = cb_c, in
// float32, every operation rounded (-ffp-contract=off):
//   own = prob[v, g] (1 - alpha[b]);  mix = own + ambient[v] alpha[b];  r = own == 0 ? 0 : own / mix      (IEEE division)
//   w = ((post[b, g] keep_c) r) ^ power;   addition[v, g] = f32( sum over c of f64(w) )                     one accumulator, in call order
// (power 2: one float32 product; another power: the float64 pow of the float32 base, rounded to float32 once)
// r is the probability that the call came from the donor and not from the soup; with alpha[b] == 0 it is 1 exactly (own != 0) and w is
// the plain M-step's.  The weight depends on the table of the iteration, so nothing of the fixed-point, tile-major or incremental
// forms applies: there is one arithmetic, the float64 sum in the reference's order.
//   k_mstep_ambient     a wavefront per (work item, 64-column word) walks the item's records in order and leaves the float64 sum of
//                       every column of its word: in the addition when the variant has this item only, else in the item's partial row
//   k_mcombine_ambient  the variants of several items: the partial sums added in item order, accepted when no float32 rounding
//                       boundary lies within 4 n u S of the total (the rule of kernels.hip: k_mcombine), else queued
//   k_mredo_ambient     a wavefront per queued (variant, column): all calls of the variant, in order, into ONE accumulator
// Per-call data - the record, alpha[cb], the bitmap word, and for a call with one live posterior in the word (nearly all of them)
// the posterior, the table entry and the whole weight - are fetched and computed a call per lane and broadcast by v_readlane; a
// 4-byte uniform request per call is what bounded dmx_ambient_profile's first form.  All stores are plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "mstep_ambient.h"

namespace dmx {

namespace {

// the contract's line for one (call, column): three roundings, one correctly rounded division, the product, the power.  The
// reference's power of 2 is one float32 product.  Another power is f32(pow(f64(c), f64(power))): a float32 `**` is libm's powf or a
// vector library's in numpy, whichever the host has, and the device's powf is a third (tests/test_gpu_parity.py compares
// dmx_mstep's other powers to float32 accuracy for that reason) - the float64 pow rounded once is what all of them approximate, and
// what the restatement can state.
template <bool SQUARE>
__device__ __forceinline__ float ambient_weight(float post, float keep, float q, float soup, float alpha, float power)
{
    const float own = q * (1.0f - alpha);
    const float mix = own + soup * alpha;
    const float r = own == 0.0f ? 0.0f : own / mix;  // alpha == 1 (and ambient == 0: 0 / 0): a droplet that is all soup teaches nothing
    const float c = (post * keep) * r;
    return SQUARE ? c * c : (float)pow((double)c, (double)power);
}

__device__ __forceinline__ float lane_value(float x, int i) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), i)); }

// One wavefront per (item of a.m.order, word w of the G columns): lane l owns the float64 accumulator of column 64 w + l.  A chunk
// of 64 records is loaded a call per lane; a call whose bitmap word has ONE bit set has its whole contribution computed by its own
// lane (one gather of the posterior, one of the table entry); the chunk is then added call by call, in order: the owner of the
// call's column adds the broadcast contribution.  A call with several live posteriors in the word is handled by the whole wavefront
// at its place in that order: its bitmap word is the mask of the row load.  Posteriors that are not live contribute exactly +0
// (r <= 1: kernels.h, NZ_FLOOR_SQUARE) and are not loaded.
template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mstep_ambient(AmbientMstepArgs x)
{
    const MstepArgs &a = x.m;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int G = a.G;
    const int W = (G + 63) >> 6;
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.n_items * W) return;
    const long long islot = slot / W;
    const int w = (int)(slot - islot * W);
    const long long item = a.order[islot];
    const int n = a.item_len[item];
    const long long v = a.item_variant[item];
    const uint2 *__restrict__ calls = a.calls + a.item_start[item];
    const int g = lane + 64 * w;
    const float *__restrict__ prob_row = x.prob + (size_t)v * G;
    const float q_mine = g < G ? prob_row[g] : 0.0f;
    const float soup = x.ambient[v];
    double acc = 0.0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int ci = c0 + lane;
        uint2 d = make_uint2(0u, 0u);
        float alpha = 0.0f;
        unsigned long long m = 0ull;
        if (ci < n) {
            d = calls[ci];
            alpha = x.alpha[d.x];
            m = a.nz[(size_t)d.x * W + w];
        }
        const float keep = __uint_as_float(d.y);
        const bool one = m != 0ull && (m & (m - 1ull)) == 0ull;
        const int col = one ? __builtin_ctzll(m) : 0;  // inside the word
        float contribution = 0.0f;
        if (one)
            contribution = ambient_weight<SQUARE>(a.post[(size_t)d.x * a.K + 64 * w + col], keep, prob_row[64 * w + col], soup, alpha, a.power);
        unsigned long long pending = __ballot(m != 0ull);
        const unsigned long long single = __ballot(one);
        while (pending) {
            const int i = __builtin_ctzll(pending);
            pending &= pending - 1ull;
            if ((single >> i) & 1ull) {  // (wave-uniform)
                const int owner = __builtin_amdgcn_readlane(col, i);
                const float c = lane_value(contribution, i);
                if (lane == owner) acc += (double)c;
            } else {
                const unsigned cb = (unsigned)__builtin_amdgcn_readlane((int)d.x, i);
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)m, i);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(m >> 32), i);
                const unsigned long long bits = ((unsigned long long)hi << 32) | lo;
                if ((bits >> lane) & 1ull)
                    acc += (double)ambient_weight<SQUARE>(a.post[(size_t)cb * a.K + g], lane_value(keep, i), q_mine, soup, lane_value(alpha, i), a.power);
            }
        }
    }
    if (g >= G) return;
    if (a.item_ptr[v + 1] - a.item_ptr[v] == 1) a.out32[(size_t)v * G + g] = (float)acc;  // (what the combining pass would form: 0.0 + acc)
    else a.partial[(size_t)item * G + g] = acc;
}

// k_mcombine (kernels.hip) for the float64 partials of k_mstep_ambient, always with the redo queue: a thread per (variant, column)
__global__ __launch_bounds__(256) void k_mcombine_ambient(AmbientMstepArgs x)
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

// The queued sums as the reference forms them.  A wavefront per (variant, column): 64 calls at a time, a call per lane - record,
// bitmap word, posterior, fraction, weight -, then the live contributions added in call order into one accumulator that every lane
// carries.
template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mredo_ambient(AmbientMstepArgs x)
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
        const float q = x.prob[(size_t)v * a.G + g];
        const float soup = x.ambient[v];
        double acc = 0.0;
        for (long long c0 = 0; c0 < n; c0 += 64) {
            float c = 0.0f;
            bool live = false;
            if (c0 + lane < n) {
                const uint2 d = calls[c0 + lane];
                live = (a.nz[(size_t)d.x * W + (g >> 6)] >> (g & 63)) & 1ull;
                if (live) c = ambient_weight<SQUARE>(a.post[(size_t)d.x * a.K + g], __uint_as_float(d.y), q, soup, x.alpha[d.x], a.power);
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

}  // namespace

hipError_t launch_mstep_ambient(hipStream_t st, const AmbientMstepArgs &a)
{
    const long long W = (a.m.G + 63) / 64;
    const long long slots = a.m.n_items * W;
    if (slots == 0) return hipSuccess;
    if (slots > 4ll * 0x7FFFFFFF) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((slots + 3) / 4)), block(256);
    if (a.m.square)
        hipLaunchKernelGGL((k_mstep_ambient<true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_mstep_ambient<false>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mcombine_ambient(hipStream_t st, const AmbientMstepArgs &a)
{
    const long long total = a.V * a.m.G;
    if (total <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.n_redo, 0, 2 * sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(k_mcombine_ambient, dim3(grid), dim3(256), 0, st, a);
    if (a.m.square)
        hipLaunchKernelGGL((k_mredo_ambient<true>), dim3(512), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_mredo_ambient<false>), dim3(512), dim3(256), 0, st, a);
    return hipGetLastError();
}

int run_mstep_ambient(dmx_ctx *c, float power, const float *d_alpha, const float *d_soup)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    // the codes and the bitmap at the floor of a float64 sum (a fixed-point M-step may have asked the E-step for a higher one)
    const float floor = live_floor_float64(power);
    if (c->nz_floor > floor) {
        HIP_TRY(launch_rebuild_nz(st, c->d_post.p, c->B, c->K, c->G, floor, c->d_nz.p, c->G <= 64 ? c->d_first.p : nullptr));
        c->nz_floor = floor;
        c->post_gathered = false;
        c->nz_rebuilds++;
    }
    AmbientMstepArgs a = {};
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
    a.m.out32 = c->d_add.p;
    a.m.n_items = c->n_items;
    a.m.G = c->G;
    a.m.square = (power == 2.0f);
    a.m.power = power;
    a.m.redo_cap = c->d_redo.n;
    a.prob = c->d_prob.p;
    a.ambient = d_soup;
    a.alpha = d_alpha;
    a.V = c->V;
    a.redo = c->d_redo.p;
    a.n_redo = c->d_n_redo.p;
    c->add_is_zero = false;
    c->add_partial = false;
    c->incr_valid = false;  // (another form writes the addition: the kept fixed-point sums no longer describe it)
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_MSTEP, &ev);
    HIP_TRY(launch_mstep_ambient(st, a));
    c->mstep_form = 1;
    timer_end(c, DMX_T_MSTEP, ev);
    timer_begin(c, DMX_T_MCOMBINE, &ev);
    HIP_TRY(launch_mcombine_ambient(st, a));
    timer_end(c, DMX_T_MCOMBINE, ev);
    return 0;
}

int run_mstep_ambient_from_host(dmx_ctx *c, float power, const float *alpha, const float *ambient, float lo, float hi)
{
    using namespace dmx::scratch;
    Scratch sc(c);
    float *d_soup = nullptr, *d_alpha = nullptr;
    DMX_TRY(soup_profile(c, sc, "dmx_mstep_ambient", ambient, lo, hi, &d_soup));
    DMX_TRY(upload(sc, &d_alpha, alpha, (size_t)c->B, c->stream));
    DMX_TRY(run_mstep_ambient(c, power, d_alpha, d_soup));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the upload read the caller's array)
    return 0;
}

}  // namespace dmx
