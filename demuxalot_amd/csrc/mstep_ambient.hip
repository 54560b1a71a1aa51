// mstep_ambient.hip -- the M-step under per-barcode ambient RNA fractions (include/demux_hip_debug.h: dmx_mstep_ambient,
// dmx_em_ambient).  For variant v, donor column g and the calls c of v in stored variant-major order, b = cb_c, in
// float32, every operation rounded (-ffp-contract=off):
//   own = prob[v, g] (1 - alpha[b]);  mix = own + ambient[v] alpha[b];  r = own == 0 ? 0 : own / mix      (IEEE division)
//   w = ((post[b, g] keep_c) r) ^ power;   addition[v, g] = f32( sum over c of f64(w) )                     one accumulator, in call order
// (power 2: one float32 product; another power: the float64 pow of the float32 base, rounded to float32 once)
// r is the probability that the call came from the donor and not from the soup; with alpha[b] == 0 it is 1 exactly (own != 0) and w is
// the plain M-step's.  The weight depends on the table of the iteration, so nothing of the fixed-point, tile-major or incremental
// forms applies: there is one arithmetic, the float64 sum in the reference's order, in the frame of mstep_weighted.h.  This file holds
//   ambient_weight      the contract's line for one (call, column)
//   k_mstep_ambient     a wavefront per (work item, 64-column word) walks the item's records in order and leaves the float64 sum of
//                       every column of its word
//   k_mredo_ambient     the frame's redo of the queued sums with this weight
// Per-call data - the record, alpha[cb], the bitmap word, and for a call with one live posterior in the word (nearly all of them)
// the posterior, the table entry and the whole weight - are fetched and computed a call per lane and broadcast by v_readlane; a
// 4-byte uniform request per call is what bounded dmx_ambient_profile's first form.  All stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "mstep_ambient.h"
#include "mstep_weighted_device.h"

namespace dmx {

namespace {

// the contract's line for one (call, column): three roundings, one correctly rounded division, the product, the power
template <bool SQUARE>
__device__ __forceinline__ float ambient_weight(float post, float keep, float q, float soup, float alpha, float power)
{
    const float own = q * (1.0f - alpha);
    const float mix = own + soup * alpha;
    const float r = own == 0.0f ? 0.0f : own / mix;  // alpha == 1 (and ambient == 0: 0 / 0): a droplet that is all soup teaches nothing
    return power_weight<SQUARE>((post * keep) * r, power);
}

// One wavefront per (item of a.m.order, word w of the G columns): lane l owns the float64 accumulator of column 64 w + l.  A chunk
// of 64 records is loaded a call per lane; a call whose bitmap word has ONE bit set has its whole contribution computed by its own
// lane (one gather of the posterior, one of the table entry); the chunk is then added call by call, in order: the owner of the
// call's column adds the broadcast contribution.  A call with several live posteriors in the word is handled by the whole wavefront
// at its place in that order: its bitmap word is the mask of the row load.  Posteriors that are not live contribute exactly +0
// (r <= 1: kernels.h, NZ_FLOOR_SQUARE) and are not loaded.
template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mstep_ambient(AmbientMstepArgs x)
{
    const MstepArgs &a = x.w.m;
    const int lane = threadIdx.x & 63;
    const int W = (a.G + 63) >> 6;
    const long long slot = wave_slot();
    if (slot >= walk_slots(x.w)) return;
    const WalkSlot s = walk_slot(x.w, slot);
    const int w = s.w, g = s.g;
    const float q_mine = g < a.G ? s.prob_row[g] : 0.0f;
    const float soup = x.ambient[s.v];
    double acc = 0.0;
    for (int c0 = 0; c0 < s.n; c0 += 64) {
        const int ci = c0 + lane;
        uint2 d = make_uint2(0u, 0u);
        float alpha = 0.0f;
        unsigned long long m = 0ull;
        if (ci < s.n) {
            d = s.calls[ci];
            alpha = x.alpha[d.x];
            m = a.nz[(size_t)d.x * W + w];
        }
        const float keep = __uint_as_float(d.y);
        const bool one = m != 0ull && (m & (m - 1ull)) == 0ull;
        const int col = one ? __builtin_ctzll(m) : 0;  // inside the word
        float contribution = 0.0f;
        if (one)
            contribution = ambient_weight<SQUARE>(a.post[(size_t)d.x * a.K + 64 * w + col], keep, s.prob_row[64 * w + col], soup, alpha, a.power);
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
                const unsigned long long bits = lane_value(m, i);
                if ((bits >> lane) & 1ull)
                    acc += (double)ambient_weight<SQUARE>(a.post[(size_t)cb * a.K + g], lane_value(keep, i), q_mine, soup, lane_value(alpha, i), a.power);
            }
        }
    }
    walk_store(x.w, s, acc);
}

// the weight object of a queued (variant, column): the table entry and the soup's profile are the sum's, the fraction the call's
struct AmbientRedoWeight {
    const AmbientMstepArgs &x;
    int g;
    float q, soup;
    template <bool SQUARE>
    __device__ __forceinline__ bool call(uint2 d, bool bit, float &c) const
    {
        const MstepArgs &a = x.w.m;
        if (bit) c = ambient_weight<SQUARE>(a.post[(size_t)d.x * a.K + g], __uint_as_float(d.y), q, soup, x.alpha[d.x], a.power);
        return bit;
    }
};

template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mredo_ambient(AmbientMstepArgs x)
{
    mredo_weighted<SQUARE>(x.w, [&x](long long v, int g) { return AmbientRedoWeight{x, g, x.w.prob[(size_t)v * x.w.m.G + g], x.ambient[v]}; });
}

}  // namespace

int run_mstep_ambient(dmx_ctx *c, float power, const float *d_alpha, const float *d_soup)
{
    AmbientMstepArgs a = {};
    DMX_TRY(begin_weighted_mstep(c, power, a.w));
    a.ambient = d_soup;
    a.alpha = d_alpha;
    return run_weighted_mstep(
        c, a.w, [&a](hipStream_t st) { return launch_walk(st, k_mstep_ambient<true>, k_mstep_ambient<false>, a); },
        [&a](hipStream_t st) { return launch_by_power(st, dim3(512), k_mredo_ambient<true>, k_mredo_ambient<false>, a); });
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
