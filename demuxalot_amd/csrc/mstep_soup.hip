// mstep_soup.hip -- the M-step of the soup's allele profile (include/demux_hip_debug.h: dmx_mstep_soup, dmx_em_ambient_soup;
// DESIGN.md 4.18).  For variant v, donor column g and the calls c of v in stored variant-major order, b = cb_c, in float32, every
// operation rounded (-ffp-contract=off):
//   amb = ambient[v] alpha[b];  own = prob[v, g] (1 - alpha[b]);  mix = own + amb;  s = amb == 0 ? 0 : amb / mix      (IEEE division)
//   t = (post[b, g] keep_c) s;   count[v, g] = f32( sum over c of f64(t) )                        one accumulator, in call order
//   total[v] = f32( sum over g ascending of f64(count[v, g]) );   beta[v] = total[v] + pseudo_count
//   ambient'[v] = the P-step's formula on the one column of betas, clipped                        (ambient_profile.hip: soup_profile)
// s is the probability that the call came from the soup and not from the donor: the complement of mstep_ambient.hip's r.  With
// alpha[b] == 0 it is 0 exactly, with alpha[b] == 1 and ambient[v] != 0 it is 1 exactly.  The power is 1 - expected counts -, so a
// posterior is live when it is not 0 (live_floor_float64(1) == 0).  One arithmetic, in the frame of mstep_weighted.h, with the
// counts in the call's scratch and not in the context's addition.  This file holds
//   soup_term           the contract's line for one (call, column)
//   k_mstep_soup        k_mstep_ambient's walk with that line: a wavefront per (work item, 64-column word)
//   k_mredo_soup        the frame's redo of the queued sums with this weight
//   k_soup_totals       total[v] and beta[v]: a thread per variant, a wavefront for more than 64 columns
// All stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "mstep_soup.h"
#include "mstep_weighted_device.h"

namespace dmx {

namespace {

// the contract's line for one (call, column): four roundings, one correctly rounded division, the product
__device__ __forceinline__ float soup_term(float post, float keep, float q, float soup, float alpha)
{
    const float amb = soup * alpha;
    const float own = q * (1.0f - alpha);
    const float mix = own + amb;
    const float s = amb == 0.0f ? 0.0f : amb / mix;  // alpha == 0 (or ambient == 0): no soup in this call; amb != 0: mix >= amb > 0
    return (post * keep) * s;
}

// k_mstep_ambient<true>'s chunk loop (mstep_ambient.hip) with soup_term in place of its weight: lane l owns the float64 accumulator
// of column 64 w + l; a chunk of 64 records is loaded a call per lane; a call whose bitmap word has ONE bit set has its whole
// contribution computed by its own lane, one division per call; the chunk is then added call by call, in order, the owner of the
// call's column adding the broadcast contribution.  A call with several live posteriors in the word is taken by the whole wavefront
// at its place in that order.  A posterior that is not live is 0 and contributes exactly +0: it is not loaded.
__global__ __launch_bounds__(256) void k_mstep_soup(SoupMstepArgs x)
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
        if (one) contribution = soup_term(a.post[(size_t)d.x * a.K + 64 * w + col], keep, s.prob_row[64 * w + col], soup, alpha);
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
                    acc += (double)soup_term(a.post[(size_t)cb * a.K + g], lane_value(keep, i), q_mine, soup, lane_value(alpha, i));
            }
        }
    }
    walk_store(x.w, s, acc);
}

// the weight object of a queued (variant, column): the table entry and the soup's profile are the sum's, the fraction the call's
// (this M-step has one power: the frame's template argument is not looked at)
struct SoupRedoWeight {
    const SoupMstepArgs &x;
    int g;
    float q, soup;
    template <bool SQUARE>
    __device__ __forceinline__ bool call(uint2 d, bool bit, float &c) const
    {
        const MstepArgs &a = x.w.m;
        if (bit) c = soup_term(a.post[(size_t)d.x * a.K + g], __uint_as_float(d.y), q, soup, x.alpha[d.x]);
        return bit;
    }
};

__global__ __launch_bounds__(256) void k_mredo_soup(SoupMstepArgs x)
{
    mredo_weighted<false>(x.w, [&x](long long v, int g) { return SoupRedoWeight{x, g, x.w.prob[(size_t)v * x.w.m.G + g], x.ambient[v]}; });
}

// total[v] = f32 of the float64 sum of count[v, .] in ascending column order, beta[v] = total[v] + pseudo_count.  WAVE: a wavefront
// per variant, four to a block - 64 columns are loaded a column per lane and added one after the other by broadcast, every lane
// carrying the accumulator; else a thread per variant.
template <bool WAVE>
__global__ __launch_bounds__(256) void k_soup_totals(const float *__restrict__ count, long long V, int G, float pseudo_count,
                                                     float *__restrict__ total, float *__restrict__ beta)
{
    if (WAVE) {
        const int lane = threadIdx.x & 63;
        const long long v = wave_slot();
        if (v >= V) return;
        const float *__restrict__ row = count + (size_t)v * G;
        double acc = 0.0;
        for (int g0 = 0; g0 < G; g0 += 64) {
            const int n = min(64, G - g0);  // wave-uniform
            const float mine = lane < n ? row[g0 + lane] : 0.0f;
            for (int i = 0; i < n; i++) acc += (double)lane_value(mine, i);
        }
        if (lane == 0) {
            const float t = (float)acc;
            total[v] = t;
            beta[v] = t + pseudo_count;
        }
    } else {
        const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (v >= V) return;
        const float *__restrict__ row = count + (size_t)v * G;
        double acc = 0.0;
        for (int g = 0; g < G; g++) acc += (double)row[g];
        const float t = (float)acc;
        total[v] = t;
        beta[v] = t + pseudo_count;
    }
}

}  // namespace

// what a call that learns the profile keeps on the device (mstep_soup.h)
struct SoupRun {
    scratch::Scratch sc;
    float pseudo_count, lo, hi;
    float *d_count = nullptr, *d_total = nullptr, *d_beta = nullptr, *d_next = nullptr;
    SoupRun(dmx_ctx *c, float pseudo, float lo_, float hi_) : sc(c), pseudo_count(pseudo), lo(lo_), hi(hi_) {}
};

void SoupRunDeleter::operator()(SoupRun *run) const { delete run; }

int prepare_soup_run(dmx_ctx *c, float pseudo_count, float lo, float hi, SoupRunPtr &run)
{
    const size_t V = (size_t)c->V;
    run.reset(new SoupRun(c, pseudo_count, lo, hi));
    SoupRun &r = *run;
    DMX_TRY(r.sc.get(&r.d_count, V * (size_t)c->G));
    DMX_TRY(r.sc.get(&r.d_total, V));
    DMX_TRY(r.sc.get(&r.d_beta, V));
    DMX_TRY(r.sc.get(&r.d_next, V + 1));
    HIP_TRY(hipMemsetAsync(r.d_total, 0, sizeof(float) * (V ? V : 1), c->stream));
    HIP_TRY(hipMemsetAsync(r.d_next, 0, sizeof(float) * (V + 1), c->stream));  // (entry V stays 0, as soup_profile leaves it)
    return 0;
}

int run_mstep_soup(dmx_ctx *c, SoupRun &r, const float *d_alpha, const float *d_soup)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    const long long V = c->V;
    SoupMstepArgs a = {};
    DMX_TRY(begin_weighted_mstep(c, 1.0f, a.w, r.d_count));
    a.ambient = d_soup;
    a.alpha = d_alpha;
    DMX_TRY(run_weighted_mstep(
        c, a.w, [&a](hipStream_t s) { return launch_walk(s, k_mstep_soup, k_mstep_soup, a); },
        [&a](hipStream_t s) { return launch_by_power(s, dim3(512), k_mredo_soup, k_mredo_soup, a); }));
    if (V == 0) return 0;
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_PSTEP, &ev);
    if (c->G > 64)
        hipLaunchKernelGGL(k_soup_totals<true>, dim3((unsigned)((V + 3) / 4)), dim3(256), 0, st, r.d_count, V, c->G, r.pseudo_count, r.d_total, r.d_beta);
    else
        hipLaunchKernelGGL(k_soup_totals<false>, dim3(grid_for(V)), dim3(256), 0, st, r.d_count, V, c->G, r.pseudo_count, r.d_total, r.d_beta);
    DMX_TRY(launched("k_soup_totals"));
    HIP_TRY(launch_probs_from_betas(st, r.d_beta, nullptr, c->d_v2snp.p, c->d_snp_ptr.p, c->d_snp_vars.p, 0LL, V, (long long)c->S, 1, nullptr, r.lo,
                                    r.hi, r.d_next));
    timer_end(c, DMX_T_PSTEP, ev);
    return 0;
}

const float *soup_run_profile(const SoupRun &run) { return run.d_next; }

int read_back_soup_counts(dmx_ctx *c, SoupRun &r, float *counts_out)
{
    if (counts_out && c->V) HIP_TRY(hipMemcpyAsync(counts_out, r.d_total, sizeof(float) * (size_t)c->V, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int run_mstep_soup_from_host(dmx_ctx *c, const float *alpha, const float *ambient, float pseudo_count, float lo, float hi, float *ambient_out,
                             float *counts_out)
{
    using namespace dmx::scratch;
    Scratch sc(c);
    float *d_soup = nullptr, *d_alpha = nullptr;
    DMX_TRY(soup_profile(c, sc, "dmx_mstep_soup", ambient, lo, hi, &d_soup));
    DMX_TRY(upload(sc, &d_alpha, alpha, (size_t)c->B, c->stream));
    SoupRunPtr run;
    DMX_TRY(prepare_soup_run(c, pseudo_count, lo, hi, run));
    DMX_TRY(run_mstep_soup(c, *run, d_alpha, d_soup));
    if (ambient_out && c->V) HIP_TRY(hipMemcpyAsync(ambient_out, run->d_next, sizeof(float) * (size_t)c->V, hipMemcpyDeviceToHost, c->stream));
    DMX_TRY(read_back_soup_counts(c, *run, counts_out));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the upload read the caller's array, the downloads fill the caller's)
    return 0;
}

}  // namespace dmx
