// ambient_profile.hip -- per-barcode ambient RNA fractions (include/demux_hip_debug.h: dmx_ambient_profile).
// For every barcode with an assigned option (a donor or a pair of donors) and every grid value alpha, the log-likelihood of the
// barcode's calls when a share alpha of its molecules comes from the soup:
//   m = q (1 - alpha) + ambient[v] alpha,   L = f32( sum over the calls in stored order of f64( log_f32(m keep + floor) ) )
// with q the exact E-step's term of the option (estep_epilogue.h: estep_terms).  At alpha == 0 the mixture IS that term (q * 1 + a * 0),
// so that column of a singlet is the donor's column of the reference's logits, bit for bit.  One wavefront per barcode as in
// k_estep_pools, with the roles turned round: everything a call contributes is the same for all lanes (q, ambient[v], keep, floor),
// and what differs per lane is the grid value.
#include <hip/hip_runtime.h>

#include <limits>
#include <vector>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "estep_epilogue.h"

namespace dmx {

namespace {

// first maximum, NaN never wins (results.hip: better)
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
constexpr int NO_POINT = 0x7FFFFFFF;

constexpr int CHUNK_CALLS = 64;  // calls a wavefront stages at a time: one per lane

// The calls of one row for this lane's grid value.  o1, o2: byte offsets of the option's columns inside a table row; w0 = 1 - alpha.
// Everything a call contributes is the same for all lanes, but fetching it through the scalar unit - records by scalar loads as
// load_batch has them, then a 4-byte scalar request per table and profile entry, each a miss of the scalar cache - bounded the pass
// at 1.7 x the exact E-step, 2.4 x for pairs (measured).  So the lanes fetch:
// lane l of a chunk of 64 calls loads call l's record fields, table entries and profile entry with vector loads and leaves
// {q, soup, keep, floor} in the wavefront's 1 KB of LDS, laid out per pair of calls as the packed operands; the walk then reads a
// pair's 32 bytes back at a wave-uniform address (a broadcast).  A chunk waits for memory three times, once per 64 calls.
template <bool PAIR>
__device__ __forceinline__ double walk_row(const AmbientArgs &a, const CallPair *__restrict__ recs, int npairs, unsigned o1, unsigned o2, float w0,
                                           float alpha, int lane, float *__restrict__ stage)
{
    double acc = 0.0;
    const int ncalls = 2 * npairs;  // a multiple of 8: rows are padded to 8 calls
    const unsigned *__restrict__ words = (const unsigned *)recs;  // a record: row_off[2], keep[2], floor[2], reserved[2]
    float *__restrict__ mine = stage + (lane >> 1) * 8 + (lane & 1);  // call l of the chunk: slot l & 1 of pair l >> 1
    for (int c0 = 0; c0 < ncalls; c0 += CHUNK_CALLS) {
        const int n = min(CHUNK_CALLS, ncalls - c0);  // wave-uniform, a multiple of 8
        if (lane < n) {
            const unsigned *__restrict__ rec = words + (size_t)((c0 + lane) >> 1) * 8 + (lane & 1);
            // (a padding record - keep 0, floor 1 - points at row 0: whatever finite values it finds there, its term is log 1 = +0)
            const unsigned row_off = rec[0];
            float q = *(const float *)((const char *)a.prob + (row_off + o1));
            if (PAIR) q = (q + *(const float *)((const char *)a.prob + (row_off + o2))) * 0.5f;
            mine[0] = q;
            mine[2] = a.ambient[aplan::row_of(row_off, a.row_shift, a.row_inverse)];
            mine[4] = __uint_as_float(rec[2]);  // keep
            mine[6] = __uint_as_float(rec[4]);  // floor
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
        for (int p = 0; p < n / 2; p++) {
            const float4 lo = *(const float4 *)(stage + p * 8), hi = *(const float4 *)(stage + p * 8 + 4);
            const npm::f32x2 q{lo.x, lo.y}, soup{lo.z, lo.w}, keep{hi.x, hi.y}, flo{hi.z, hi.w};
            const npm::f32x2 own = q * w0;  // two products, one sum, each rounded (-ffp-contract=off)
            const npm::f32x2 other = soup * alpha;
            const npm::f32x2 m = own + other;
            npm::f32x2 t = m * keep;
            t = t + flo;
            const npm::f32x2 lp = npm::log_f32_hot2(t);
            acc += (double)lp.x;  // call order preserved
            acc += (double)lp.y;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next chunk overwrites what this one read)
        __builtin_amdgcn_wave_barrier();
    }
    return acc;
}

// One wavefront per barcode of a.order; lane j holds grid point j, lanes past the grid walk along with alpha = 0 and store nothing.
__global__ __launch_bounds__(256) void k_ambient_profile(AmbientArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.B) return;
    const int b = __builtin_amdgcn_readfirstlane(a.order[slot]);
    const int c1 = __builtin_amdgcn_readfirstlane(a.donor1[b]);
    const int c2 = __builtin_amdgcn_readfirstlane(a.donor2[b]);
    const bool on_grid = lane < a.A;
    const float nan = __builtin_nanf("");
    if (c1 < 0) {  // skipped (wave-uniform)
        if (a.loglik && on_grid) a.loglik[(long long)b * a.A + lane] = nan;
        if (lane == 0) {
            a.best[b] = -1;
            a.ll_best[b] = nan;
            a.ll_zero[b] = nan;
        }
        return;
    }
    const float alpha = on_grid ? a.alphas[lane] : 0.0f;
    const float w0 = 1.0f - alpha;
    const long long pbeg = a.pair_ptr[b];
    const int npairs = (int)(a.pair_ptr[b + 1] - pbeg);
    const CallPair *__restrict__ recs = a.pairs + pbeg;
    const unsigned o1 = (unsigned)c1 * 4u, o2 = (unsigned)c2 * 4u;  // (c2 is read by a pair alone)
    __shared__ __attribute__((aligned(16))) float staged[4][CHUNK_CALLS * 4];
    float *stage = staged[wave];
    const double acc = c2 < 0 ? walk_row<false>(a, recs, npairs, o1, o1, w0, alpha, lane, stage) : walk_row<true>(a, recs, npairs, o1, o2, w0, alpha, lane, stage);
    const float ll = (float)acc;

    float bv = on_grid ? ll : -__builtin_inff();
    int bi = on_grid ? lane : NO_POINT;
    if (!(bv == bv)) bi = NO_POINT;  // (NaN never wins, and is never what a tie is broken against)
    bv = bi == NO_POINT ? -__builtin_inff() : bv;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (a.loglik && on_grid) a.loglik[(long long)b * a.A + lane] = ll;
    const int z = a.zero_column;  // uniform
    const float at_zero = z >= 0 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ll), z)) : nan;
    if (lane == 0) {
        a.best[b] = bi != NO_POINT ? bi : -1;
        a.ll_best[b] = bi != NO_POINT ? bv : nan;
        a.ll_zero[b] = at_zero;
    }
}

// calls per variant from the M-step's work items (runs of one variant's calls): integer additions, so any order gives the count
__global__ __launch_bounds__(256) void k_count_variant_calls(const int *__restrict__ item_variant, const int *__restrict__ item_len,
                                                             long long n_items, long long V, unsigned *__restrict__ count)
{
    const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_items) return;
    const int v = item_variant[it];
    if (v >= 0 && v < V) atomicAdd(count + v, (unsigned)item_len[it]);
}

// beta[v] = f32(count + 1); flags[0] |= 1 where that is not exact
__global__ __launch_bounds__(256) void k_count_betas(const unsigned *__restrict__ count, long long V, float *__restrict__ beta,
                                                     int *__restrict__ flags)
{
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const unsigned c = count[v];
    if (!aplan::count_is_exact(c)) atomicOr(flags, 1);
    beta[v] = (float)(c + 1u);
}

}  // namespace

hipError_t launch_ambient_profile(hipStream_t st, const AmbientArgs &a)
{
    if (a.B == 0) return hipSuccess;
    if (a.A < 1 || a.A > aplan::MAX_ALPHAS || a.zero_column >= a.A) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ambient_profile, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// the soup's profile: the caller's, or the P-step's formula on the call counts (one column: beta[v] = calls of v + 1)
int soup_profile(dmx_ctx *c, scratch::Scratch &sc, const char *who, const float *ambient, float lo, float hi, float **soup)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const long long V = c->V;
    const hipStream_t st = c->stream;
    float *d_soup = nullptr;
    DMX_TRY(sc.get(&d_soup, (size_t)V + 1));
    *soup = d_soup;
    HIP_TRY(hipMemsetAsync(d_soup, 0, sizeof(float) * ((size_t)V + 1), st));
    if (ambient) {
        if (V) HIP_TRY(hipMemcpyAsync(d_soup, ambient, sizeof(float) * (size_t)V, hipMemcpyHostToDevice, st));
    } else if (V) {
        if (c->n_csc != c->N || (c->n_items > 0 && (!c->d_item_variant.p || !c->d_item_len.p)))
            return fail(DMX_ERR_UNSUPPORTED, "%s: the resident M-step records are not this problem's calls; supply `ambient`", who);
        unsigned *d_count = nullptr;
        float *d_beta = nullptr;
        int *d_flags = nullptr;
        DMX_TRY(sc.get(&d_count, (size_t)V));
        DMX_TRY(sc.get(&d_beta, (size_t)V));
        DMX_TRY(sc.get(&d_flags, 1));
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned) * (size_t)V, st));
        HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int), st));
        if (c->n_items > 0) {
            hipLaunchKernelGGL(k_count_variant_calls, dim3(grid_for(c->n_items)), dim3(256), 0, st, c->d_item_variant.p, c->d_item_len.p, c->n_items,
                               V, d_count);
            DMX_TRY(launched("k_count_variant_calls"));
        }
        hipLaunchKernelGGL(k_count_betas, dim3(grid_for(V)), dim3(256), 0, st, d_count, V, d_beta, d_flags);
        DMX_TRY(launched("k_count_betas"));
        int flags = 0;
        HIP_TRY(hipMemcpyAsync(&flags, d_flags, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (flags) return fail(DMX_ERR_UNSUPPORTED, "%s: a variant has 2^24 calls or more: its count is no float32; supply `ambient`", who);
        HIP_TRY(launch_probs_from_betas(st, d_beta, nullptr, c->d_v2snp.p, c->d_snp_ptr.p, c->d_snp_vars.p, 0LL, V, (long long)c->S, 1, nullptr,
                                        lo, hi, d_soup));
    }
    return 0;
}

int run_ambient_profile(dmx_ctx *c, const AmbientPlan &plan)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const long long B = c->B, V = c->V;
    const int A = plan.n_alphas;
    const hipStream_t st = c->stream;
    Scratch sc(c);

    float *d_soup = nullptr;
    DMX_TRY(soup_profile(c, sc, "dmx_ambient_profile", plan.ambient, plan.lo, plan.hi, &d_soup));

    AmbientArgs a = {};
    a.pair_ptr = c->d_pair_ptr.p;
    a.pairs = c->d_call_pairs.p;
    a.order = c->d_bc_order.p;
    a.B = B;
    a.prob = c->d_prob.p;
    a.ambient = d_soup;
    const aplan::RowDivide rows = aplan::row_divide((unsigned)c->G * 4u);
    a.row_shift = rows.shift;
    a.row_inverse = rows.inverse;
    a.A = A;
    a.zero_column = aplan::zero_column(A, plan.alphas);
    float *d_alphas = nullptr;
    int *d_donor1 = nullptr, *d_donor2 = nullptr;
    static_assert(sizeof(int) == sizeof(int32_t), "");
    DMX_TRY(upload(sc, &d_alphas, plan.alphas, (size_t)A, st));
    DMX_TRY(upload(sc, &d_donor1, (const int *)plan.donor1, (size_t)B, st));
    DMX_TRY(upload(sc, &d_donor2, (const int *)plan.donor2, (size_t)B, st));
    a.alphas = d_alphas;
    a.donor1 = d_donor1;
    a.donor2 = d_donor2;
    if (plan.loglik) DMX_TRY(sc.get(&a.loglik, (size_t)B * (size_t)A));
    DMX_TRY(sc.get(&a.best, (size_t)B));
    DMX_TRY(sc.get(&a.ll_best, (size_t)B));
    DMX_TRY(sc.get(&a.ll_zero, (size_t)B));

    {
        TimerSpan ev{nullptr, nullptr};
        SpanGuard ev_guard{c, &ev};
        timer_begin(c, DMX_T_ESTEP, &ev);
        HIP_TRY(launch_ambient_profile(st, a));
        timer_end(c, DMX_T_ESTEP, ev);
    }

    if (plan.loglik && B) HIP_TRY(hipMemcpyAsync(plan.loglik, a.loglik, sizeof(float) * (size_t)B * (size_t)A, hipMemcpyDeviceToHost, st));
    if (plan.best && B) HIP_TRY(hipMemcpyAsync(plan.best, a.best, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (plan.ll_best && B) HIP_TRY(hipMemcpyAsync(plan.ll_best, a.ll_best, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (plan.ll_zero && B) HIP_TRY(hipMemcpyAsync(plan.ll_zero, a.ll_zero, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (plan.ambient_out && V) HIP_TRY(hipMemcpyAsync(plan.ambient_out, d_soup, sizeof(float) * (size_t)V, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the uploads read the caller's arrays, the downloads fill them)
    return 0;
}

}  // namespace dmx
