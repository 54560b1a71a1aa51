// results.hip -- device-side reductions of the posterior matrix, so that the [B, K] result need not cross
// PCIe (4.3 GB per rank at 130k barcodes x 8256 options) when the caller only wants what users of the reference
// take from the DataFrame:
//   probs[probs.max(axis=1).gt(thr)].idxmax(axis=1)   examples/2-with-detection-of-new-SNPs.ipynb cell 14,
//                                                     demuxalot/snp_detection.py:166
//   probs[genotype_names].sum()                       same notebook, cells 19 / 21
//   the few best options of each barcode (singlet vs doublet calls)
//   the pair columns of a doublet run folded back onto donors: singlet / doublet mass, best singlet and pair, donor marginals
//   the posterior of each barcode's possible options       demuxalot/utils.py:265-296 (_compute_qualities)
#include <hip/hip_runtime.h>

#include "device_scratch.h"

namespace {

using namespace dmx::scratch;

constexpr int TOP_MAX = 4;

// (value, column) ordering of the reductions: larger value first, lower column first among equals -- the first
// maximum, as DataFrame.idxmax / np.argmax return it; NaNs never win (as `v > best` is false for them).
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// One wavefront per barcode: the TOP best options, best first.  Each lane keeps the TOP best of its own columns
// (sorted registers, unrolled insertion), then TOP rounds of a wave-wide arg-max pop the lanes' heads.
template <int TOP>
__global__ __launch_bounds__(256) void k_top_options(const float *__restrict__ post, long long B, int K, float threshold,
                                                     int *__restrict__ best, float *__restrict__ best_p,
                                                     unsigned long long *__restrict__ n_above)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float *row = post + (size_t)b * K;
    float v[TOP];
    int ix[TOP];
#pragma unroll
    for (int t = 0; t < TOP; t++) {
        v[t] = -__builtin_inff();
        ix[t] = 0x7FFFFFFF;
    }
    for (int k = lane; k < K; k += 64) {
        float x = row[k];
        int xi = k;
        if (x != x) continue;  // NaN: never selected
#pragma unroll
        for (int t = 0; t < TOP; t++) {
            if (better(x, xi, v[t], ix[t])) {  // insert here, push the rest down
                const float tv = v[t];
                const int ti = ix[t];
                v[t] = x;
                ix[t] = xi;
                x = tv;
                xi = ti;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TOP; r++) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi == ix[0] && bi != 0x7FFFFFFF) {  // the winning lane pops its head
#pragma unroll
            for (int t = 0; t + 1 < TOP; t++) {
                v[t] = v[t + 1];
                ix[t] = ix[t + 1];
            }
            v[TOP - 1] = -__builtin_inff();
            ix[TOP - 1] = 0x7FFFFFFF;
        }
        if (lane == 0) {
            const bool have = bi != 0x7FFFFFFF;
            if (TOP == 1) {
                // thresholded assignment: -1 unless the best posterior is strictly above the threshold (Series.gt)
                const bool ok = have && bv > threshold;
                best[b] = ok ? bi : -1;
                best_p[b] = have ? bv : __builtin_nanf("");
                if (ok && n_above) atomicAdd(n_above, 1ull);
            } else {
                best[(size_t)b * TOP + r] = have ? bi : -1;
                best_p[(size_t)b * TOP + r] = have ? bv : __builtin_nanf("");
            }
        }
    }
}

// Column sums over barcodes in two deterministic passes: float64 partial sums of row slabs, then the slabs in
// order.  (pandas adds float32 values row by row; the float64 sums here are at least as accurate.)
constexpr int SUM_SLABS = 512;
__global__ __launch_bounds__(256) void k_option_partial(const float *__restrict__ post, long long B, int K,
                                                        double *__restrict__ partial)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const long long per = (B + SUM_SLABS - 1) / SUM_SLABS;
    const long long b0 = (long long)blockIdx.y * per;
    const long long b1 = b0 + per < B ? b0 + per : B;
    if (k >= K) return;
    double s = 0.0;
    for (long long b = b0; b < b1; b++) s += (double)post[(size_t)b * K + k];
    partial[(size_t)blockIdx.y * K + k] = s;
}

__global__ __launch_bounds__(256) void k_option_final(const double *__restrict__ partial, int K, double *__restrict__ sums)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int j = 0; j < SUM_SLABS; j++) s += partial[(size_t)j * K + k];
    sums[k] = s;
}

// ---- donor-level read-out -----------------------------------------------------------------------------------
// The pair columns folded back onto donors in one pass over the matrix.  Columns: singlets 0 .. G-1, then pair (g1 < g2) at
// G + g1 (2G - g1 - 1) / 2 + (g2 - g1 - 1); K == G: no pair columns.  A TEAM of 64 (one wavefront; four barcodes per workgroup)
// or 256 threads (the workgroup) takes one barcode:
//   1. its row comes in with coalesced loads; on the way every thread adds its singlet and pair columns in float64 and keeps
//      the first maximum (better()) of either kind, and with STAGE the row is left in LDS;
//   2. the team's partial results are combined in a fixed order (xor shuffles inside a wavefront, then the wavefronts 0 .. 3);
//   3. MARG: thread g adds the columns that contain donor g, widened to float64, in ASCENDING COLUMN ORDER - singlet g,
//      (0, g) .. (g-1, g), (g, g+1) .. (g, G-1): G terms for every donor, so the threads finish together - and rounds once.
//      The order is the contract (no atomics): the result is that of the sequential loop, bit for bit.
// STAGE false reads step 3 from global memory in the same order (rows beyond DONOR_LDS_ROW floats).
constexpr int DONOR_LDS_ROW = 256 * 33;  // floats of a row staged in LDS: the doublets of 128 donors (8256), 33 KB
constexpr int NO_COLUMN = 0x7FFFFFFF;

struct DonorOut {
    double *singlet_mass, *doublet_mass;
    int *best_singlet, *best_pair;
    float *best_singlet_prob, *best_pair_prob;
    float *marginals;
};

template <int TEAM, bool MARG, bool STAGE>
__global__ __launch_bounds__(256) void k_donor_readout(const float *__restrict__ post, long long B, int K, int G, DonorOut o)
{
    extern __shared__ float staged_rows[];
    __shared__ double w_s[4], w_d[4];
    __shared__ float w_sv[4], w_pv[4];
    __shared__ int w_si[4], w_pi[4];
    constexpr int TEAMS = 256 / TEAM;
    const int team = threadIdx.x / TEAM, t = threadIdx.x % TEAM, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = (long long)blockIdx.x * TEAMS + team;
    const bool live = b < B;  // uniform over the team; the barriers below are reached by every thread
    const float *row = post + (size_t)(live ? b : 0) * K;
    float *stage = staged_rows + (STAGE ? (size_t)team * K : 0);
    double s = 0.0, d = 0.0;
    float sv = -__builtin_inff(), pv = -__builtin_inff();
    int si = NO_COLUMN, pi = NO_COLUMN;
    if (live) {
#pragma unroll 4
        for (int k = t; k < K; k += TEAM) {
            const float x = row[k];
            if (STAGE) stage[k] = x;
            if (k < G) {
                s += (double)x;
                if (better(x, k, sv, si)) {
                    sv = x;
                    si = k;
                }
            } else {
                d += (double)x;
                if (better(x, k, pv, pi)) {
                    pv = x;
                    pi = k;
                }
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        s += __shfl_xor(s, off);
        d += __shfl_xor(d, off);
        const float osv = __shfl_xor(sv, off), opv = __shfl_xor(pv, off);
        const int osi = __shfl_xor(si, off), opi = __shfl_xor(pi, off);
        if (better(osv, osi, sv, si)) {
            sv = osv;
            si = osi;
        }
        if (better(opv, opi, pv, pi)) {
            pv = opv;
            pi = opi;
        }
    }
    if (TEAM == 256 && lane == 0) {
        w_s[wave] = s;
        w_d[wave] = d;
        w_sv[wave] = sv;
        w_si[wave] = si;
        w_pv[wave] = pv;
        w_pi[wave] = pi;
    }
    if (TEAM == 256 || STAGE) __syncthreads();
    if (live && t == 0) {
        if (TEAM == 256) {
            for (int w = 1; w < 4; w++) {
                s += w_s[w];
                d += w_d[w];
                if (better(w_sv[w], w_si[w], sv, si)) {
                    sv = w_sv[w];
                    si = w_si[w];
                }
                if (better(w_pv[w], w_pi[w], pv, pi)) {
                    pv = w_pv[w];
                    pi = w_pi[w];
                }
            }
        }
        o.singlet_mass[b] = s;
        o.doublet_mass[b] = d;
        o.best_singlet[b] = si != NO_COLUMN ? si : -1;
        o.best_singlet_prob[b] = si != NO_COLUMN ? sv : __builtin_nanf("");
        o.best_pair[b] = pi != NO_COLUMN ? pi : -1;
        o.best_pair_prob[b] = pi != NO_COLUMN ? pv : __builtin_nanf("");
    }
    if (MARG && live) {
        const float *src = STAGE ? stage : row;
        const bool pairs = K > G;
        for (int g = t; g < G; g += TEAM) {
            double m = (double)src[g];
            if (pairs) {
                long long col = (long long)G + g - 1;  // (0, g); (g1 + 1, g) lies G - g1 - 2 columns after (g1, g)
                for (int g1 = 0; g1 < g; g1++) {
                    m += (double)src[col];
                    col += G - g1 - 2;
                }
                col = (long long)G + (long long)g * (2 * G - g - 1) / 2;  // (g, g + 1)
                for (int g2 = g + 1; g2 < G; g2++) m += (double)src[col++];
            }
            o.marginals[(size_t)b * G + g] = (float)m;
        }
    }
}

// Allowed mass: the listed posteriors of each barcode, widened to float64 and added in list order, and whether the row's first
// maximum (best[], from k_top_options<1>) is in the list.  One thread per barcode: the order is sequential by contract.
__global__ __launch_bounds__(256) void k_allowed_mass(const float *__restrict__ post, long long B, int K,
                                                      const long long *__restrict__ start, const int *__restrict__ options,
                                                      const int *__restrict__ best, double *__restrict__ mass,
                                                      int *__restrict__ best_is_allowed)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float *row = post + (size_t)b * K;
    const int top = best[b];
    double m = 0.0;
    int hit = 0;
    for (long long j = start[b]; j < start[b + 1]; j++) {
        const int k = options[j];
        m += (double)row[k];
        hit |= k == top;
    }
    mass[b] = m;
    best_is_allowed[b] = hit;
}

int check_ready(dmx_ctx *c, const char *who)
{
    if (!c) return fail(DMX_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->have_post) return fail(DMX_ERR_INVALID, "call order: dmx_estep / dmx_em before %s", who);
    return 0;
}

}  // namespace

extern "C" {

int dmx_get_assignments_above(dmx_ctx *c, float threshold, int32_t *best, float *best_p, int64_t *n_assigned)
{
    DMX_TRY(check_ready(c, "dmx_get_assignments_above"));
    Scratch sc(c);
    unsigned long long *d_n;
    DMX_TRY(sc.get(&d_n, 1));
    HIP_TRY(hipMemsetAsync(d_n, 0, sizeof(unsigned long long), c->stream));
    if (c->B > 0) {
        hipLaunchKernelGGL(k_top_options<1>, dim3((unsigned)((c->B + 3) / 4)), dim3(256), 0, c->stream, c->d_post.p, c->B, c->K,
                           threshold, c->d_best.p, c->d_bestp.p, d_n);
        DMX_TRY(launched("k_top_options"));
    }
    unsigned long long n = 0;
    if (best && c->B) HIP_TRY(hipMemcpyAsync(best, c->d_best.p, sizeof(int) * c->B, hipMemcpyDeviceToHost, c->stream));
    if (best_p && c->B) HIP_TRY(hipMemcpyAsync(best_p, c->d_bestp.p, sizeof(float) * c->B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_assigned) *n_assigned = (int64_t)n;
    return 0;
}

int dmx_get_top_options(dmx_ctx *c, int32_t k, int32_t *options, float *probs)
{
    DMX_TRY(check_ready(c, "dmx_get_top_options"));
    if (k < 1 || k > TOP_MAX) return fail(DMX_ERR_INVALID, "k must be 1..%d", TOP_MAX);
    if (c->B == 0) return 0;
    if (!options || !probs) return fail(DMX_ERR_INVALID, "null outputs");
    const size_t n = (size_t)c->B * k;
    Scratch sc(c);
    int *d_i;
    float *d_p;
    DMX_TRY(sc.get(&d_i, n));
    DMX_TRY(sc.get(&d_p, n));
    const dim3 grid((unsigned)((c->B + 3) / 4)), block(256);
    const float none = -__builtin_inff();
    switch (k) {
    case 1: hipLaunchKernelGGL(k_top_options<1>, grid, block, 0, c->stream, c->d_post.p, c->B, c->K, none, d_i, d_p, nullptr); break;
    case 2: hipLaunchKernelGGL(k_top_options<2>, grid, block, 0, c->stream, c->d_post.p, c->B, c->K, none, d_i, d_p, nullptr); break;
    case 3: hipLaunchKernelGGL(k_top_options<3>, grid, block, 0, c->stream, c->d_post.p, c->B, c->K, none, d_i, d_p, nullptr); break;
    default: hipLaunchKernelGGL(k_top_options<4>, grid, block, 0, c->stream, c->d_post.p, c->B, c->K, none, d_i, d_p, nullptr); break;
    }
    DMX_TRY(launched("k_top_options"));
    HIP_TRY(hipMemcpyAsync(options, d_i, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(probs, d_p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_get_option_sums(dmx_ctx *c, double *sums)
{
    DMX_TRY(check_ready(c, "dmx_get_option_sums"));
    if (!sums) return fail(DMX_ERR_INVALID, "null output");
    const int K = c->K;
    Scratch sc(c);
    double *d_part, *d_sums;
    DMX_TRY(sc.get(&d_part, (size_t)SUM_SLABS * K));
    DMX_TRY(sc.get(&d_sums, (size_t)K));
    const unsigned kb = (unsigned)((K + 255) / 256);
    hipLaunchKernelGGL(k_option_partial, dim3(kb, SUM_SLABS), dim3(256), 0, c->stream, c->d_post.p, c->B, K, d_part);
    hipLaunchKernelGGL(k_option_final, dim3(kb), dim3(256), 0, c->stream, d_part, K, d_sums);
    DMX_TRY(launched("k_option_partial / k_option_final"));
    HIP_TRY(hipMemcpyAsync(sums, d_sums, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_get_donor_readout(dmx_ctx *c, double *singlet_mass, double *doublet_mass, int32_t *best_singlet, float *best_singlet_prob,
                          int32_t *best_pair, float *best_pair_prob, float *donor_marginals)
{
    DMX_TRY(check_ready(c, "dmx_get_donor_readout"));
    if (c->B == 0) return 0;
    const long long B = c->B;
    const int K = c->K, G = c->G;
    if (G < 1 || (K != G && (long long)K != (long long)G * (G + 1) / 2))
        return fail(DMX_ERR_INVALID, "dmx_get_donor_readout: %d options are neither the singlets nor the singlets and pairs of %d donors", K, G);
    Scratch sc(c);
    DonorOut o = {};
    DMX_TRY(sc.get(&o.singlet_mass, (size_t)B));
    DMX_TRY(sc.get(&o.doublet_mass, (size_t)B));
    DMX_TRY(sc.get(&o.best_singlet, (size_t)B));
    DMX_TRY(sc.get(&o.best_pair, (size_t)B));
    DMX_TRY(sc.get(&o.best_singlet_prob, (size_t)B));
    DMX_TRY(sc.get(&o.best_pair_prob, (size_t)B));
    if (donor_marginals) DMX_TRY(sc.get(&o.marginals, (size_t)B * G));
    const float *post = c->d_post.p;
    const dim3 per_wave((unsigned)((B + 3) / 4)), per_group((unsigned)B), block(256);
    // the team depends on G alone, so that the masses - whose order of additions follows the team - keep their bits whether the
    // marginals are asked for or not
    if (!donor_marginals && G <= 64)  // nothing is read twice: no LDS
        hipLaunchKernelGGL((k_donor_readout<64, false, false>), per_wave, block, 0, c->stream, post, B, K, G, o);
    else if (!donor_marginals)
        hipLaunchKernelGGL((k_donor_readout<256, false, false>), per_group, block, 0, c->stream, post, B, K, G, o);
    else if (G <= 64)  // K <= 2080: four rows of 8 KB in LDS, lane g is donor g
        hipLaunchKernelGGL((k_donor_readout<64, true, true>), per_wave, block, 4 * (size_t)K * sizeof(float), c->stream, post, B, K, G, o);
    else if (K <= DONOR_LDS_ROW)
        hipLaunchKernelGGL((k_donor_readout<256, true, true>), per_group, block, (size_t)K * sizeof(float), c->stream, post, B, K, G, o);
    else
        hipLaunchKernelGGL((k_donor_readout<256, true, false>), per_group, block, 0, c->stream, post, B, K, G, o);
    DMX_TRY(launched("k_donor_readout"));
    const hipStream_t st = c->stream;
    if (singlet_mass) HIP_TRY(hipMemcpyAsync(singlet_mass, o.singlet_mass, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (doublet_mass) HIP_TRY(hipMemcpyAsync(doublet_mass, o.doublet_mass, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (best_singlet) HIP_TRY(hipMemcpyAsync(best_singlet, o.best_singlet, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    if (best_singlet_prob) HIP_TRY(hipMemcpyAsync(best_singlet_prob, o.best_singlet_prob, sizeof(float) * B, hipMemcpyDeviceToHost, st));
    if (best_pair) HIP_TRY(hipMemcpyAsync(best_pair, o.best_pair, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    if (best_pair_prob) HIP_TRY(hipMemcpyAsync(best_pair_prob, o.best_pair_prob, sizeof(float) * B, hipMemcpyDeviceToHost, st));
    if (donor_marginals) HIP_TRY(hipMemcpyAsync(donor_marginals, o.marginals, sizeof(float) * (size_t)B * G, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int dmx_get_allowed_mass(dmx_ctx *c, const int64_t *allowed_start, const int32_t *allowed_options, double *mass, int32_t *best_is_allowed)
{
    DMX_TRY(check_ready(c, "dmx_get_allowed_mass"));
    if (c->B == 0) return 0;
    const long long B = c->B;
    const int K = c->K;
    if (!allowed_start) return fail(DMX_ERR_INVALID, "dmx_get_allowed_mass: null allowed_start");
    if (allowed_start[0] != 0) return fail(DMX_ERR_INVALID, "dmx_get_allowed_mass: allowed_start[0] is %lld, not 0", (long long)allowed_start[0]);
    for (long long b = 0; b < B; b++)
        if (allowed_start[b + 1] < allowed_start[b])
            return fail(DMX_ERR_INVALID, "dmx_get_allowed_mass: allowed_start decreases at barcode %lld", b);
    const long long n = allowed_start[B];
    if (n > 0 && !allowed_options) return fail(DMX_ERR_INVALID, "dmx_get_allowed_mass: null allowed_options");
    for (long long j = 0; j < n; j++)
        if (allowed_options[j] < 0 || allowed_options[j] >= K)
            return fail(DMX_ERR_INVALID, "dmx_get_allowed_mass: allowed_options[%lld] = %d is outside [0, %d)", j, (int)allowed_options[j], K);
    Scratch sc(c);
    long long *d_start;
    int *d_options, *d_top, *d_hit;
    float *d_top_p;
    double *d_mass;
    static_assert(sizeof(long long) == sizeof(int64_t), "");
    DMX_TRY(upload(sc, &d_start, (const long long *)allowed_start, (size_t)B + 1, c->stream));
    DMX_TRY(upload(sc, &d_options, (const int *)allowed_options, (size_t)n, c->stream));
    DMX_TRY(sc.get(&d_top, (size_t)B));
    DMX_TRY(sc.get(&d_top_p, (size_t)B));
    DMX_TRY(sc.get(&d_hit, (size_t)B));
    DMX_TRY(sc.get(&d_mass, (size_t)B));
    hipLaunchKernelGGL(k_top_options<1>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, c->d_post.p, B, K, -__builtin_inff(), d_top,
                       d_top_p, nullptr);
    hipLaunchKernelGGL(k_allowed_mass, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, c->d_post.p, B, K, d_start, d_options,
                       d_top, d_mass, d_hit);
    DMX_TRY(launched("k_top_options / k_allowed_mass"));
    if (mass) HIP_TRY(hipMemcpyAsync(mass, d_mass, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    if (best_is_allowed) HIP_TRY(hipMemcpyAsync(best_is_allowed, d_hit, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
