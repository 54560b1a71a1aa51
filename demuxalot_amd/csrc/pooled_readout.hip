// pooled_readout.hip -- the resident compact result of a pooled pass (the "pooled slot" of dmx_ctx) and the read-outs over it
// (include/demux_hip_debug.h "Pooled results kept resident").  What results.hip is to the dense [B, K] posteriors this
// file is to the compact rows of dmx_estep_pools, dmx_estep_ambient and the two grid passes: the rows stay on the device, and what
// users take from them - the best options, the masses, the donor marginals, the option sums of every pool, the allowed mass - is
// reduced there.  Option indices are pool-local: for a pool of g donors option i < g is singlet i, pair (i < j) is at
// g + i (2g - i - 1) / 2 + (j - i - 1).  The order of additions is the contract (no atomics touch a result), so every output is
// checkable bit for bit; what the entries refuse is pooled_readout_plan.h's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>

#include "device_scratch.h"
#include "estep_pools.h"
#include "pooled_readout_plan.h"

namespace dmx {

namespace {

using namespace dmx::scratch;

constexpr int ROW_MAX = (int)pplan::MAX_OPTIONS;  // floats of the longest compact row
constexpr int NO_COLUMN = 0x7FFFFFFF;
constexpr int SUM_SLABS = prplan::SUM_SLABS;

// first maximum, NaN never wins (results.hip: better)
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

struct ReadoutArgs {
    const float *post;
    const long long *row_ptr;
    const int *pool_of, *pool_size;
    long long B;
    const long long *marg_ptr;
    double *singlet_mass, *doublet_mass;  // every output: nullable
    int *best_option, *best_singlet, *best_pair;
    float *best_prob, *best_singlet_prob, *best_pair_prob;
    float *marginals;
};

// One wavefront per barcode, four barcodes per workgroup (k_donor_readout<64> of results.hip on compact rows):
//   1. the row comes in with coalesced loads; on the way every lane keeps the first maximum (better()) of its singlet and of its pair
//      options, and with MASS or MARG the row is left in LDS (4 KB per wavefront);
//   2. the lanes' maxima are combined by xor shuffles; the row's first maximum is the better of the two kinds;
//   3. MASS: lane 0 adds the singlets and lane 1 the pairs, widened to float64, sequentially in ASCENDING OPTION ORDER - the pooled
//      pass's own definition of doublet_mass (estep_pools_row.h: pool_row_close), so the two are equal bit for bit;
//   4. MARG: lane i adds the options that contain donor i in ascending option order - singlet i, (0, i) .. (i-1, i), (i, i+1) ..
//      (i, g-1) - and rounds once (results.hip's rule on the pool's own columns).
// A barcode in no pool has no row: -1 / NaN everywhere, written here.
template <bool MASS, bool MARG>
__global__ __launch_bounds__(256) void k_pooled_readout(ReadoutArgs a)
{
    constexpr bool STAGE = MASS || MARG;
    __shared__ float staged_rows[STAGE ? 4 * ROW_MAX : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = (long long)blockIdx.x * 4 + wave;
    const bool live = b < a.B;  // uniform over the wavefront; the barrier below is reached by every thread
    const int p = live ? a.pool_of[b] : -1;
    const long long first = p >= 0 ? a.row_ptr[b] : 0;
    const int K = p >= 0 ? (int)(a.row_ptr[b + 1] - first) : 0;  // 1 .. ROW_MAX (pools_plan.h: check)
    const int g = p >= 0 ? a.pool_size[p] : 0;
    const float *__restrict__ row = a.post + first;
    float *stage = staged_rows + (STAGE ? wave * ROW_MAX : 0);
    float sv = -__builtin_inff(), pv = -__builtin_inff();
    int si = NO_COLUMN, pi = NO_COLUMN;
#pragma unroll 4
    for (int k = lane; k < K; k += 64) {
        const float x = row[k];
        if (STAGE) stage[k] = x;
        if (k < g) {
            if (better(x, k, sv, si)) {
                sv = x;
                si = k;
            }
        } else if (better(x, k, pv, pi)) {
            pv = x;
            pi = k;
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
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
    if (STAGE) __syncthreads();
    double mass = 0.0;
    if (MASS && lane < 2) {
        const int lo = lane == 0 ? 0 : g, hi = lane == 0 ? g : K;
        int k = lo;
        for (; k + 8 <= hi; k += 8) {  // eight LDS reads in flight, then their additions in order: the chain is the additions alone
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = stage[k + j];
#pragma unroll
            for (int j = 0; j < 8; j++) mass += (double)x[j];
        }
        for (; k < hi; k++) mass += (double)stage[k];
    }
    const double s = __shfl(mass, 0), d = __shfl(mass, 1);
    if (live && lane == 0) {
        const float none = __builtin_nanf("");
        const bool have_s = si != NO_COLUMN, have_p = pi != NO_COLUMN;
        const bool pair_wins = have_p && (!have_s || pv > sv);  // (a pair's index is above every singlet's: it wins on value alone)
        if (MASS && a.singlet_mass) a.singlet_mass[b] = p >= 0 ? s : (double)none;
        if (MASS && a.doublet_mass) a.doublet_mass[b] = p >= 0 ? d : (double)none;
        if (a.best_option) a.best_option[b] = pair_wins ? pi : have_s ? si : -1;
        if (a.best_prob) a.best_prob[b] = pair_wins ? pv : have_s ? sv : none;
        if (a.best_singlet) a.best_singlet[b] = have_s ? si : -1;
        if (a.best_singlet_prob) a.best_singlet_prob[b] = have_s ? sv : none;
        if (a.best_pair) a.best_pair[b] = have_p ? pi : -1;
        if (a.best_pair_prob) a.best_pair_prob[b] = have_p ? pv : none;
    }
    if (MARG && p >= 0) {
        const bool pairs = K > g;
        float *__restrict__ out = a.marginals + a.marg_ptr[b];
        for (int i = lane; i < g; i += 64) {
            double m = (double)stage[i];
            if (pairs) {
                int col = g + i - 1;  // (0, i); (j + 1, i) lies g - j - 2 options after (j, i)
                for (int j = 0; j < i; j++) {
                    m += (double)stage[col];
                    col += g - j - 2;
                }
                col = g + i * (2 * g - i - 1) / 2;  // (i, i + 1)
                for (int j = i + 1; j < g; j++) m += (double)stage[col++];
            }
            out[i] = (float)m;
        }
    }
}

// k_top_options of results.hip on compact rows: a barcode in no pool has a row of no entries, so -1 / NaN throughout
template <int TOP>
__global__ __launch_bounds__(256) void k_pooled_top_options(const float *__restrict__ post, const long long *__restrict__ row_ptr, long long B,
                                                            int *__restrict__ best, float *__restrict__ best_p)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long first = row_ptr[b];
    const int K = (int)(row_ptr[b + 1] - first);
    const float *row = post + first;
    float v[TOP];
    int ix[TOP];
#pragma unroll
    for (int t = 0; t < TOP; t++) {
        v[t] = -__builtin_inff();
        ix[t] = NO_COLUMN;
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
        if (bi == ix[0] && bi != NO_COLUMN) {  // the winning lane pops its head
#pragma unroll
            for (int t = 0; t + 1 < TOP; t++) {
                v[t] = v[t + 1];
                ix[t] = ix[t + 1];
            }
            v[TOP - 1] = -__builtin_inff();
            ix[TOP - 1] = NO_COLUMN;
        }
        if (lane == 0) {
            const bool have = bi != NO_COLUMN;
            best[(size_t)b * TOP + r] = have ? bi : -1;
            best_p[(size_t)b * TOP + r] = have ? bv : __builtin_nanf("");
        }
    }
}

// Option sums of every pool in two deterministic passes (k_option_partial / k_option_final of results.hip on the pool's list of
// barcodes): slab j of pool p is list positions [j per, min((j + 1) per, n_p)), per = ceil(n_p / 512), added sequentially; then the
// 512 slab sums in slab order.  grid: (256 options, slab, pool); an empty pool has empty slabs: zeros.
__global__ __launch_bounds__(256) void k_pooled_option_partial(const float *__restrict__ post, const long long *__restrict__ row_ptr,
                                                               const long long *__restrict__ opt_ptr, const long long *__restrict__ list_ptr,
                                                               const int *__restrict__ list, long long n_options, double *__restrict__ partial)
{
    const int k = blockIdx.x * 256 + threadIdx.x, p = blockIdx.z;
    const long long o0 = opt_ptr[p];
    if (k >= opt_ptr[p + 1] - o0) return;
    const long long l0 = list_ptr[p], n = list_ptr[p + 1] - l0;
    const long long per = (n + SUM_SLABS - 1) / SUM_SLABS;
    const long long i0 = (long long)blockIdx.y * per;
    const long long i1 = i0 + per < n ? i0 + per : n;
    double s = 0.0;
    for (long long i = i0; i < i1; i++) s += (double)post[row_ptr[list[l0 + i]] + k];
    partial[(size_t)blockIdx.y * n_options + o0 + k] = s;
}

__global__ __launch_bounds__(256) void k_pooled_option_final(const double *__restrict__ partial, long long n_options, double *__restrict__ sums)
{
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_options) return;
    double s = 0.0;
    for (int j = 0; j < SUM_SLABS; j++) s += partial[(size_t)j * n_options + o];
    sums[o] = s;
}

// k_allowed_mass of results.hip with pool-local options: one thread per barcode, the order is sequential by contract
__global__ __launch_bounds__(256) void k_pooled_allowed_mass(const float *__restrict__ post, const long long *__restrict__ row_ptr,
                                                             const int *__restrict__ pool_of, long long B, const long long *__restrict__ start,
                                                             const int *__restrict__ options, const int *__restrict__ best,
                                                             double *__restrict__ mass, int *__restrict__ best_is_allowed)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    if (pool_of[b] < 0) {  // (its list is empty: pooled_readout_plan.h)
        mass[b] = (double)__builtin_nanf("");
        best_is_allowed[b] = 0;
        return;
    }
    const float *row = post + row_ptr[b];
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

// the rows of one pool's barcodes as a dense [n, K] block of 4-byte words (float32 or int32 alike)
__global__ __launch_bounds__(256) void k_pooled_gather_pool(const unsigned *__restrict__ values, const long long *__restrict__ row_ptr,
                                                            const int *__restrict__ list, long long n, int K, unsigned *__restrict__ out)
{
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= n * K) return;
    const long long r = at / K;
    out[at] = values[row_ptr[list[r]] + (at - r * K)];
}

// (pools_plan.h's one text that is read behind its value: "1035 options in a pool, ..."; every other value follows its text)
int refuse(const char *who, const prplan::Verdict &v)
{
    if (v.value >= 0 && std::strncmp(v.what, "options in a pool", 17) == 0) return fail(v.status, "%s: %lld %s (at %lld)", who, v.value, v.what, v.at);
    if (v.value >= 0 && v.at >= 0) return fail(v.status, "%s: %s (at %lld: %lld)", who, v.what, v.at, v.value);
    if (v.value >= 0) return fail(v.status, "%s: %s (%lld)", who, v.what, v.value);
    if (v.at >= 0) return fail(v.status, "%s: %s (at %lld)", who, v.what, v.at);
    return fail(v.status, "%s: %s", who, v.what);
}

int check_slot(dmx_ctx *c, const char *who)
{
    if (!c) return fail(DMX_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->pooled.present)
        return fail(DMX_ERR_INVALID, "call order: a pooled pass with dmx_set_keep_pooled(ctx, 1), or dmx_pooled_upload, before %s", who);
    return 0;
}

// a block of the slot's own: allocated from the context's cache, filled from the host
template <typename T>
int slot_block(dmx_ctx *c, PooledSlot &s, T **out, const T *host, size_t count)
{
    void *p = nullptr;
    DMX_TRY(ctx_malloc(c, &p, (count ? count : 1) * sizeof(T)));
    *out = (T *)p;  // (the slot's from here: free_pooled_slot gives it back)
    s.bytes += (int64_t)((count ? count : 1) * sizeof(T));
    if (count) HIP_TRY(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// every pool's barcodes, ascending, from the slot's host copy of pool_of (4 bytes per barcode), and where every barcode's donor
// marginals begin (8 bytes per barcode: the read-out uploads nothing per call)
int slot_lists(dmx_ctx *c, PooledSlot &s)
{
    std::vector<int32_t> list;
    prplan::pool_lists(s.B, s.n_pools, s.h_pool_of.data(), s.h_pool_list_ptr, list);
    prplan::marg_ptr(s.B, s.h_pool_of.data(), s.h_pool_size.data(), s.h_marg_ptr);
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "");
    DMX_TRY(slot_block(c, s, &s.marg_ptr, (const long long *)s.h_marg_ptr.data(), s.h_marg_ptr.size()));
    DMX_TRY(slot_block(c, s, &s.pool_list_ptr, (const long long *)s.h_pool_list_ptr.data(), s.h_pool_list_ptr.size()));
    DMX_TRY(slot_block(c, s, &s.pool_list, (const int *)list.data(), list.size()));
    HIP_TRY(hipStreamSynchronize(c->stream));  // `list` is a local
    return 0;
}

void install_slot(dmx_ctx *c, PooledSlot &s)
{
    host::free_pooled_slot(c, c->pooled);
    s.present = true;
    c->pooled = std::move(s);
}

void present_matrices(const PooledSlot &s, bool (&present)[prplan::N_WHAT])
{
    present[prplan::LOGITS] = s.logits != nullptr;
    present[prplan::PROBS] = s.post != nullptr;
    present[prplan::ALPHA_INDEX] = s.alpha_index != nullptr;
    present[prplan::ALPHA_MEAN] = s.alpha_mean != nullptr;
}

const void *matrix_of(const PooledSlot &s, int what)
{
    return what == prplan::LOGITS ? (const void *)s.logits : what == prplan::PROBS ? (const void *)s.post : what == prplan::ALPHA_INDEX ? (const void *)s.alpha_index : (const void *)s.alpha_mean;
}

template <typename T>
int download(dmx_ctx *c, T *host, const T *device, size_t count)
{
    if (host && count) HIP_TRY(hipMemcpyAsync(host, device, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

}  // namespace

// The hand-over of a pass's compact result to the context's slot (estep_pools.h): the layout arrays and the rows leave the run's
// temporaries (`rows`; the grid passes' alpha_index / alpha_mean leave `grid`) and become the slot's - no copy, no second allocation
// of size row_ptr[B].  Everything that can fail - the host copies, the pool lists and their upload - comes first: a failure leaves the
// previous slot in place and the run's temporaries to the run.
int keep_pooled_result(dmx_ctx *c, const PoolsPlan &plan, const PoolEstepArgs &a, scratch::Scratch &rows, scratch::Scratch *grid,
                       const int *alpha_index, const float *alpha_mean)
{
    const long long B = c->B, P = plan.n_pools;
    PooledSlot s;
    s.with_doublets = plan.with_doublets;
    s.B = B;
    s.n_pools = P;
    s.n_values = B > 0 ? (long long)plan.row_ptr[B] : 0;
    s.h_opt_ptr.assign(plan.opt_ptr.begin(), plan.opt_ptr.end());
    s.h_pool_size = plan.pool_size;
    s.h_pool_of.assign(plan.pool_of_barcode, plan.pool_of_barcode + B);
    s.h_row_ptr.assign(plan.row_ptr, plan.row_ptr + B + 1);
    if (const int rc = slot_lists(c, s)) {
        host::free_pooled_slot(c, s);
        return rc;
    }
    bool all = true;
    auto take = [&](scratch::Scratch &from, auto *&mine, const auto *block, size_t count, size_t size) {
        if (!from.hand_over(block)) return void(all = false);
        mine = const_cast<std::remove_reference_t<decltype(mine)>>(block);
        s.bytes += (int64_t)((count ? count : 1) * size);
    };
    take(rows, s.opt_ptr, a.opt_ptr, (size_t)P + 1, sizeof(long long));
    take(rows, s.opts, a.opts, plan.opts.size(), sizeof(unsigned));
    take(rows, s.pool_size, a.pool_size, (size_t)P, sizeof(int));
    take(rows, s.pool_of, a.pool_of, (size_t)B, sizeof(int));
    take(rows, s.row_ptr, a.row_ptr, (size_t)B + 1, sizeof(long long));
    take(rows, s.logits, (const float *)a.logits, (size_t)s.n_values, sizeof(float));
    take(rows, s.post, (const float *)a.post, (size_t)s.n_values, sizeof(float));
    if (grid && alpha_index) take(*grid, s.alpha_index, alpha_index, (size_t)s.n_values, sizeof(int));
    if (grid && alpha_mean) take(*grid, s.alpha_mean, alpha_mean, (size_t)s.n_values, sizeof(float));
    if (!all) {  // (a block that is not the run's: what was taken goes back to the cache, the rest is still the run's)
        host::free_pooled_slot(c, s);
        return fail(DMX_ERR_HIP, "dmx_set_keep_pooled: a result buffer is not one of the pass's temporaries");
    }
    install_slot(c, s);
    return 0;
}

}  // namespace dmx

using namespace dmx;

extern "C" {

int dmx_set_keep_pooled(dmx_ctx *c, int keep)
{
    if (!c) return fail(DMX_ERR_INVALID, "null ctx");
    if (keep != 0 && keep != 1) return fail(DMX_ERR_INVALID, "dmx_set_keep_pooled: keep must be 0 or 1");
    c->keep_pooled = keep;
    return 0;
}

int dmx_pooled_upload(dmx_ctx *c, int64_t B, int32_t G, int with_doublets, int32_t n_pools, const int64_t *pool_start, const int32_t *pool_donors,
                      const int32_t *pool_of_barcode, const int64_t *row_ptr, const float *logits, const float *probs)
{
    if (!c) return fail(DMX_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    const prplan::Verdict verdict = prplan::check_upload(G, B, with_doublets, n_pools, pool_start, pool_donors, pool_of_barcode, row_ptr, probs);
    if (verdict.status != prplan::OK) return refuse("dmx_pooled_upload", verdict);
    static const float no_penalty = 0.0f;
    const pplan::Pools pools{with_doublets, n_pools, pool_start, pool_donors, &no_penalty, pool_of_barcode, row_ptr};
    std::vector<long long> opt_ptr;
    std::vector<unsigned> opts;
    PooledSlot s;
    pplan::layout(pools, opt_ptr, opts, s.h_pool_size);
    s.with_doublets = with_doublets != 0;
    s.B = B;
    s.n_pools = n_pools;
    s.n_values = row_ptr[B];
    s.h_opt_ptr.assign(opt_ptr.begin(), opt_ptr.end());
    s.h_pool_of.assign(pool_of_barcode, pool_of_barcode + B);
    s.h_row_ptr.assign(row_ptr, row_ptr + B + 1);
    const size_t n = (size_t)s.n_values;
    int rc = slot_block(c, s, &s.opt_ptr, opt_ptr.data(), opt_ptr.size());
    if (!rc) rc = slot_block(c, s, &s.opts, opts.data(), opts.size());
    if (!rc) rc = slot_block(c, s, &s.pool_size, s.h_pool_size.data(), s.h_pool_size.size());
    if (!rc) rc = slot_block(c, s, &s.pool_of, (const int *)pool_of_barcode, (size_t)B);
    if (!rc) rc = slot_block(c, s, &s.row_ptr, (const long long *)row_ptr, (size_t)B + 1);
    if (!rc) rc = slot_block(c, s, &s.post, probs, n);
    if (!rc && logits) rc = slot_block(c, s, &s.logits, logits, n);
    if (!rc) rc = slot_lists(c, s);  // (synchronises: the uploads read the caller's arrays and this function's locals)
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        host::free_pooled_slot(c, s);
        return rc;
    }
    install_slot(c, s);
    return 0;
}

int dmx_pooled_info(dmx_ctx *c, int64_t info[8])
{
    if (!c) return fail(DMX_ERR_INVALID, "null ctx");
    if (!info) return fail(DMX_ERR_INVALID, "dmx_pooled_info: null info");
    const PooledSlot &s = c->pooled;
    info[0] = s.present;
    info[1] = s.B;
    info[2] = s.n_pools;
    info[3] = s.n_values;
    info[4] = s.with_doublets;
    info[5] = s.logits != nullptr;
    info[6] = s.alpha_index != nullptr;
    info[7] = s.alpha_mean != nullptr;
    return 0;
}

int dmx_pooled_release(dmx_ctx *c)
{
    if (!c) return fail(DMX_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    host::release_pooled_slot(c);
    return 0;
}

int dmx_pooled_get(dmx_ctx *c, int what, int64_t b0, int64_t b1, void *out)
{
    DMX_TRY(check_slot(c, "dmx_pooled_get"));
    const PooledSlot &s = c->pooled;
    bool present[prplan::N_WHAT];
    present_matrices(s, present);
    const prplan::Verdict verdict = prplan::check_get(s.B, what, present, b0, b1);
    if (verdict.status != prplan::OK) return refuse("dmx_pooled_get", verdict);
    const long long first = s.h_row_ptr[(size_t)b0], n = s.h_row_ptr[(size_t)b1] - first;
    if (n == 0) return 0;
    if (!out) return fail(DMX_ERR_INVALID, "dmx_pooled_get: null output");
    HIP_TRY(hipMemcpyAsync(out, (const unsigned *)matrix_of(s, what) + first, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_pooled_get_pool(dmx_ctx *c, int what, int32_t pool, void *out)
{
    DMX_TRY(check_slot(c, "dmx_pooled_get_pool"));
    const PooledSlot &s = c->pooled;
    bool present[prplan::N_WHAT];
    present_matrices(s, present);
    const prplan::Verdict verdict = prplan::check_get_pool(s.n_pools, what, present, pool);
    if (verdict.status != prplan::OK) return refuse("dmx_pooled_get_pool", verdict);
    const long long l0 = s.h_pool_list_ptr[(size_t)pool], n = s.h_pool_list_ptr[(size_t)pool + 1] - l0;
    const int K = (int)(s.h_opt_ptr[(size_t)pool + 1] - s.h_opt_ptr[(size_t)pool]);
    if (n == 0) return 0;
    if (!out) return fail(DMX_ERR_INVALID, "dmx_pooled_get_pool: null output");
    Scratch sc(c);
    unsigned *d_block;
    DMX_TRY(sc.get(&d_block, (size_t)n * K));
    hipLaunchKernelGGL(k_pooled_gather_pool, dim3(grid_for(n * K)), dim3(256), 0, c->stream, (const unsigned *)matrix_of(s, what), s.row_ptr,
                       s.pool_list + l0, n, K, d_block);
    DMX_TRY(launched("k_pooled_gather_pool"));
    HIP_TRY(hipMemcpyAsync(out, d_block, sizeof(unsigned) * (size_t)n * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_pooled_readout(dmx_ctx *c, double *singlet_mass, double *doublet_mass, int32_t *best_option, float *best_prob, int32_t *best_singlet,
                       float *best_singlet_prob, int32_t *best_pair, float *best_pair_prob, int64_t *marg_ptr_out, float *donor_marginals)
{
    DMX_TRY(check_slot(c, "dmx_pooled_readout"));
    const PooledSlot &s = c->pooled;
    const long long B = s.B;
    const std::vector<int64_t> &marg_ptr = s.h_marg_ptr;
    if (marg_ptr_out) std::copy(marg_ptr.begin(), marg_ptr.end(), marg_ptr_out);
    const bool maxima = best_option || best_prob || best_singlet || best_singlet_prob || best_pair || best_pair_prob;
    if (B == 0 || !(singlet_mass || doublet_mass || maxima || donor_marginals)) return 0;  // (marg_ptr alone is the host's)
    const size_t n_marg = donor_marginals ? (size_t)marg_ptr[(size_t)B] : 0;
    Scratch sc(c);
    ReadoutArgs a = {};
    a.post = s.post;
    a.row_ptr = s.row_ptr;
    a.pool_of = s.pool_of;
    a.pool_size = s.pool_size;
    a.B = B;
    if (singlet_mass) DMX_TRY(sc.get(&a.singlet_mass, (size_t)B));
    if (doublet_mass) DMX_TRY(sc.get(&a.doublet_mass, (size_t)B));
    if (best_option) DMX_TRY(sc.get(&a.best_option, (size_t)B));
    if (best_prob) DMX_TRY(sc.get(&a.best_prob, (size_t)B));
    if (best_singlet) DMX_TRY(sc.get(&a.best_singlet, (size_t)B));
    if (best_singlet_prob) DMX_TRY(sc.get(&a.best_singlet_prob, (size_t)B));
    if (best_pair) DMX_TRY(sc.get(&a.best_pair, (size_t)B));
    if (best_pair_prob) DMX_TRY(sc.get(&a.best_pair_prob, (size_t)B));
    if (donor_marginals) {
        a.marg_ptr = s.marg_ptr;
        DMX_TRY(sc.get(&a.marginals, n_marg));
    }
    const bool mass = singlet_mass || doublet_mass, marg = donor_marginals != nullptr;
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    if (mass && marg)
        hipLaunchKernelGGL((k_pooled_readout<true, true>), grid, block, 0, c->stream, a);
    else if (mass)
        hipLaunchKernelGGL((k_pooled_readout<true, false>), grid, block, 0, c->stream, a);
    else if (marg)
        hipLaunchKernelGGL((k_pooled_readout<false, true>), grid, block, 0, c->stream, a);
    else
        hipLaunchKernelGGL((k_pooled_readout<false, false>), grid, block, 0, c->stream, a);
    DMX_TRY(launched("k_pooled_readout"));
    DMX_TRY(download(c, singlet_mass, a.singlet_mass, (size_t)B));
    DMX_TRY(download(c, doublet_mass, a.doublet_mass, (size_t)B));
    DMX_TRY(download(c, (int *)best_option, a.best_option, (size_t)B));
    DMX_TRY(download(c, best_prob, a.best_prob, (size_t)B));
    DMX_TRY(download(c, (int *)best_singlet, a.best_singlet, (size_t)B));
    DMX_TRY(download(c, best_singlet_prob, a.best_singlet_prob, (size_t)B));
    DMX_TRY(download(c, (int *)best_pair, a.best_pair, (size_t)B));
    DMX_TRY(download(c, best_pair_prob, a.best_pair_prob, (size_t)B));
    DMX_TRY(download(c, donor_marginals, a.marginals, n_marg));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_pooled_top_options(dmx_ctx *c, int32_t k, int32_t *options, float *probs)
{
    DMX_TRY(check_slot(c, "dmx_pooled_top_options"));
    const prplan::Verdict verdict = prplan::check_top(k);
    if (verdict.status != prplan::OK) return refuse("dmx_pooled_top_options", verdict);
    const PooledSlot &s = c->pooled;
    const long long B = s.B;
    if (B == 0) return 0;
    if (!options || !probs) return fail(DMX_ERR_INVALID, "dmx_pooled_top_options: null outputs");
    const size_t n = (size_t)B * k;
    Scratch sc(c);
    int *d_i;
    float *d_p;
    DMX_TRY(sc.get(&d_i, n));
    DMX_TRY(sc.get(&d_p, n));
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    switch (k) {
    case 1: hipLaunchKernelGGL(k_pooled_top_options<1>, grid, block, 0, c->stream, s.post, s.row_ptr, B, d_i, d_p); break;
    case 2: hipLaunchKernelGGL(k_pooled_top_options<2>, grid, block, 0, c->stream, s.post, s.row_ptr, B, d_i, d_p); break;
    case 3: hipLaunchKernelGGL(k_pooled_top_options<3>, grid, block, 0, c->stream, s.post, s.row_ptr, B, d_i, d_p); break;
    default: hipLaunchKernelGGL(k_pooled_top_options<4>, grid, block, 0, c->stream, s.post, s.row_ptr, B, d_i, d_p); break;
    }
    DMX_TRY(launched("k_pooled_top_options"));
    HIP_TRY(hipMemcpyAsync(options, d_i, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(probs, d_p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_pooled_option_sums(dmx_ctx *c, double *sums, int64_t *n_barcodes)
{
    DMX_TRY(check_slot(c, "dmx_pooled_option_sums"));
    const PooledSlot &s = c->pooled;
    const long long P = s.n_pools, n_options = P ? (long long)s.h_opt_ptr[(size_t)P] : 0;
    if (n_barcodes)
        for (long long p = 0; p < P; p++) n_barcodes[p] = s.h_pool_list_ptr[(size_t)p + 1] - s.h_pool_list_ptr[(size_t)p];
    if (!sums || n_options == 0) return 0;
    long long widest = 0;
    for (long long p = 0; p < P; p++) widest = std::max<long long>(widest, s.h_opt_ptr[(size_t)p + 1] - s.h_opt_ptr[(size_t)p]);
    if (P > 65535) return fail(DMX_ERR_UNSUPPORTED, "dmx_pooled_option_sums: %lld pools, more than the 65535 of one launch", P);
    Scratch sc(c);
    double *d_part, *d_sums;
    DMX_TRY(sc.get(&d_part, (size_t)SUM_SLABS * (size_t)n_options));
    DMX_TRY(sc.get(&d_sums, (size_t)n_options));
    hipLaunchKernelGGL(k_pooled_option_partial, dim3(grid_for(widest), SUM_SLABS, (unsigned)P), dim3(256), 0, c->stream, s.post, s.row_ptr, s.opt_ptr,
                       s.pool_list_ptr, s.pool_list, n_options, d_part);
    hipLaunchKernelGGL(k_pooled_option_final, dim3(grid_for(n_options)), dim3(256), 0, c->stream, d_part, n_options, d_sums);
    DMX_TRY(launched("k_pooled_option_partial / k_pooled_option_final"));
    HIP_TRY(hipMemcpyAsync(sums, d_sums, (size_t)n_options * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int dmx_pooled_allowed_mass(dmx_ctx *c, const int64_t *allowed_start, const int32_t *allowed_options, double *mass, int32_t *best_is_allowed)
{
    DMX_TRY(check_slot(c, "dmx_pooled_allowed_mass"));
    const PooledSlot &s = c->pooled;
    const long long B = s.B;
    if (B == 0) return 0;
    const prplan::Verdict verdict = prplan::check_allowed(B, s.h_pool_of.data(), s.h_row_ptr.data(), allowed_start, allowed_options);
    if (verdict.status != prplan::OK) return refuse("dmx_pooled_allowed_mass", verdict);
    const long long n = allowed_start[B];
    Scratch sc(c);
    long long *d_start;
    int *d_options, *d_top, *d_hit;
    float *d_top_p;
    double *d_mass;
    DMX_TRY(upload(sc, &d_start, (const long long *)allowed_start, (size_t)B + 1, c->stream));
    DMX_TRY(upload(sc, &d_options, (const int *)allowed_options, (size_t)n, c->stream));
    DMX_TRY(sc.get(&d_top, (size_t)B));
    DMX_TRY(sc.get(&d_top_p, (size_t)B));
    DMX_TRY(sc.get(&d_hit, (size_t)B));
    DMX_TRY(sc.get(&d_mass, (size_t)B));
    hipLaunchKernelGGL(k_pooled_top_options<1>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, c->stream, s.post, s.row_ptr, B, d_top, d_top_p);
    hipLaunchKernelGGL(k_pooled_allowed_mass, dim3(grid_for(B)), dim3(256), 0, c->stream, s.post, s.row_ptr, s.pool_of, B, d_start, d_options, d_top,
                       d_mass, d_hit);
    DMX_TRY(launched("k_pooled_top_options / k_pooled_allowed_mass"));
    if (mass) HIP_TRY(hipMemcpyAsync(mass, d_mass, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    if (best_is_allowed) HIP_TRY(hipMemcpyAsync(best_is_allowed, d_hit, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
