// mstep_doublet_shares.hip -- the M-step that learns from doublets of unequal shares (include/demux_hip_debug.h:
// dmx_mstep_doublet_shares, dmx_em_doublet_shares).  mstep_doublets.hip's contract with one change.  For a live pair
// k = (d1, d2) of barcode b, d1 ahead of d2 in the pool's option order, and w = share_mean[b, k], in float32, every operation rounded
// (-ffp-contract=off):
//   w_own = w for g == d1, 1.0f - w for g == d2;  w_other = the other of the two
//   a = prob[v, g] w_own;  o = prob[v, h] w_other;  r = a == 0 ? 0 : a / (a + o);   credit = credit + post[k] r      (IEEE division)
// Everything else - the live dense credit, the threshold, the row's option order, w = (credit keep) ^ power, the float64 accumulator
// per (v, g) in call order, the combining pass with the redo queue - is mstep_doublets.hip's, in the frame of mstep_weighted.h.
// This file holds
//   k_live_pair_shares        k_live_pairs' fill with the pair's share beside its posterior: (g | h << 16, posterior bits, share bits, 0),
//                             one 16-byte store per live pair behind the scanned counts (the counts are k_live_pairs<false>'s)
//   k_mstep_doublet_shares    k_mstep_doublets' walk; a lane that computes an entry's terms forms both products once and both
//                             donors' quotients over the one sum (float32 addition commutes)
//   k_mredo_doublet_shares    the frame's redo of the queued sums with this weight
// and the list's buffers of a call (DoubletSharesRun).  Per-call data are fetched a call per lane and broadcast by v_readlane (no
// uniform 4-byte request per call: DESIGN.md 4.6).  All stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "device_scratch.h"
#include "mstep_doublet_shares.h"
#include "mstep_weighted_device.h"

namespace dmx {

namespace {

typedef unsigned long long ull;

template <bool SQUARE>
__device__ __forceinline__ float credit_weight(float credit, float keep, float power)
{
    return power_weight<SQUARE>(credit * keep, power);
}

// both donors' responsibilities for a call in the mixture p1 w + p2 (1 - w) the pair's posterior mean share stands for: the two
// products, their one sum, a quotient each (+0 where the donor's own product is 0)
__device__ __forceinline__ void responsibilities(float p1, float p2, float share, float &r1, float &r2)
{
    const float a1 = p1 * share, a2 = p2 * (1.0f - share);
    const float sum = a1 + a2;
    r1 = a1 == 0.0f ? 0.0f : a1 / sum;
    r2 = a2 == 0.0f ? 0.0f : a2 / sum;
}

// One list entry for the columns of word w: both donors' terms post * r, when one of the donors lies in the word (else the entry stays
// out: g = h = -1 as the caller set them)
__device__ __forceinline__ void pair_terms(uint4 entry, const float *__restrict__ prob_row, int w, int &g, int &h, float &term_g, float &term_h)
{
    const int dg = (int)(entry.x & 0xFFFFu), dh = (int)(entry.x >> 16);
    if ((dg >> 6) != w && (dh >> 6) != w) return;
    const float posterior = __uint_as_float(entry.y);
    float rg, rh;
    responsibilities(prob_row[dg], prob_row[dh], __uint_as_float(entry.z), rg, rh);
    term_g = posterior * rg;
    term_h = posterior * rh;
    g = dg;
    h = dh;
}

// k_live_pairs<true> with the share: one wavefront per barcode, the pair options of its row 64 per trip, a lane each; the options at or
// above the threshold keep their order through the ballot's prefix count.  live_ptr is the scan of what k_live_pairs<false> counted
// on the same rows with the same threshold, so no entry lies outside the barcode's part of the list.
__global__ __launch_bounds__(256) void k_live_pair_shares(DoubletRows r, const float *__restrict__ share_mean, long long B, float threshold,
                                                          const ull *__restrict__ live_ptr, uint4 *__restrict__ entries)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int p = r.pool_of[b];
    if (p < 0) return;
    const int singles = r.pool_size[p];
    const long long o0 = r.opt_ptr[p];
    const int n_options = (int)(r.opt_ptr[p + 1] - o0);
    const float *__restrict__ row = r.post + r.row_ptr[b];
    const float *__restrict__ shares = share_mean + r.row_ptr[b];
    const ull base = live_ptr[b], end = live_ptr[b + 1];
    ull n = 0;
    for (int k0 = singles; k0 < n_options; k0 += 64) {
        const int k = k0 + lane;
        float posterior = 0.0f;
        bool live = false;
        if (k < n_options) {
            posterior = row[k];
            live = posterior >= threshold;
        }
        const ull found = __ballot(live);
        const ull at = base + n + (ull)__popcll(found & ((1ull << lane) - 1ull));
        if (live && at < end) entries[at] = make_uint4(r.opts[o0 + k], __float_as_uint(posterior), __float_as_uint(shares[k]), 0u);
        n += (ull)__popcll(found);
    }
}

// k_mstep_doublets' walk (mstep_doublets.hip says how a chunk of 64 records is handled) over the 16-byte entries.  The chunk loop is that
// kernel's line for line but for the entry's type: a fix to either is a fix to both.
constexpr int AHEAD = 4;  // list entries a call's own lane fetches with the record

template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mstep_doublet_shares(DoubletSharesMstepArgs x)
{
    const MstepArgs &a = x.w.m;
    const int lane = threadIdx.x & 63;
    const int W = (a.G + 63) >> 6;
    const long long slot = wave_slot();
    if (slot >= walk_slots(x.w)) return;
    const WalkSlot s = walk_slot(x.w, slot);
    const int w = s.w, g = s.g;
    const float *__restrict__ prob_row = s.prob_row;
    double acc = 0.0;
    for (int c0 = 0; c0 < s.n; c0 += 64) {
        const int ci = c0 + lane;
        uint2 d = make_uint2(0u, 0u);
        ull m = 0ull, first = 0ull;
        int n_live = 0;
        if (ci < s.n) {
            d = s.calls[ci];
            m = a.nz[(size_t)d.x * W + w];
            first = x.live_ptr[d.x];
            n_live = (int)(x.live_ptr[d.x + 1] - first);
        }
        const float keep = __uint_as_float(d.y);
        const bool paired = n_live > 0;
        const bool lone = m != 0ull && (m & (m - 1ull)) == 0ull;  // ONE live posterior in the word: fetched by the call's own lane
        const bool one = !paired && lone;
        const int col = lone ? __builtin_ctzll(m) : 0;  // inside the word
        float posterior = 0.0f, contribution = 0.0f;
        if (lone) posterior = a.post[(size_t)d.x * a.K + 64 * w + col];
        if (one) contribution = credit_weight<SQUARE>(posterior, keep, a.power);
        // the first AHEAD entries of the call's list are fetched and their terms computed here, a call per lane
        int ahead_g[AHEAD], ahead_h[AHEAD];  // (an entry with no donor in this word stays out of the additions: -1)
        float ahead_term_g[AHEAD], ahead_term_h[AHEAD];
        bool here = false;
#pragma unroll
        for (int k = 0; k < AHEAD; k++) {
            ahead_g[k] = ahead_h[k] = -1;
            ahead_term_g[k] = ahead_term_h[k] = 0.0f;
            if (k < n_live) pair_terms(x.entries[first + (ull)k], prob_row, w, ahead_g[k], ahead_h[k], ahead_term_g[k], ahead_term_h[k]);
            here = here || ahead_g[k] >= 0;
        }
        ull pending = __ballot(m != 0ull || n_live > AHEAD || here);  // (a short list of pairs of other words' columns: nothing to add here)
        const ull single = __ballot(one);
        const ull lonely = __ballot(lone);
        const ull with_pairs = __ballot(paired);
        while (pending) {
            const int i = __builtin_ctzll(pending);
            pending &= pending - 1ull;
            if ((single >> i) & 1ull) {  // (wave-uniform)
                const int owner = __builtin_amdgcn_readlane(col, i);
                const float c = lane_value(contribution, i);
                if (lane == owner) acc += (double)c;
                continue;
            }
            float credit = 0.0f;
            if ((lonely >> i) & 1ull) {  // (wave-uniform)
                const int owner = __builtin_amdgcn_readlane(col, i);
                const float p = lane_value(posterior, i);
                if (lane == owner) credit = p;
            } else {
                const unsigned cb = (unsigned)__builtin_amdgcn_readlane((int)d.x, i);
                const ull bits = lane_value(m, i);
                if ((bits >> lane) & 1ull) credit = a.post[(size_t)cb * a.K + g];
            }
            if ((with_pairs >> i) & 1ull) {  // (wave-uniform)
                const ull list = lane_value(first, i);
                const int length = __builtin_amdgcn_readlane(n_live, i);
#pragma unroll
                for (int k = 0; k < AHEAD; k++) {  // the entries the call's own lane holds
                    if (k >= length) break;
                    const int jg = __builtin_amdgcn_readlane(ahead_g[k], i), jh = __builtin_amdgcn_readlane(ahead_h[k], i);
                    const float tg = lane_value(ahead_term_g[k], i), th = lane_value(ahead_term_h[k], i);
                    if (g == jg) credit = credit + tg;
                    else if (g == jh) credit = credit + th;
                }
                for (int t0 = AHEAD; t0 < length; t0 += 64) {  // the entries behind them, 64 per trip, a lane each
                    const int t = t0 + lane;
                    int eg = -1, eh = -1;
                    float term_g = 0.0f, term_h = 0.0f;
                    if (t < length) pair_terms(x.entries[list + (ull)t], prob_row, w, eg, eh, term_g, term_h);
                    ull todo = __ballot(eg >= 0);
                    while (todo) {
                        const int j = __builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        const int jg = __builtin_amdgcn_readlane(eg, j), jh = __builtin_amdgcn_readlane(eh, j);
                        const float tg = lane_value(term_g, j), th = lane_value(term_h, j);
                        if (g == jg) credit = credit + tg;
                        else if (g == jh) credit = credit + th;
                    }
                }
            }
            if (credit != 0.0f) acc += (double)credit_weight<SQUARE>(credit, lane_value(keep, i), a.power);  // (+0 adds nothing)
        }
    }
    walk_store(x.w, s, acc);
}

// the weight object of a queued (variant, column): the live singlet's posterior, then the barcode's list walked by the call's lane in
// list order; a call whose credit stays +0 adds nothing
struct DoubletSharesRedoWeight {
    const DoubletSharesMstepArgs &x;
    int g;
    const float *__restrict__ prob_row;
    template <bool SQUARE>
    __device__ __forceinline__ bool call(uint2 d, bool bit, float &c) const
    {
        const MstepArgs &a = x.w.m;
        float credit = 0.0f;
        if (bit) credit = a.post[(size_t)d.x * a.K + g];
        const ull l1 = x.live_ptr[d.x + 1];
        for (ull t = x.live_ptr[d.x]; t < l1; t++) {
            const uint4 pair = x.entries[t];
            const int dg = (int)(pair.x & 0xFFFFu), dh = (int)(pair.x >> 16);
            if (dg != g && dh != g) continue;
            const float share = __uint_as_float(pair.z);
            const float a1 = prob_row[dg] * share, a2 = prob_row[dh] * (1.0f - share);  // (responsibilities' products and sum, one quotient)
            const float own = dg == g ? a1 : a2;
            credit = credit + __uint_as_float(pair.y) * (own == 0.0f ? 0.0f : own / (a1 + a2));
        }
        const bool live = credit != 0.0f;
        if (live) c = credit_weight<SQUARE>(credit, __uint_as_float(d.y), a.power);
        return live;
    }
};

template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mredo_doublet_shares(DoubletSharesMstepArgs x)
{
    mredo_weighted<SQUARE>(x.w, [&x](long long v, int g) { return DoubletSharesRedoWeight{x, g, x.w.prob + (size_t)v * x.w.m.G}; });
}

}  // namespace

hipError_t launch_live_share_fill(hipStream_t st, const DoubletRows &rows, const float *share_mean, long long B, float min_pair_posterior,
                                  const DoubletShareList &list)
{
    if (B <= 0) return hipSuccess;
    if (B > 4ll * 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_live_pair_shares, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, rows, share_mean, B, min_pair_posterior, list.live_ptr,
                       list.entries);
    return hipGetLastError();
}

// what a call keeps on the device for its M-steps (mstep_doublet_shares.h)
struct DoubletSharesRun {
    scratch::Scratch sc;
    DoubletRows rows = {};
    const float *share_mean = nullptr;  // compact like rows.post; null: pools without pair options
    DoubletShareList list = {};
    explicit DoubletSharesRun(dmx_ctx *c) : sc(c) {}
};

void DoubletSharesRunDeleter::operator()(DoubletSharesRun *run) const { delete run; }

// the list's buffers: the entries by the bound, every pair option of every pooled barcode - 16 bytes each -, so that no M-step reads
// the list's length back
static int allocate_list(dmx_ctx *c, DoubletSharesRun &r, long long pair_options)
{
    const size_t B = (size_t)c->B;
    DMX_TRY(r.sc.get(&r.list.count, B + 1));
    DMX_TRY(r.sc.get(&r.list.live_ptr, B + 1));
    DMX_TRY(r.sc.get(&r.list.entries, (size_t)pair_options));
    HIP_TRY(hipMemsetAsync(r.list.count, 0, sizeof(unsigned long long) * (B + 1), c->stream));  // (count[B] stays 0: the scan's last entry is the length)
    return 0;
}

int prepare_doublet_shares_run(dmx_ctx *c, const PairSharesRun &estep, long long pair_options, DoubletSharesRunPtr &run)
{
    run.reset(new DoubletSharesRun(c));
    const PoolEstepArgs a = pools_launch_view(pair_shares_run_pools(estep)).args;
    run->rows = {a.post, a.row_ptr, a.pool_of, a.opt_ptr, a.opts, a.pool_size};
    run->share_mean = pair_shares_run_mean(estep);
    return allocate_list(c, *run, pair_options);
}

int run_mstep_doublet_shares(dmx_ctx *c, float power, float min_pair_posterior, DoubletSharesRun &r)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    DoubletSharesMstepArgs a = {};
    DMX_TRY(begin_weighted_mstep(c, power, a.w));
    a.live_ptr = r.list.live_ptr;
    a.entries = r.list.entries;
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);  // the list: a pass over the E-step's rows
    // (without shares the pools have no pair option: nothing is counted, the scan is all 0 and no walk reads the list)
    if (r.share_mean) HIP_TRY(launch_live_count(st, r.rows, c->B, min_pair_posterior, r.list.count));
    DMX_TRY(scratch::exclusive_scan(r.sc, r.list.count, r.list.live_ptr, 0ull, (size_t)c->B + 1, rocprim::plus<unsigned long long>(), st));
    if (r.share_mean) HIP_TRY(launch_live_share_fill(st, r.rows, r.share_mean, c->B, min_pair_posterior, r.list));
    timer_end(c, DMX_T_ESTEP, ev);
    return run_weighted_mstep(
        c, a.w, [&a](hipStream_t s) { return launch_walk(s, k_mstep_doublet_shares<true>, k_mstep_doublet_shares<false>, a); },
        [&a](hipStream_t s) { return launch_by_power(s, dim3(512), k_mredo_doublet_shares<true>, k_mredo_doublet_shares<false>, a); });
}

int run_mstep_doublet_shares_from_host(dmx_ctx *c, float power, float min_pair_posterior, const PoolsPlan &plan, const float *rows,
                                       const float *shares, long long pair_options)
{
    using namespace dmx::scratch;
    const hipStream_t st = c->stream;
    const size_t B = (size_t)c->B, P = (size_t)plan.n_pools;
    DoubletSharesRunPtr run(new DoubletSharesRun(c));
    Scratch &sc = run->sc;
    long long *d_opt_ptr, *d_row_ptr;
    unsigned *d_opts;
    int *d_pool_size, *d_pool_of;
    float *d_rows, *d_shares;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "");
    DMX_TRY(upload(sc, &d_opt_ptr, plan.opt_ptr.data(), P + 1, st));
    DMX_TRY(upload(sc, &d_opts, plan.opts.data(), plan.opts.size(), st));
    DMX_TRY(upload(sc, &d_pool_size, plan.pool_size.data(), P, st));
    DMX_TRY(upload(sc, &d_pool_of, (const int *)plan.pool_of_barcode, B, st));
    DMX_TRY(upload(sc, &d_row_ptr, (const long long *)plan.row_ptr, B + 1, st));
    DMX_TRY(upload(sc, &d_rows, rows, (size_t)plan.row_ptr[B], st));
    DMX_TRY(upload(sc, &d_shares, shares, (size_t)plan.row_ptr[B], st));
    run->rows = {d_rows, d_row_ptr, d_pool_of, d_opt_ptr, d_opts, d_pool_size};
    run->share_mean = d_shares;
    DMX_TRY(allocate_list(c, *run, pair_options));
    DMX_TRY(run_mstep_doublet_shares(c, power, min_pair_posterior, *run));
    HIP_TRY(hipStreamSynchronize(st));  // (the uploads read the caller's arrays)
    return 0;
}

}  // namespace dmx
