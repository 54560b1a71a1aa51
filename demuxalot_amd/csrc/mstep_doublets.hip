// mstep_doublets.hip -- the M-step that also learns from doublet posteriors (include/demux_hip_debug.h: dmx_mstep_doublets,
// dmx_em_doublets).  For variant v, donor column g and the calls c of v in stored variant-major order, b = cb_c, in
// float32, every operation rounded (-ffp-contract=off):
//   credit = dense[b, g] when it is live at live_floor_float64(power), else +0
//   for every pair option k of b's row with post[k] >= min_pair_posterior that contains g, in the row's option order, h its other donor:
//       r = prob[v, g] == 0 ? 0 : prob[v, g] / (prob[v, g] + prob[v, h]);   credit = credit + post[k] r      (IEEE division)
//   w = (credit keep_c) ^ power;   addition[v, g] = f32( sum over c of f64(w) )                    one accumulator, in call order
// (power 2: one float32 product; another power: the float64 pow of the float32 base, rounded to float32 once - power_weight)
// r is the donor's responsibility for the call in the even mixture (p_g + p_h) / 2 the pair was scored with.  The weight depends on the
// table of the iteration, so nothing of the fixed-point, tile-major or incremental forms applies: one arithmetic, the float64 sum in
// the reference's order, in the frame of mstep_weighted.h.  This file holds
//   k_live_pairs          a wavefront per barcode compacts the pair part of its row by ballot: <false> counts the options at or above
//                         the threshold, <true> writes them as (g | h << 16, posterior bits) behind the scanned counts, in option order
//   k_mstep_doublets      a wavefront per (work item, 64-column word), lane l owning the float64 sum of column 64 w + l.  A call of a
//                         barcode without live pairs goes k_mstep_ambient's way; a call of one with live pairs is handled by the whole
//                         wavefront at its place in call order
//   k_mredo_doublets      the frame's redo of the queued sums with this weight
// and the list's buffers of a call (DoubletRun).  Per-call data - the record, the bitmap word, the two ends of the barcode's list - are
// fetched a call per lane and broadcast by v_readlane (no uniform 4-byte request per call: DESIGN.md 4.6).  All stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "device_scratch.h"
#include "mstep_doublets.h"
#include "mstep_weighted_device.h"

namespace dmx {

namespace {

typedef unsigned long long ull;

template <bool SQUARE>
__device__ __forceinline__ float credit_weight(float credit, float keep, float power)
{
    return power_weight<SQUARE>(credit * keep, power);
}

// the donor's share of a call in the even mixture of the pair (own + other: float32 addition commutes, so both donors of a pair divide
// by the same sum)
__device__ __forceinline__ float responsibility(float own, float other) { return own == 0.0f ? 0.0f : own / (own + other); }

// One list entry for the columns of word w: both donors' terms post * r, when one of the donors lies in the word (else the entry stays
// out: g = h = -1 as the caller set them)
__device__ __forceinline__ void pair_terms(uint2 entry, const float *__restrict__ prob_row, int w, int &g, int &h, float &term_g, float &term_h)
{
    const int dg = (int)(entry.x & 0xFFFFu), dh = (int)(entry.x >> 16);
    if ((dg >> 6) != w && (dh >> 6) != w) return;
    const float posterior = __uint_as_float(entry.y);
    const float pg = prob_row[dg], ph = prob_row[dh];
    term_g = posterior * responsibility(pg, ph);
    term_h = posterior * responsibility(ph, pg);
    g = dg;
    h = dh;
}

// One wavefront per barcode: the pair options of its row, 64 per trip, a lane each; the options at or above the threshold keep their
// order through the ballot's prefix count.  FILL writes them behind live_ptr[b], which is the scan of what the counting form left, so
// no entry lies outside the barcode's part of the list.
template <bool FILL>
__global__ __launch_bounds__(256) void k_live_pairs(DoubletRows r, long long B, float threshold, ull *__restrict__ count,
                                                    const ull *__restrict__ live_ptr, uint2 *__restrict__ entries)
{
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int p = r.pool_of[b];
    ull n = 0;
    if (p >= 0) {
        const int singles = r.pool_size[p];
        const long long o0 = r.opt_ptr[p];
        const int n_options = (int)(r.opt_ptr[p + 1] - o0);
        const float *__restrict__ row = r.post + r.row_ptr[b];
        const ull base = FILL ? live_ptr[b] : 0ull;
        for (int k0 = singles; k0 < n_options; k0 += 64) {
            const int k = k0 + lane;
            float posterior = 0.0f;
            bool live = false;
            if (k < n_options) {
                posterior = row[k];
                live = posterior >= threshold;
            }
            const ull found = __ballot(live);
            if (FILL && live) entries[base + n + (ull)__popcll(found & ((1ull << lane) - 1ull))] = make_uint2(r.opts[o0 + k], __float_as_uint(posterior));
            n += (ull)__popcll(found);
        }
    }
    if (!FILL && lane == 0) count[b] = n;
}

// One wavefront per (item of a.m.order, word w of the G columns): lane l owns the float64 accumulator of column 64 w + l.  A chunk of 64
// records is loaded a call per lane, with the bitmap word and the ends of the barcode's list.  Without live pairs the call is
// k_mstep_ambient's at fraction 0: one live posterior in the word has its weight computed by the call's own lane, several are handled
// by the whole wavefront.  With live pairs the whole wavefront forms the credits of the word's columns at the call's place in call
// order - also when the bitmap word is empty: the live singlets first (one live posterior comes from the call's own lane), then the
// list - the terms of its first AHEAD entries come from the call's own lane, which fetched them with the record; the entries behind
// them go 64 per trip, a lane each computing both donors' terms -, and the owning lanes add the terms in list order.
constexpr int AHEAD = 4;  // list entries a call's own lane fetches with the record

template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mstep_doublets(DoubletMstepArgs x)
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
        // the first AHEAD entries of the call's list - for most droplets all of them - are fetched and their terms computed here, a call
        // per lane, so that the wavefront's turn at the call starts with no load of the list or the table
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
struct DoubletRedoWeight {
    const DoubletMstepArgs &x;
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
            const uint2 pair = x.entries[t];
            const int dg = (int)(pair.x & 0xFFFFu), dh = (int)(pair.x >> 16);
            if (dg == g) credit = credit + __uint_as_float(pair.y) * responsibility(prob_row[dg], prob_row[dh]);
            else if (dh == g) credit = credit + __uint_as_float(pair.y) * responsibility(prob_row[dh], prob_row[dg]);
        }
        const bool live = credit != 0.0f;
        if (live) c = credit_weight<SQUARE>(credit, __uint_as_float(d.y), a.power);
        return live;
    }
};

template <bool SQUARE>
__global__ __launch_bounds__(256) void k_mredo_doublets(DoubletMstepArgs x)
{
    mredo_weighted<SQUARE>(x.w, [&x](long long v, int g) { return DoubletRedoWeight{x, g, x.w.prob + (size_t)v * x.w.m.G}; });
}

}  // namespace

hipError_t launch_live_count(hipStream_t st, const DoubletRows &rows, long long B, float min_pair_posterior, unsigned long long *count)
{
    if (B <= 0) return hipSuccess;
    if (B > 4ll * 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_live_pairs<false>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, rows, B, min_pair_posterior, count, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_live_fill(hipStream_t st, const DoubletRows &rows, long long B, float min_pair_posterior, const DoubletList &list)
{
    if (B <= 0) return hipSuccess;
    if (B > 4ll * 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_live_pairs<true>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, rows, B, min_pair_posterior, nullptr, list.live_ptr, list.entries);
    return hipGetLastError();
}

// what a call keeps on the device for its M-steps (mstep_doublets.h)
struct DoubletRun {
    scratch::Scratch sc;
    DoubletRows rows = {};
    DoubletList list = {};
    explicit DoubletRun(dmx_ctx *c) : sc(c) {}
};

void DoubletRunDeleter::operator()(DoubletRun *run) const { delete run; }

// the list's buffers: the entries by the bound, every pair option of every pooled barcode - 8 bytes each, what the rows' logits and
// posteriors take together - so that no M-step reads the list's length back
static int allocate_list(dmx_ctx *c, DoubletRun &r, long long pair_options)
{
    const size_t B = (size_t)c->B;
    DMX_TRY(r.sc.get(&r.list.count, B + 1));
    DMX_TRY(r.sc.get(&r.list.live_ptr, B + 1));
    DMX_TRY(r.sc.get(&r.list.entries, (size_t)pair_options));
    HIP_TRY(hipMemsetAsync(r.list.count, 0, sizeof(unsigned long long) * (B + 1), c->stream));  // (count[B] stays 0: the scan's last entry is the length)
    return 0;
}

int prepare_doublet_run(dmx_ctx *c, const PoolsRun &pooled, long long pair_options, DoubletRunPtr &run)
{
    run.reset(new DoubletRun(c));
    const PoolEstepArgs a = pools_launch_view(pooled).args;
    run->rows = {a.post, a.row_ptr, a.pool_of, a.opt_ptr, a.opts, a.pool_size};
    return allocate_list(c, *run, pair_options);
}

int run_mstep_doublets(dmx_ctx *c, float power, float min_pair_posterior, DoubletRun &r)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    DoubletMstepArgs a = {};
    DMX_TRY(begin_weighted_mstep(c, power, a.w));
    a.live_ptr = r.list.live_ptr;
    a.entries = r.list.entries;
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);  // the list: a pass over the E-step's rows
    HIP_TRY(launch_live_count(st, r.rows, c->B, min_pair_posterior, r.list.count));
    DMX_TRY(scratch::exclusive_scan(r.sc, r.list.count, r.list.live_ptr, 0ull, (size_t)c->B + 1, rocprim::plus<unsigned long long>(), st));
    HIP_TRY(launch_live_fill(st, r.rows, c->B, min_pair_posterior, r.list));
    timer_end(c, DMX_T_ESTEP, ev);
    return run_weighted_mstep(
        c, a.w, [&a](hipStream_t s) { return launch_walk(s, k_mstep_doublets<true>, k_mstep_doublets<false>, a); },
        [&a](hipStream_t s) { return launch_by_power(s, dim3(512), k_mredo_doublets<true>, k_mredo_doublets<false>, a); });
}

int run_mstep_doublets_from_host(dmx_ctx *c, float power, float min_pair_posterior, const PoolsPlan &plan, const float *rows, long long pair_options)
{
    using namespace dmx::scratch;
    const hipStream_t st = c->stream;
    const size_t B = (size_t)c->B, P = (size_t)plan.n_pools;
    DoubletRunPtr run(new DoubletRun(c));
    Scratch &sc = run->sc;
    long long *d_opt_ptr, *d_row_ptr;
    unsigned *d_opts;
    int *d_pool_size, *d_pool_of;
    float *d_rows;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "");
    DMX_TRY(upload(sc, &d_opt_ptr, plan.opt_ptr.data(), P + 1, st));
    DMX_TRY(upload(sc, &d_opts, plan.opts.data(), plan.opts.size(), st));
    DMX_TRY(upload(sc, &d_pool_size, plan.pool_size.data(), P, st));
    DMX_TRY(upload(sc, &d_pool_of, (const int *)plan.pool_of_barcode, B, st));
    DMX_TRY(upload(sc, &d_row_ptr, (const long long *)plan.row_ptr, B + 1, st));
    DMX_TRY(upload(sc, &d_rows, rows, (size_t)plan.row_ptr[B], st));
    run->rows = {d_rows, d_row_ptr, d_pool_of, d_opt_ptr, d_opts, d_pool_size};
    DMX_TRY(allocate_list(c, *run, pair_options));
    DMX_TRY(run_mstep_doublets(c, power, min_pair_posterior, *run));
    HIP_TRY(hipStreamSynchronize(st));  // (the uploads read the caller's arrays)
    return 0;
}

}  // namespace dmx
