// estep_pools.hip -- the pooled E-step: every barcode against the donors of its own pool (include/demux_hip_debug.h:
// dmx_estep_pools).  The arithmetic is the exact E-step's, operation for operation (estep_epilogue.h:
// estep_terms<A, true, H>, numpy's exp, reg_row_sum, one division), so a barcode's row equals, bit for bit, what the
// reference computes for the genotype list of its pool on the column subset of the same table.  What differs from
// k_estep_direct's 64-lane path is where a lane's two table columns come from - the option list of the barcode's pool instead
// of the one global list - and that the rows are compact: row_ptr[b] .. row_ptr[b + 1].
// Learning within pools (dmx_estep_pools_resident, dmx_em_pools) runs the DENSE form of the same kernel, which also
// leaves the singlet posteriors as a [B, G] matrix for the M-step; the host half is prepare / launch / read back, so that a call of
// several E-steps prepares and reads back once.
#include <hip/hip_runtime.h>

#include <limits>

#include "device_scratch.h"
#include "estep_epilogue.h"
#include "estep_pools.h"

namespace dmx {

namespace {

// first maximum, NaN never wins (results.hip: better)
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
constexpr int NO_OPTION = 0x7FFFFFFF;

// One wavefront per barcode.  Lane l, slot s takes option l + 64 s of the barcode's pool; slots entirely past the pool's last
// option are skipped wave-uniformly.  Everything about the row and the pool lives in SGPRs: records by scalar loads, a call's row
// offset as the scalar offset of the buffer loads on the table, the lane's two column offsets fixed for the whole row.
// DENSE: the lanes that hold the pool's singlet options also store their posterior at the donor's table column of the barcode's row
// of a.dense ([B, G]: what the M-step reads).  Nothing else of that row is written here - the other columns are the host's zeros.
template <int A, bool PAIRS, int U, bool DENSE>
__global__ __launch_bounds__(256) void k_estep_pools(PoolEstepArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.n_list) return;
    const int b = __builtin_amdgcn_readfirstlane(a.list[slot]);
    const int p = __builtin_amdgcn_readfirstlane(a.pool_of[b]);
    const long long obeg = a.opt_ptr[p];
    const int K = (int)(a.opt_ptr[p + 1] - obeg);  // 1 .. 64 A
    const int n_single = a.pool_size[p];
    const float pen_pair = a.pair_penalty[p];
    const unsigned *__restrict__ opts = a.opts + obeg;
    const int n_slots = (K + 63) >> 6;

    unsigned o1[A], o2[A];  // byte offsets of this lane's column(s) inside a table row
    int kk[A];
    bool valid[A];
#pragma unroll
    for (int s = 0; s < A; s++) {
        const int k = lane + 64 * s;
        valid[s] = k < K;
        kk[s] = valid[s] ? k : K - 1;  // (a lane without an option repeats the last one: loads stay inside the table)
        const unsigned pr = opts[kk[s]];
        o1[s] = (pr & 0xFFFFu) * 4u;
        o2[s] = (pr >> 16) * 4u;
    }
    double acc[A];
#pragma unroll
    for (int s = 0; s < A; s++) acc[s] = 0.0;

    const long long pbeg = a.pair_ptr[b];
    const int npairs = (int)(a.pair_ptr[b + 1] - pbeg);  // a multiple of 4: rows are padded to 8 calls
    const CallPair *__restrict__ recs = a.pairs + pbeg;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.prob, 0, (int)a.prob_bytes, 0x00020000);
    constexpr int H = U / 2;
    static_assert(H == 1 || H == 2 || H == 4, "batches tile a row of whole 8-call groups");
    for (int j0 = 0; j0 < npairs; j0 += H) {
        RecBatch<A, H, PAIRS> x;
        load_batch<A, H, PAIRS>(x, recs, j0, rsrc, o1, o2, n_slots);
        estep_terms<A, PAIRS, H>(x.p1, x.p2, x.keep, x.flo, acc, n_slots);
    }

    // ---- epilogue: the logit, the softmax as the exact forms evaluate it, the compact row, the two read-outs ----
    float lg[A], x[A];
    float mx = -__builtin_inff();
#pragma unroll
    for (int s = 0; s < A; s++) {
        const float pen = kk[s] >= n_single ? pen_pair : 0.0f;
        lg[s] = (float)((double)pen + acc[s]);
        mx = valid[s] ? fmaxf(mx, lg[s]) : mx;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
#pragma unroll
    for (int s = 0; s < A; s++) x[s] = npm::exp_f32(lg[s] - mx);
    const float tot = reg_row_sum<64, A>(x, K, lane, 0);
    const long long row = a.row_ptr[b];
    float post[A];
    float bv = -__builtin_inff();
    int bi = NO_OPTION;
#pragma unroll
    for (int s = 0; s < A; s++) {
        post[s] = x[s] / tot;
        if (valid[s]) {
            a.logits[row + kk[s]] = lg[s];
            a.post[row + kk[s]] = post[s];
            if (better(post[s], kk[s], bv, bi)) {
                bv = post[s];
                bi = kk[s];
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    // the pair posteriors, widened to float64 and added in ascending option order: the order is the contract, so the sum is a
    // sequential one; option k sits in lane k % 64 of slot k / 64 and comes out by v_readlane (k is wave-uniform)
    double mass = 0.0;
    if (PAIRS) {
#pragma unroll
        for (int s = 0; s < A; s++) {
            const int lo = max(n_single - 64 * s, 0), hi = min(K - 64 * s, 64);
            for (int l = lo; l < hi; l++)
                mass += (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, post[s]), l));
        }
    }
    if (lane == 0) {
        a.best[b] = bi != NO_OPTION ? bi : -1;
        a.best_prob[b] = bi != NO_OPTION ? bv : __builtin_nanf("");
        a.pair_mass[b] = mass;
    }
    if (DENSE) {
        // with pairs a pool has at most 44 donors (POOL_MAX_OPTIONS): its singlets are all in slot 0
        static_assert(POOL_MAX_OPTIONS < 64 * 65 / 2, "a pool with pairs and 64 donors or more: singlets beyond slot 0");
        constexpr int SINGLET_SLOTS = PAIRS ? 1 : A;
        float *__restrict__ out = a.dense + (long long)b * a.G;
#pragma unroll
        for (int s = 0; s < SINGLET_SLOTS; s++)
            if (valid[s] && kk[s] < n_single) out[o1[s] >> 2] = post[s];
    }
}

template <int A, int U, bool DENSE>
void launch_form(hipStream_t st, const PoolEstepArgs &a, bool pairs)
{
    const dim3 grid((unsigned)((a.n_list + 3) / 4)), block(256);
    if (pairs)
        hipLaunchKernelGGL((k_estep_pools<A, true, U, DENSE>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_estep_pools<A, false, U, DENSE>), grid, block, 0, st, a);
}

template <int A, int U>
void launch_one(hipStream_t st, const PoolEstepArgs &a, bool pairs, bool dense)
{
    if (dense)
        launch_form<A, U, true>(st, a, pairs);
    else
        launch_form<A, U, false>(st, a, pairs);
}

}  // namespace

// calls per batch as k_estep_direct's exact 64-lane launches have them (kernels.hip: launch_estep)
hipError_t launch_estep_pools(hipStream_t st, const PoolEstepArgs &a, int slots, bool pairs, bool dense)
{
    if (a.n_list == 0) return hipSuccess;
    if (dense && (a.dense == nullptr || a.G <= 0)) return hipErrorInvalidValue;
    switch (slots) {
    case 1: launch_one<1, 8>(st, a, pairs, dense); break;
    case 2: launch_one<2, 4>(st, a, pairs, dense); break;
    case 4: launch_one<4, 2>(st, a, pairs, dense); break;
    case 8: launch_one<8, 2>(st, a, pairs, dense); break;
    case 16: launch_one<16, 2>(st, a, pairs, dense); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// what a pooled call keeps on the device between its parts (estep_pools.h)
struct PoolsRun {
    scratch::Scratch sc;
    const PoolsPlan *plan;
    PoolEstepArgs a = {};
    int *d_lists[POOL_BUCKETS] = {};
    long long n_lists[POOL_BUCKETS] = {};
    long long n_values = 0;
    bool dense = false;
    PoolsRun(dmx_ctx *c, const PoolsPlan *p) : sc(c), plan(p) {}
};

void PoolsRunDeleter::operator()(PoolsRun *run) const { delete run; }

int prepare_estep_pools(dmx_ctx *c, const PoolsPlan &plan, bool dense, PoolsRunPtr &run)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const long long B = c->B, P = plan.n_pools;
    const hipStream_t st = c->stream;
    run.reset(new PoolsRun(c, &plan));
    PoolsRun &r = *run;
    r.dense = dense;
    r.n_values = B > 0 ? (long long)plan.row_ptr[B] : 0;

    // the barcodes of every bucket, longest rows first: the context's `order` filtered, so a launch's tail is its shortest rows
    std::vector<int> order((size_t)B);
    if (B) {
        HIP_TRY(hipMemcpyAsync(order.data(), c->d_bc_order.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    std::vector<int> lists[POOL_BUCKETS];
    for (long long j = 0; j < B; j++) {
        const int b = order[(size_t)j];
        const int p = plan.pool_of_barcode[b];
        if (p < 0) continue;
        lists[pool_bucket_of((int)(plan.opt_ptr[(size_t)p + 1] - plan.opt_ptr[(size_t)p]))].push_back(b);
    }

    Scratch &sc = r.sc;
    PoolEstepArgs &a = r.a;
    a.pair_ptr = c->d_pair_ptr.p;
    a.pairs = c->d_call_pairs.p;
    a.prob = c->d_prob.p;
    a.prob_bytes = (unsigned)((unsigned long long)c->prob_rows * c->G * 4ull);
    long long *d_opt_ptr, *d_row_ptr;
    unsigned *d_opts;
    int *d_pool_size, *d_pool_of;
    float *d_pen;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "");
    DMX_TRY(upload(sc, &d_opt_ptr, plan.opt_ptr.data(), (size_t)P + 1, st));
    DMX_TRY(upload(sc, &d_opts, plan.opts.data(), plan.opts.size(), st));
    DMX_TRY(upload(sc, &d_pool_size, plan.pool_size.data(), (size_t)P, st));
    DMX_TRY(upload(sc, &d_pen, plan.pair_penalty, (size_t)P, st));
    DMX_TRY(upload(sc, &d_pool_of, (const int *)plan.pool_of_barcode, (size_t)B, st));
    DMX_TRY(upload(sc, &d_row_ptr, (const long long *)plan.row_ptr, (size_t)B + 1, st));
    a.opt_ptr = d_opt_ptr;
    a.opts = d_opts;
    a.pool_size = d_pool_size;
    a.pair_penalty = d_pen;
    a.pool_of = d_pool_of;
    a.row_ptr = d_row_ptr;
    DMX_TRY(sc.get(&a.logits, (size_t)r.n_values));
    DMX_TRY(sc.get(&a.post, (size_t)r.n_values));
    DMX_TRY(sc.get(&a.best, (size_t)B));
    DMX_TRY(sc.get(&a.best_prob, (size_t)B));
    DMX_TRY(sc.get(&a.pair_mass, (size_t)B));
    a.G = c->G;
    for (int k = 0; k < POOL_BUCKETS; k++) {
        DMX_TRY(upload(sc, &r.d_lists[k], lists[k].data(), lists[k].size(), st));
        r.n_lists[k] = (long long)lists[k].size();
    }
    HIP_TRY(hipStreamSynchronize(st));  // `lists` are locals
    return 0;
}

int launch_estep_pools_pass(dmx_ctx *c, PoolsRun &r, float power)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    PoolEstepArgs a = r.a;
    a.dense = r.dense ? c->d_post.p : nullptr;  // [B, G]: K = G
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);
    for (int k = 0; k < POOL_BUCKETS; k++) {
        a.list = r.d_lists[k];
        a.n_list = r.n_lists[k];
        HIP_TRY(launch_estep_pools(st, a, pool_bucket_slots(k), r.plan->with_doublets, r.dense));
    }
    if (r.dense) {
        // the bitmap and the codes of the M-step from the [B, G] matrix, with the floor a full-table E-step of this power takes
        // (dmx_steps.cpp: fill_estep_args); the context as run_estep leaves it, without statistics of the dense calls
        const float floor = power == 2.0f ? NZ_FLOOR_SQUARE : 0.0f;
        HIP_TRY(launch_rebuild_nz(st, c->d_post.p, c->B, c->G, c->G, floor, c->d_nz.p, c->G <= 64 ? c->d_first.p : nullptr));
        c->post_gathered = false;
        c->dense_stat_valid = false;
        c->nz_floor = floor;
        c->guard_ran = false;
        c->have_post = true;
        c->logits_readable = false;  // (d_logits holds nothing of this pass)
    }
    timer_end(c, DMX_T_ESTEP, ev);
    return 0;
}

int read_back_estep_pools(dmx_ctx *c, PoolsRun &r)
{
    using namespace dmx::host;
    const long long B = c->B, n_values = r.n_values;
    const hipStream_t st = c->stream;
    const PoolsPlan &plan = *r.plan;
    const PoolEstepArgs &a = r.a;
    if (plan.logits_out && n_values) HIP_TRY(hipMemcpyAsync(plan.logits_out, a.logits, sizeof(float) * (size_t)n_values, hipMemcpyDeviceToHost, st));
    if (plan.probs_out && n_values) HIP_TRY(hipMemcpyAsync(plan.probs_out, a.post, sizeof(float) * (size_t)n_values, hipMemcpyDeviceToHost, st));
    if (plan.best_option && B) HIP_TRY(hipMemcpyAsync(plan.best_option, a.best, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (plan.best_prob && B) HIP_TRY(hipMemcpyAsync(plan.best_prob, a.best_prob, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (plan.doublet_mass && B) HIP_TRY(hipMemcpyAsync(plan.doublet_mass, a.pair_mass, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (long long b = 0; b < B; b++) {  // no launch visits the barcodes of no pool
        if (plan.pool_of_barcode[b] >= 0) continue;
        if (plan.best_option) plan.best_option[b] = -1;
        if (plan.best_prob) plan.best_prob[b] = std::numeric_limits<float>::quiet_NaN();
        if (plan.doublet_mass) plan.doublet_mass[b] = std::numeric_limits<double>::quiet_NaN();
    }
    return 0;
}

PoolsLaunchView pools_launch_view(const PoolsRun &run)
{
    PoolsLaunchView view = {};
    view.args = run.a;
    for (int k = 0; k < POOL_BUCKETS; k++) {
        view.lists[k] = run.d_lists[k];
        view.n_lists[k] = run.n_lists[k];
    }
    view.with_doublets = run.plan->with_doublets;
    return view;
}

int run_estep_pools(dmx_ctx *c, const PoolsPlan &plan)
{
    PoolsRunPtr run;
    DMX_TRY(prepare_estep_pools(c, plan, false, run));
    DMX_TRY(launch_estep_pools_pass(c, *run, 2.0f));
    return read_back_estep_pools(c, *run);
}

}  // namespace dmx
