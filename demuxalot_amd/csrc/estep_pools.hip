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
#include "estep_pools_row.h"

namespace dmx {

namespace {

// pool_row_open, the walk as k_estep_direct's exact 64-lane path has it (estep_epilogue.h: load_batch, estep_terms), pool_row_close
template <int A, bool PAIRS, int U, bool DENSE>
__global__ __launch_bounds__(256) void k_estep_pools(PoolEstepArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.n_list) return;
    PoolRow<A> row;
    pool_row_open<A>(a, slot, lane, row);
    double acc[A];
#pragma unroll
    for (int s = 0; s < A; s++) acc[s] = 0.0;

    const CallPair *__restrict__ recs = a.pairs + row.pbeg;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.prob, 0, (int)a.prob_bytes, 0x00020000);
    constexpr int H = U / 2;
    static_assert(H == 1 || H == 2 || H == 4, "batches tile a row of whole 8-call groups");
    for (int j0 = 0; j0 < row.npairs; j0 += H) {
        RecBatch<A, H, PAIRS> x;
        load_batch<A, H, PAIRS>(x, recs, j0, rsrc, row.o1, row.o2, row.n_slots);
        estep_terms<A, PAIRS, H>(x.p1, x.p2, x.keep, x.flo, acc, row.n_slots);
    }
    // close reads a copy of the sums: handed `acc` itself, the array the walk's functions wrote through, the multi-slot kernels set
    // their sums up with other moves and k_estep_ambient<4, false, 2> took two registers more
    double sum[A];
#pragma unroll
    for (int s = 0; s < A; s++) sum[s] = acc[s];
    pool_row_close<A, PAIRS, DENSE>(a, lane, row, sum);
}

template <int A, int U>
void launch_one(hipStream_t st, const PoolEstepArgs &a, bool pairs, bool dense)
{
    const dim3 grid((unsigned)((a.n_list + 3) / 4)), block(256);
    if (pairs && dense)
        hipLaunchKernelGGL((k_estep_pools<A, true, U, true>), grid, block, 0, st, a);
    else if (pairs)
        hipLaunchKernelGGL((k_estep_pools<A, true, U, false>), grid, block, 0, st, a);
    else if (dense)
        hipLaunchKernelGGL((k_estep_pools<A, false, U, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_estep_pools<A, false, U, false>), grid, block, 0, st, a);
}

}  // namespace

hipError_t launch_estep_pools(hipStream_t st, const PoolEstepArgs &a, int slots, bool pairs, bool dense)
{
    if (a.n_list == 0) return hipSuccess;
    if (dense && (a.dense == nullptr || a.G <= 0)) return hipErrorInvalidValue;
    return launch_pool_form(slots, [&](auto form) { launch_one<decltype(form)::A, decltype(form)::U>(st, a, pairs, dense); });
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

int close_dense_pools_pass(dmx_ctx *c, float power)
{
    // the bitmap and the codes of the M-step from the [B, G] matrix, with the floor a full-table E-step of this power takes
    // (dmx_steps.cpp: fill_estep_args); the flags: DESIGN.md 4.15
    const float floor = live_floor_float64(power);
    HIP_TRY(launch_rebuild_nz(c->stream, c->d_post.p, c->B, c->G, c->G, floor, c->d_nz.p, c->G <= 64 ? c->d_first.p : nullptr));
    c->dense_pass_done(floor);
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
    if (r.dense) DMX_TRY(close_dense_pools_pass(c, power));
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

int keep_pools_run(dmx_ctx *c, PoolsRun &r, scratch::Scratch *grid, const int *alpha_index, const float *alpha_mean)
{
    if (!c->keep_pooled) return 0;
    return keep_pooled_result(c, *r.plan, r.a, r.sc, grid, alpha_index, alpha_mean);
}

int run_estep_pools(dmx_ctx *c, const PoolsPlan &plan)
{
    PoolsRunPtr run;
    DMX_TRY(prepare_estep_pools(c, plan, false, run));
    DMX_TRY(launch_estep_pools_pass(c, *run, 2.0f));
    DMX_TRY(read_back_estep_pools(c, *run));
    return keep_pools_run(c, *run);
}

}  // namespace dmx
