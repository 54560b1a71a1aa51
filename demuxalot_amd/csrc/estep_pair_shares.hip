// estep_pair_shares.hip -- the pooled E-step with every pair option summed over a grid of mixing shares (include/demux_hip_debug.h:
// dmx_estep_pair_shares).  A pair option (d1, d2) of a barcode's pool is scored at every point j of a grid of shares:
//   q = prob[v, d1] shares[j] + prob[v, d2] (1 - shares[j]),   S[b, k, j] = sum over the calls in stored order of f64( log_f32(q keep + floor) )
// and its logit is the log of the weighted sum over j of exp(f32(f64(pen) + S) + log_weights[j]), by the recurrence it shares with
// dmx_estep_ambient_grid_marginal (estep_grid_device.h: grid_fold, grid_finish).  A singlet option is
// dmx_estep_pools' own: the grid and the weights do not enter it.
// The two ends of a row are k_estep_pools' (estep_pools_row.h), the walk between them is its walk with the grid inside it: a batch's
// gathered p1, p2 - what the E-step pays for - serve J grid points, each with a float64 sum per slot of its own; the row is walked
// ceil(n_shares / J) times and every walk is closed into the running log-sum-exp.  pool_row_close gets the largest term's float64 sum
// plus the float32 correction, as the marginal pass hands it over.
// Singlet lanes walk with the weights (1, 0): p * 1 + p * 0 is p (the table has no negative and no non-finite entry), so their sums are
// the pooled pass's; their state is closed from the grid's first point alone with a weight of 0, so s stays 1, log_f32(1) is +0 and the
// close receives the sum itself.  They are recomputed on every walk: n of n (n + 1) / 2 options.  With pairs a pool has at most 44
// donors, so every singlet sits in slot 0: the other slots take their two weights from SGPRs.
// The DENSE form (dmx_estep_pair_shares_resident, dmx_em_doublet_shares) is the same kernel closed with the dense
// pool_row_close; its host side is the pass in three parts - prepare / launch pass / read back (PairSharesRun) - with share_mean kept
// on the device for the M-step between two E-steps (mstep_doublet_shares.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "device_scratch.h"
#include "estep_epilogue.h"
#include "estep_grid.h"
#include "estep_grid_device.h"
#include "estep_pair_shares.h"
#include "estep_pools_row.h"
#include "pair_shares_plan.h"

namespace dmx {

namespace {

static_assert(POOL_MAX_OPTIONS < 64 * 65 / 2, "a pool with pairs and 64 donors or more: singlets beyond slot 0");

// estep_terms (estep_epilogue.h) for J shares on one batch of gathered entries: acc[i][s] is grid point i's sum of slot s.
// own1 / own2: this lane's two weights in slot 0, per grid point; first / second: the weights of every other slot (wave-uniform)
template <int A, int H, int J>
__device__ __forceinline__ void share_terms(const npm::f32x2 (&p1)[H][A], const npm::f32x2 (&p2)[H][A], const npm::f32x2 (&keep)[H],
                                            const npm::f32x2 (&flo)[H], const float (&own1)[J], const float (&own2)[J], const float (&first)[J],
                                            const float (&second)[J], double (&acc)[J][A], int n_slots, int n_points)
{
#pragma unroll
    for (int q = 0; q < H; q++) {
#pragma unroll
        for (int i = 0; i < J; i++) {
            if (J > 1 && i >= n_points) continue;  // wave-uniform: past the grid's last point
#pragma unroll
            for (int s = 0; s < A; s++) {
                if (A > 1 && s >= n_slots) continue;  // wave-uniform: slot entirely past the last option
                const npm::f32x2 a = p1[q][s] * (s == 0 ? own1[i] : first[i]);  // two products, one sum, each rounded (-ffp-contract=off)
                const npm::f32x2 b = p2[q][s] * (s == 0 ? own2[i] : second[i]);
                const npm::f32x2 m = a + b;
                npm::f32x2 t = m * keep[q];
                t = t + flo[q];
                const npm::f32x2 lp = npm::log_f32_hot2(t);
                acc[i][s] += (double)lp.x;  // call order preserved: 2q before 2q+1
                acc[i][s] += (double)lp.y;
            }
        }
    }
}

// The state per (lane, slot), its fold and its finish are the frame's (estep_grid_device.h), with the shares where the
// marginal pass has its fractions: registers for one and two slots, LDS from four slots on.
// DENSE: the close also leaves the barcode's singlet posteriors in a.dense, as k_estep_pools' dense form does (learning under shares:
// mstep_doublet_shares.hip); everything else is the same kernel.
template <int A, int U, int J, bool DENSE>
__global__ __launch_bounds__(256) void k_estep_pair_shares(PairSharesArgs args)
{
    constexpr bool IN_LDS = A >= 4;
    __shared__ GridSumState lds_state[IN_LDS ? 4 * A * 64 : 1];
    __shared__ int lds_j[IN_LDS ? 4 * A * 64 : 1];
    const PoolEstepArgs &a = args.pools;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.n_list) return;
    PoolRow<A> row;
    pool_row_open<A>(a, slot, lane, row);
    const int n_shares = args.n_shares;
    const bool single = row.kk[0] < row.n_single;  // this lane's option of slot 0 is a singlet

    const int mine = (wave * A) * 64 + lane;  // + 64 s: this lane's entry of slot s
    GridSums<A> sums;
    sums.open(lds_state, lds_j, mine);

    const CallPair *__restrict__ recs = a.pairs + row.pbeg;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.prob, 0, (int)a.prob_bytes, 0x00020000);
    constexpr int H = U / 2;
    static_assert(H == 1 || H == 2 || H == 4, "batches tile a row of whole 8-call groups");
    for (int g0 = 0; g0 < n_shares; g0 += J) {
        const int n_points = min(J, n_shares - g0);  // wave-uniform
        float first[J], second[J], own1[J], own2[J];
#pragma unroll
        for (int i = 0; i < J; i++) {
            first[i] = grid_value(args.shares, g0, i, n_points);
            second[i] = 1.0f - first[i];
            own1[i] = single ? 1.0f : first[i];
            own2[i] = single ? 0.0f : second[i];
        }
        double acc[J][A];
#pragma unroll
        for (int i = 0; i < J; i++)
#pragma unroll
            for (int s = 0; s < A; s++) acc[i][s] = 0.0;

        for (int j0 = 0; j0 < row.npairs; j0 += H) {
            RecBatch<A, H, true> x;
            load_batch<A, H, true>(x, recs, j0, rsrc, row.o1, row.o2, row.n_slots);
            share_terms<A, H, J>(x.p1, x.p2, x.keep, x.flo, own1, own2, first, second, acc, row.n_slots, n_points);
        }

#pragma unroll
        for (int i = 0; i < J; i++) {
            if (J > 1 && i >= n_points) continue;
            // (formed here, after the walk, every time; the empty statements tie the LDS address and the option to this turn of the
            // loop, so that neither they nor the penalties as float64 live through the walk - estep_ambient_grid.hip says why they
            // are not volatile)
            int at = mine;
            if (IN_LDS) asm("" : "+v"(at) : "s"(g0));
#pragma unroll
            for (int s = 0; s < A; s++) {
                int kk = row.kk[s];
                if (IN_LDS) asm("" : "+v"(kk) : "s"(g0));
                const bool alone = s == 0 && kk < row.n_single;  // a singlet: the grid's first point, a weight of 0
                const double pen = (double)(kk >= row.n_single ? row.pen_pair : 0.0f);
                GridSumState st, next;
                int jm, j_next;
                sums.load(at, s, st, jm);
                grid_fold(st, jm, pen, acc[i][s], args.log_weights, g0 + i, first[i], alone, next, j_next);
                sums.store(at, s, next, j_next);
            }
        }
    }
    double row_sum[A];  // (every store behind the last walk)
    float mean[A];
    int index[A];
#pragma unroll
    for (int s = 0; s < A; s++) {
        GridSumState st;
        int jm;
        sums.load(mine, s, st, jm);
        row_sum[s] = grid_finish(st, jm, args.log_weights, s == 0 && single, mean[s], index[s]);
    }
    pool_row_close<A, true, DENSE>(a, lane, row, row_sum);
    const long long out_row = a.row_ptr[row.b];
#pragma unroll
    for (int s = 0; s < A; s++)
        if (row.valid[s]) {
            args.share_index[out_row + row.kk[s]] = index[s];
            args.share_mean[out_row + row.kk[s]] = mean[s];
        }
}

template <int A, int U>
void launch_one(hipStream_t st, const PairSharesArgs &a, bool dense)
{
    const dim3 grid((unsigned)((a.pools.n_list + 3) / 4)), block(256);
    if (dense)
        hipLaunchKernelGGL((k_estep_pair_shares<A, U, GridPoints<A>::J, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_estep_pair_shares<A, U, GridPoints<A>::J, false>), grid, block, 0, st, a);
}

}  // namespace

hipError_t launch_estep_pair_shares(hipStream_t st, const PairSharesArgs &a, int slots, bool dense)
{
    if (a.pools.n_list == 0) return hipSuccess;
    if (a.n_shares < 1 || a.n_shares > psplan::MAX_SHARES || !a.shares || !a.log_weights || !a.share_index || !a.share_mean) return hipErrorInvalidValue;
    if (dense && (a.pools.dense == nullptr || a.pools.G <= 0)) return hipErrorInvalidValue;
    return launch_pool_form(slots, [&](auto form) { launch_one<decltype(form)::A, decltype(form)::U>(st, a, dense); });
}

// what a call that learns under shares keeps on the device between its parts (estep_pair_shares.h)
struct PairSharesRun {
    scratch::Scratch sc;
    PoolsRunPtr pools;
    PairSharesScoring scoring;
    const PoolsPlan *plan;
    GridOutputs out;
    PairSharesArgs a = {};
    size_t n_values = 0;
    PairSharesRun(dmx_ctx *c, const PoolsPlan *p, const PairSharesScoring &s) : sc(c), scoring(s), plan(p) {}
};

void PairSharesRunDeleter::operator()(PairSharesRun *run) const { delete run; }

int prepare_pair_shares_run(dmx_ctx *c, const PoolsPlan &plan, const PairSharesScoring &scoring, PairSharesRunPtr &run)
{
    using namespace dmx::scratch;
    const hipStream_t st = c->stream;
    run.reset(new PairSharesRun(c, &plan, scoring));
    PairSharesRun &r = *run;
    r.n_values = c->B > 0 ? (size_t)plan.row_ptr[c->B] : 0;
    DMX_TRY(prepare_estep_pools(c, plan, true, r.pools));
    if (!plan.with_doublets) return 0;  // no pair option anywhere: the dense pooled pass, and nothing to say about shares
    float *d_shares = nullptr, *d_log_weights = nullptr;
    DMX_TRY(upload(r.sc, &d_shares, scoring.shares, (size_t)scoring.n_shares, st));
    DMX_TRY(upload_log_weights(r.sc, &d_log_weights, scoring.log_weights, scoring.n_shares, st));
    DMX_TRY(r.out.get(r.sc, r.n_values, (size_t)c->B, true));
    r.a.shares = d_shares;
    r.a.log_weights = d_log_weights;
    r.a.n_shares = scoring.n_shares;
    r.a.share_index = r.out.index;
    r.a.share_mean = r.out.mean;
    HIP_TRY(hipStreamSynchronize(st));  // (the uploads read the caller's arrays)
    return 0;
}

int launch_pair_shares_pass(dmx_ctx *c, PairSharesRun &r, float power)
{
    using namespace dmx::host;
    if (!r.plan->with_doublets) return launch_estep_pools_pass(c, *r.pools, power);
    const PoolsLaunchView view = pools_launch_view(*r.pools);
    PairSharesArgs a = r.a;
    DMX_TRY(run_grid_estep(c, view, r.out, nullptr, [&](hipStream_t s, const PoolEstepArgs &pools, int slots) {
        a.pools = pools;
        a.pools.dense = c->d_post.p;  // [B, G]: K = G
        return launch_estep_pair_shares(s, a, slots, true);
    }));
    TimerSpan ev{nullptr, nullptr};  // the rebuild of the bitmap and the codes: a second span of the same slot
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);
    DMX_TRY(close_dense_pools_pass(c, power));
    timer_end(c, DMX_T_ESTEP, ev);
    return 0;
}

int read_back_pair_shares(dmx_ctx *c, PairSharesRun &r)
{
    const PairSharesScoring &scoring = r.scoring;
    const size_t B = (size_t)c->B;
    if (r.plan->with_doublets) {
        DMX_TRY(r.out.download(c->stream, r.n_values, B, scoring.share_index, scoring.share_mean, scoring.best_share_index, scoring.best_share_mean));
    } else {
        if (scoring.share_index) std::fill_n(scoring.share_index, r.n_values, -1);
        if (scoring.share_mean) std::fill_n(scoring.share_mean, r.n_values, std::numeric_limits<float>::quiet_NaN());
        if (scoring.best_share_index) std::fill_n(scoring.best_share_index, B, -1);
        if (scoring.best_share_mean) std::fill_n(scoring.best_share_mean, B, std::numeric_limits<float>::quiet_NaN());
    }
    return read_back_estep_pools(c, *r.pools);  // (synchronises)
}

const PoolsRun &pair_shares_run_pools(const PairSharesRun &run) { return *run.pools; }
const float *pair_shares_run_mean(const PairSharesRun &run) { return run.out.mean; }

int run_estep_pair_shares(dmx_ctx *c, const PoolsPlan &plan, const PairSharesScoring &scoring)
{
    using namespace dmx::scratch;
    const long long B = c->B;
    const hipStream_t st = c->stream;
    const size_t n_values = B > 0 ? (size_t)plan.row_ptr[B] : 0;
    PoolsRunPtr run;
    DMX_TRY(prepare_estep_pools(c, plan, false, run));
    if (!plan.with_doublets) {
        // no pair option anywhere: the pooled pass, and nothing to say about shares
        DMX_TRY(launch_estep_pools_pass(c, *run, 2.0f));
        DMX_TRY(read_back_estep_pools(c, *run));
        if (scoring.share_index) std::fill_n(scoring.share_index, n_values, -1);
        if (scoring.share_mean) std::fill_n(scoring.share_mean, n_values, std::numeric_limits<float>::quiet_NaN());
        if (scoring.best_share_index) std::fill_n(scoring.best_share_index, (size_t)B, -1);
        if (scoring.best_share_mean) std::fill_n(scoring.best_share_mean, (size_t)B, std::numeric_limits<float>::quiet_NaN());
        return 0;
    }
    const PoolsLaunchView view = pools_launch_view(*run);

    Scratch sc(c);
    float *d_shares = nullptr, *d_log_weights = nullptr;
    GridOutputs out;
    DMX_TRY(upload(sc, &d_shares, scoring.shares, (size_t)scoring.n_shares, st));
    DMX_TRY(upload_log_weights(sc, &d_log_weights, scoring.log_weights, scoring.n_shares, st));
    DMX_TRY(out.get(sc, n_values, (size_t)B, true));

    PairSharesArgs a = {};
    a.shares = d_shares;
    a.log_weights = d_log_weights;
    a.n_shares = scoring.n_shares;
    a.share_index = out.index;
    a.share_mean = out.mean;
    DMX_TRY(run_grid_estep(c, view, out, nullptr, [&](hipStream_t s, const PoolEstepArgs &pools, int slots) {
        a.pools = pools;
        return launch_estep_pair_shares(s, a, slots);
    }));
    DMX_TRY(out.download(st, n_values, (size_t)B, scoring.share_index, scoring.share_mean, scoring.best_share_index, scoring.best_share_mean));
    return read_back_estep_pools(c, *run);  // (synchronises: the uploads read the caller's arrays, the downloads fill them)
}

}  // namespace dmx
