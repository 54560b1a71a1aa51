// estep_pair_shares.hip -- the pooled E-step with every pair option summed over a grid of mixing shares (include/demux_hip_debug.h:
// dmx_estep_pair_shares).  A pair option (d1, d2) of a barcode's pool is scored at every point j of a grid of shares:
//   q = prob[v, d1] shares[j] + prob[v, d2] (1 - shares[j]),   S[b, k, j] = sum over the calls in stored order of f64( log_f32(q keep + floor) )
// and its logit is the log of the weighted sum over j of exp(f32(f64(pen) + S) + log_weights[j]), by dmx_estep_ambient_grid_marginal's
// recurrence (estep_ambient_grid.hip: the MARGINAL forms), statement for statement.  A singlet option is
// dmx_estep_pools' own: the grid and the weights do not enter it.
// The two ends of a row are k_estep_pools' (estep_pools_row.h), the walk between them is its walk with the grid inside it: a batch's
// gathered p1, p2 - what the E-step pays for - serve J grid points, each with a float64 sum per slot of its own; the row is walked
// ceil(n_shares / J) times and every walk is closed into the running log-sum-exp.  pool_row_close gets the largest term's float64 sum
// plus the float32 correction, as the marginal pass hands it over.
// Singlet lanes walk with the weights (1, 0): p * 1 + p * 0 is p (the table has no negative and no non-finite entry), so their sums are
// the pooled pass's; their state is closed from the grid's first point alone with a weight of 0, so s stays 1, log_f32(1) is +0 and the
// close receives the sum itself.  They are recomputed on every walk: n of n (n + 1) / 2 options.  With pairs a pool has at most 44
// donors, so every singlet sits in slot 0: the other slots take their two weights from SGPRs.
#include <hip/hip_runtime.h>

#include <limits>
#include <vector>

#include "device_scratch.h"
#include "estep_ambient_grid.h"
#include "estep_epilogue.h"
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

// The state per (lane, slot) is the marginal pass's (estep_ambient_grid.hip): the running maximum's float64 sum and grid point jm,
// s = sum of exp(t - m), u = sum of shares[j] exp(t - m); m is formed again from the kept sum and log_weights[jm] where it is compared.
// Registers for one and two slots; from four slots on one 16-byte LDS entry and jm beside it, every lane its own entries (no barrier),
// stored whether it changed or not - what DESIGN.md 4.10 found about occupancy and about the wave-uniform record loads holds here too.
struct alignas(16) ShareState {
    double sum;
    float s, u;
};

template <int A, int U, int J>
__global__ __launch_bounds__(256) void k_estep_pair_shares(PairSharesArgs args)
{
    constexpr bool IN_LDS = A >= 4;
    __shared__ ShareState lds_state[IN_LDS ? 4 * A * 64 : 1];
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

    double best_sum[A];
    int best_j[A];
    float sum_exp[A], sum_share[A];
    const int mine = (wave * A) * 64 + lane;  // + 64 s: this lane's entry of slot s
#pragma unroll
    for (int s = 0; s < A; s++) {
        best_sum[s] = __builtin_nan("");  // (NaN until a value has counted: the logit of an option whose every value is NaN)
        best_j[s] = -1;
        sum_exp[s] = 1.0f;
        sum_share[s] = 0.0f;
        if (IN_LDS) {
            lds_state[mine + 64 * s] = ShareState{best_sum[s], sum_exp[s], sum_share[s]};
            lds_j[mine + 64 * s] = best_j[s];
        }
    }

    const CallPair *__restrict__ recs = a.pairs + row.pbeg;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.prob, 0, (int)a.prob_bytes, 0x00020000);
    constexpr int H = U / 2;
    static_assert(H == 1 || H == 2 || H == 4, "batches tile a row of whole 8-call groups");
    for (int g0 = 0; g0 < n_shares; g0 += J) {
        const int n_points = min(J, n_shares - g0);  // wave-uniform
        float first[J], second[J], own1[J], own2[J];
#pragma unroll
        for (int i = 0; i < J; i++) {
            first[i] = args.shares[g0 + min(i, n_points - 1)];  // (a point past the grid repeats the last one and is not used)
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
                const float lambda = (float)(pen + acc[i][s]);
                const int j_so_far = IN_LDS ? lds_j[at + 64 * s] : best_j[s];
                ShareState st;
                if (IN_LDS)
                    st = lds_state[at + 64 * s];
                else
                    st = ShareState{best_sum[s], sum_exp[s], sum_share[s]};
                const float lw = args.log_weights[g0 + i], lw_so_far = args.log_weights[max(j_so_far, 0)];
                const float t = lambda + (alone ? 0.0f : lw);
                const float m = (float)(pen + st.sum) + (alone ? 0.0f : lw_so_far);  // as it was formed when jm won
                const bool opens = j_so_far < 0, moves = opens || t > m;
                const bool counts = alone ? g0 + i == 0 : t == t;  // a NaN is skipped; a singlet's later points too
                // one exponential serves the three cases: the old sums shrink (t > m), the new term shrinks (t < m), neither
                // (t == m, -inf == -inf among them, where the difference is no number)
                const float e = t == m ? 1.0f : npm::exp_f32(moves ? m - t : t - m);
                const float s_moved = st.s * e + 1.0f, u_moved = st.u * e + first[i];
                const float s_stays = st.s + e, u_stays = st.u + first[i] * e;
                ShareState next;  // (stored whether it changed or not: no store under a lane's own condition)
                next.s = !counts ? st.s : opens ? 1.0f : moves ? s_moved : s_stays;
                next.u = !counts ? st.u : opens ? first[i] : moves ? u_moved : u_stays;
                next.sum = counts && moves ? acc[i][s] : st.sum;
                const int j_next = counts && moves ? g0 + i : j_so_far;
                if (IN_LDS) {
                    lds_state[at + 64 * s] = next;
                    lds_j[at + 64 * s] = j_next;
                } else {
                    best_sum[s] = next.sum;
                    sum_exp[s] = next.s;
                    sum_share[s] = next.u;
                    best_j[s] = j_next;
                }
            }
        }
    }
    // the maximum's float64 sum plus the float32 correction log_weights[jm] + log(s): what pool_row_close takes as the row's sum
    float mean[A];
    int index[A];
#pragma unroll
    for (int s = 0; s < A; s++) {
        const bool alone = s == 0 && single;
        const int jm = IN_LDS ? lds_j[mine + 64 * s] : best_j[s];
        ShareState st;
        if (IN_LDS)
            st = lds_state[mine + 64 * s];
        else
            st = ShareState{best_sum[s], sum_exp[s], sum_share[s]};
        const float lw = args.log_weights[max(jm, 0)];
        const float correction = (alone ? 0.0f : lw) + npm::log_f32(st.s);  // (a singlet: 0 + log(1) = +0)
        best_sum[s] = st.sum + (double)correction;                          // (NaN stays NaN: the state stayed empty)
        mean[s] = jm < 0 || alone ? __builtin_nanf("") : st.u / st.s;
        index[s] = alone ? -1 : jm;
    }
    pool_row_close<A, true, false>(a, lane, row, best_sum);
    const long long out_row = a.row_ptr[row.b];
#pragma unroll
    for (int s = 0; s < A; s++)
        if (row.valid[s]) {
            args.share_index[out_row + row.kk[s]] = index[s];
            args.share_mean[out_row + row.kk[s]] = mean[s];
        }
}

// Grid points per walk (J) by option slots per lane (A): DESIGN.md 4.8's, for its reasons
template <int A>
struct SharePoints {
    static constexpr int J = A == 1 ? 4 : A == 2 ? 2 : 1;
};

template <int A, int U>
void launch_one(hipStream_t st, const PairSharesArgs &a)
{
    const dim3 grid((unsigned)((a.pools.n_list + 3) / 4)), block(256);
    hipLaunchKernelGGL((k_estep_pair_shares<A, U, SharePoints<A>::J>), grid, block, 0, st, a);
}

}  // namespace

hipError_t launch_estep_pair_shares(hipStream_t st, const PairSharesArgs &a, int slots)
{
    if (a.pools.n_list == 0) return hipSuccess;
    if (a.n_shares < 1 || a.n_shares > psplan::MAX_SHARES || !a.shares || !a.log_weights || !a.share_index || !a.share_mean) return hipErrorInvalidValue;
    return launch_pool_form(slots, [&](auto form) { launch_one<decltype(form)::A, decltype(form)::U>(st, a); });
}

int run_estep_pair_shares(dmx_ctx *c, const PoolsPlan &plan, const PairSharesScoring &scoring)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const long long B = c->B;
    const hipStream_t st = c->stream;
    const size_t n_values = B > 0 ? (size_t)plan.row_ptr[B] : 0;
    PoolsRunPtr run;
    DMX_TRY(prepare_estep_pools(c, plan, false, run));
    if (!plan.with_doublets) {
        // no pair option anywhere: the pooled pass, and nothing to say about shares
        DMX_TRY(launch_estep_pools_pass(c, *run, 2.0f));
        DMX_TRY(read_back_estep_pools(c, *run));
        for (size_t i = 0; i < n_values; i++) {
            if (scoring.share_index) scoring.share_index[i] = -1;
            if (scoring.share_mean) scoring.share_mean[i] = std::numeric_limits<float>::quiet_NaN();
        }
        for (long long b = 0; b < B; b++) {
            if (scoring.best_share_index) scoring.best_share_index[b] = -1;
            if (scoring.best_share_mean) scoring.best_share_mean[b] = std::numeric_limits<float>::quiet_NaN();
        }
        return 0;
    }
    const PoolsLaunchView view = pools_launch_view(*run);
    // the prior over the grid: absent means all 0, which adds nothing anywhere (x + 0.0f is x in every comparison and sum here)
    const std::vector<float> no_weights(scoring.log_weights ? 0 : (size_t)scoring.n_shares, 0.0f);

    Scratch sc(c);
    float *d_shares = nullptr, *d_log_weights = nullptr, *d_share_mean = nullptr, *d_best_mean = nullptr;
    int *d_share_index = nullptr, *d_best_index = nullptr;
    DMX_TRY(upload(sc, &d_shares, scoring.shares, (size_t)scoring.n_shares, st));
    DMX_TRY(upload(sc, &d_log_weights, scoring.log_weights ? scoring.log_weights : no_weights.data(), (size_t)scoring.n_shares, st));
    DMX_TRY(sc.get(&d_share_index, n_values));
    DMX_TRY(sc.get(&d_share_mean, n_values));
    DMX_TRY(sc.get(&d_best_index, (size_t)B));
    DMX_TRY(sc.get(&d_best_mean, (size_t)B));

    PairSharesArgs a = {};
    a.pools = view.args;
    a.pools.dense = nullptr;
    a.shares = d_shares;
    a.log_weights = d_log_weights;
    a.n_shares = scoring.n_shares;
    a.share_index = d_share_index;
    a.share_mean = d_share_mean;
    {
        TimerSpan ev{nullptr, nullptr};
        SpanGuard ev_guard{c, &ev};
        timer_begin(c, DMX_T_ESTEP, &ev);
        for (int k = 0; k < POOL_BUCKETS; k++) {
            a.pools.list = view.lists[k];
            a.pools.n_list = view.n_lists[k];
            HIP_TRY(launch_estep_pair_shares(st, a, pool_bucket_slots(k)));
        }
        // the best option's entries, -1 / NaN where there is none: the marginal pass's gather, a thread per barcode
        HIP_TRY(launch_best_alpha_mean(st, B, view.args.pool_of, view.args.row_ptr, view.args.best, d_share_index, d_share_mean, d_best_index, d_best_mean));
        timer_end(c, DMX_T_ESTEP, ev);
    }
    if (scoring.share_index && n_values) HIP_TRY(hipMemcpyAsync(scoring.share_index, d_share_index, sizeof(int) * n_values, hipMemcpyDeviceToHost, st));
    if (scoring.share_mean && n_values) HIP_TRY(hipMemcpyAsync(scoring.share_mean, d_share_mean, sizeof(float) * n_values, hipMemcpyDeviceToHost, st));
    if (scoring.best_share_index && B) HIP_TRY(hipMemcpyAsync(scoring.best_share_index, d_best_index, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (scoring.best_share_mean && B) HIP_TRY(hipMemcpyAsync(scoring.best_share_mean, d_best_mean, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    return read_back_estep_pools(c, *run);  // (synchronises: the uploads read the caller's arrays, the downloads fill them)
}

}  // namespace dmx
