// estep_ambient_grid.hip -- the pooled E-step with every option at its own best ambient fraction (include/demux_hip_debug.h:
// dmx_estep_ambient_grid).  Every option k of a barcode's pool is scored as dmx_estep_ambient scores it, at every
// point j of a grid of fractions:
//   m = q (1 - alphas[j]) + ambient[v] alphas[j],   lambda[b, k, j] = f32( f64(pen) + sum over the calls in stored order of f64( log_f32(m keep + floor) ) )
// and the option's logit is the first maximum of lambda[b, k, .] over j (compared in float32; NaN never wins): the model choice
// between "a contaminated singlet" and "a doublet" happens inside one softmax.  With one grid value the pass is dmx_estep_ambient
// with that fraction for every barcode, bit for bit; column j of the profile is dmx_estep_ambient's logits at alphas[j].
// The two ends of a row are k_estep_pools' own (estep_pools_row.h), the walk between them k_estep_ambient's, with the grid inside it:
// a batch's gathered table entries - what the E-step pays for - serve J grid points, each with a float64 sum per slot of its own; the
// row is walked ceil(n_alphas / J) times, and after every walk the J sums are closed into lambda and compared with the best so far,
// of which the float64 sum and j are kept.  pool_row_close gets the winner's sum, unchanged.  The stream beside the records holds
// ambient[v] itself (k_soup_terms with a fraction of exactly 1: x * 1.0f is x); the wave-uniform product ambient[v] alphas[j] is
// formed once per (pair of calls, j), rounded once, as k_soup_terms forms it for one fraction.
// dmx_estep_ambient_grid_marginal is the same pass with the grid summed: the MARGINAL forms below close every walk into
// a running log-sum-exp over j instead of a running maximum.
#include <hip/hip_runtime.h>

#include <vector>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "estep_ambient.h"
#include "estep_ambient_grid.h"
#include "estep_epilogue.h"
#include "estep_pools_row.h"

namespace dmx {

namespace {

// estep_terms_mixed (estep_ambient.hip) for J fractions on one batch of gathered entries: acc[i][s] is grid point i's sum of slot s
template <int A, bool PAIRS, int H, int J>
__device__ __forceinline__ void grid_terms(npm::f32x2 (&p1)[H][A], const npm::f32x2 (&p2)[H][A], const npm::f32x2 (&keep)[H], const npm::f32x2 (&flo)[H],
                                           const npm::f32x2 (&soup)[H], const float (&alpha)[J], const float (&w0)[J], double (&acc)[J][A], int n_slots,
                                           int n_points)
{
#pragma unroll
    for (int q = 0; q < H; q++) {
        if (PAIRS) {
#pragma unroll
            for (int s = 0; s < A; s++) {
                if (A > 1 && s >= n_slots) continue;  // wave-uniform: slot entirely past the last option
                p1[q][s] = (p1[q][s] + p2[q][s]) * 0.5f;
            }
        }
#pragma unroll
        for (int i = 0; i < J; i++) {
            if (J > 1 && i >= n_points) continue;  // wave-uniform: past the grid's last point
            const npm::f32x2 sa = soup[q] * alpha[i];  // the contract's second product, the same for all lanes, rounded once
#pragma unroll
            for (int s = 0; s < A; s++) {
                if (A > 1 && s >= n_slots) continue;
                const npm::f32x2 own = p1[q][s] * w0[i];  // two products, one sum, each rounded (-ffp-contract=off)
                const npm::f32x2 m = own + sa;
                npm::f32x2 t = m * keep[q];
                t = t + flo[q];
                const npm::f32x2 lp = npm::log_f32_hot2(t);
                acc[i][s] += (double)lp.x;  // call order preserved: 2q before 2q+1
                acc[i][s] += (double)lp.y;
            }
        }
    }
}

// PROFILE: lambda itself is stored after every walk.  A form of its own, because a store ahead of the next walk's wave-uniform
// record loads turns those into vector loads: the form without it keeps every store behind its last walk.
// The best so far per (lane, slot) - the float64 sum and its grid point - is read and written once per walk.  The forms of 4 slots
// and more keep it in LDS (BEST_IN_LDS: 12 bytes per lane and slot, every lane its own entries, so no barrier): in registers it
// would sit on top of the walk's sums and batch for the whole walk and halve the wide forms' occupancy.
// MARGINAL (dmx_estep_ambient_grid_marginal): the grid is summed, not only searched.  With t = lambda + log_weights[j]
// the state per (lane, slot) is the running maximum m of t with its grid point jm and float64 sum, and s = sum of exp(t - m),
// u = sum of alphas[j] exp(t - m), both rescaled when the maximum moves - one exp_f32 per (slot, grid point), at the close of a walk.
// m itself is not kept: it is formed again from the kept sum and log_weights[jm] exactly as it was formed first, so the state is
// 20 bytes per lane and slot and two blocks of the widest form still share a CU's LDS.  log_f32(s), the division and every store
// stay behind the last walk.  In LDS the state is one 16-byte entry and jm beside it, stored whether it changed or not: with four
// arrays and stores under a lane's own condition the 16-slot forms had so many LDS accesses that the compiler no longer proved the
// wave-uniform record loads unclobbered and made them vector loads.
struct alignas(16) MarginalState {  // one 16-byte LDS access per (lane, slot) and direction; jm beside it
    double sum;
    float s, u;
};

template <int A, bool PAIRS, int U, int J, bool PROFILE, bool MARGINAL>
__global__ __launch_bounds__(256) void k_estep_ambient_grid(AmbientGridArgs args)
{
    static_assert(!(PROFILE && MARGINAL), "the profile is the max mode's");
    constexpr bool BEST_IN_LDS = A >= 4;
    __shared__ double lds_sum[BEST_IN_LDS ? 4 * A * 64 : 1];
    __shared__ int lds_j[BEST_IN_LDS ? 4 * A * 64 : 1];
    __shared__ MarginalState lds_state[BEST_IN_LDS && MARGINAL ? 4 * A * 64 : 1];  // (in place of lds_sum)
    const PoolEstepArgs &a = args.pools;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.n_list) return;
    PoolRow<A> row;
    pool_row_open<A>(a, slot, lane, row);
    const int n_alphas = args.n_alphas;
    const long long out_row = PROFILE ? a.row_ptr[row.b] : 0;

    // the best so far per slot: the float64 sum (NaN until a value has won: the logit of an option whose every value is NaN) and
    // its grid point; its float32 value is formed again from the sum where it is compared - exactly as it was formed first
    double best_sum[A];
    int best_j[A];
    float sum_exp[MARGINAL ? A : 1], sum_alpha[MARGINAL ? A : 1];  // MARGINAL: s and u of the slot
    const int mine = (wave * A) * 64 + lane;  // + 64 s: this lane's entry of slot s
#pragma unroll
    for (int s = 0; s < A; s++) {
        best_sum[s] = __builtin_nan("");
        best_j[s] = -1;
        if (MARGINAL) {
            sum_exp[s] = 1.0f;
            sum_alpha[s] = 0.0f;
        }
        if (BEST_IN_LDS) {
            if (MARGINAL)
                lds_state[mine + 64 * s] = MarginalState{best_sum[s], sum_exp[s], sum_alpha[s]};
            else
                lds_sum[mine + 64 * s] = best_sum[s];
            lds_j[mine + 64 * s] = best_j[s];
        }
    }

    const CallPair *__restrict__ recs = a.pairs + row.pbeg;
    const float2 *__restrict__ soup_stream = args.soup + row.pbeg;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.prob, 0, (int)a.prob_bytes, 0x00020000);
    constexpr int H = U / 2;
    static_assert(H == 1 || H == 2 || H == 4, "batches tile a row of whole 8-call groups");
    for (int g0 = 0; g0 < n_alphas; g0 += J) {
        const int n_points = min(J, n_alphas - g0);  // wave-uniform
        float alpha[J], w0[J];
#pragma unroll
        for (int i = 0; i < J; i++) {
            alpha[i] = args.alphas[g0 + min(i, n_points - 1)];  // (a point past the grid repeats the last one and is not used)
            w0[i] = 1.0f - alpha[i];
        }
        double acc[J][A];
#pragma unroll
        for (int i = 0; i < J; i++)
#pragma unroll
            for (int s = 0; s < A; s++) acc[i][s] = 0.0;

        for (int j0 = 0; j0 < row.npairs; j0 += H) {
            RecBatch<A, H, PAIRS> x;
            load_batch<A, H, PAIRS>(x, recs, j0, rsrc, row.o1, row.o2, row.n_slots);
            const int j = __builtin_amdgcn_readfirstlane(j0);  // wave-uniform, as in load_batch: the profile's entries come by scalar loads too
            npm::f32x2 soup[H];
#pragma unroll
            for (int q = 0; q < H; q++) {
                const float2 st = soup_stream[j + q];
                soup[q] = npm::f32x2{st.x, st.y};
            }
            grid_terms<A, PAIRS, H, J>(x.p1, x.p2, x.keep, x.flo, soup, alpha, w0, acc, row.n_slots, n_points);
        }

#pragma unroll
        for (int i = 0; i < J; i++) {
            if (J > 1 && i >= n_points) continue;
            // (formed here, after the walk, every time: left to the compiler, the slots' penalties as float64 and their LDS
            // addresses are hoisted out of the grid's loop and live through the walk - 3 registers per slot, 48 in the widest form.
            // The empty statements tie the two values to this turn of the loop; they are not volatile and name no memory: a
            // volatile one counts as a store, and a store ahead of the next walk turns its record loads into vector loads)
            int at = mine;
            if (BEST_IN_LDS) asm("" : "+v"(at) : "s"(g0));
#pragma unroll
            for (int s = 0; s < A; s++) {
                int kk = row.kk[s];
                if (BEST_IN_LDS) asm("" : "+v"(kk) : "s"(g0));
                const double pen = (double)(kk >= row.n_single ? row.pen_pair : 0.0f);
                const float lambda = (float)(pen + acc[i][s]);
                const int j_so_far = BEST_IN_LDS ? lds_j[at + 64 * s] : best_j[s];
                if constexpr (MARGINAL) {
                    MarginalState st;
                    if (BEST_IN_LDS)
                        st = lds_state[at + 64 * s];
                    else
                        st = MarginalState{best_sum[s], sum_exp[s], sum_alpha[s]};
                    const float t = lambda + args.log_weights[g0 + i];  // (wave-uniform: a scalar load)
                    const float m = (float)(pen + st.sum) + args.log_weights[max(j_so_far, 0)];  // as it was formed when jm won
                    const bool first = j_so_far < 0, moves = first || t > m, counts = t == t;  // a NaN is skipped
                    // one exponential serves the three cases: the old sums shrink (t > m), the new term shrinks (t < m), neither
                    // (t == m, -inf == -inf among them, where the difference is no number)
                    const float e = t == m ? 1.0f : npm::exp_f32(moves ? m - t : t - m);
                    const float s_moved = st.s * e + 1.0f, u_moved = st.u * e + alpha[i];
                    const float s_stays = st.s + e, u_stays = st.u + alpha[i] * e;
                    MarginalState next;  // (stored whether it changed or not: no store under a lane's own condition)
                    next.s = !counts ? st.s : first ? 1.0f : moves ? s_moved : s_stays;
                    next.u = !counts ? st.u : first ? alpha[i] : moves ? u_moved : u_stays;
                    next.sum = counts && moves ? acc[i][s] : st.sum;
                    const int j_next = counts && moves ? g0 + i : j_so_far;
                    if (BEST_IN_LDS) {
                        lds_state[at + 64 * s] = next;
                        lds_j[at + 64 * s] = j_next;
                    } else {
                        best_sum[s] = next.sum;
                        sum_exp[s] = next.s;
                        sum_alpha[s] = next.u;
                        best_j[s] = j_next;
                    }
                    continue;
                }
                const double sum_so_far = BEST_IN_LDS ? lds_sum[at + 64 * s] : best_sum[s];
                const float so_far = (float)(pen + sum_so_far);
                // ascending j: a later value wins only if it is larger; the first value that is no NaN wins over nothing
                if (lambda > so_far || (j_so_far < 0 && lambda == lambda)) {
                    if (BEST_IN_LDS) {
                        lds_sum[at + 64 * s] = acc[i][s];
                        lds_j[at + 64 * s] = g0 + i;
                    } else {
                        best_sum[s] = acc[i][s];
                        best_j[s] = g0 + i;
                    }
                }
                if (PROFILE && row.valid[s]) args.profile[(out_row + row.kk[s]) * n_alphas + (g0 + i)] = lambda;
            }
        }
    }
    if (BEST_IN_LDS && !MARGINAL) {
#pragma unroll
        for (int s = 0; s < A; s++) best_sum[s] = lds_sum[mine + 64 * s];
    }
    float mean[MARGINAL ? A : 1];
    if constexpr (MARGINAL) {
        // the maximum's float64 sum plus the float32 correction log_weights[jm] + log(s): what pool_row_close takes as the row's sum
#pragma unroll
        for (int s = 0; s < A; s++) {
            const int jm = BEST_IN_LDS ? lds_j[mine + 64 * s] : best_j[s];
            MarginalState st;
            if (BEST_IN_LDS)
                st = lds_state[mine + 64 * s];
            else
                st = MarginalState{best_sum[s], sum_exp[s], sum_alpha[s]};
            const float correction = args.log_weights[max(jm, 0)] + npm::log_f32(st.s);
            best_sum[s] = st.sum + (double)correction;  // (NaN stays NaN: the state stayed empty)
            mean[s] = jm < 0 ? __builtin_nanf("") : st.u / st.s;
        }
    }
    pool_row_close<A, PAIRS, false>(a, lane, row, best_sum);
    const long long first = a.row_ptr[row.b];
#pragma unroll
    for (int s = 0; s < A; s++)
        if (row.valid[s]) {
            args.alpha_index[first + row.kk[s]] = BEST_IN_LDS ? lds_j[mine + 64 * s] : best_j[s];
            if constexpr (MARGINAL) args.alpha_mean[first + row.kk[s]] = mean[s];
        }
}

__global__ __launch_bounds__(256) void k_best_alpha_index(long long B, const int *__restrict__ pool_of, const long long *__restrict__ row_ptr,
                                                          const int *__restrict__ best, const int *__restrict__ alpha_index,
                                                          int *__restrict__ best_alpha_index)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int j = -1;
    if (pool_of[b] >= 0) {  // (nothing has written best[b] of a barcode in no pool)
        const int k = best[b];
        if (k >= 0) j = alpha_index[row_ptr[b] + k];
    }
    best_alpha_index[b] = j;
}

// the marginal mode's sibling: the best option's grid point and its posterior mean fraction in one gather
__global__ __launch_bounds__(256) void k_best_alpha_mean(long long B, const int *__restrict__ pool_of, const long long *__restrict__ row_ptr,
                                                         const int *__restrict__ best, const int *__restrict__ alpha_index,
                                                         const float *__restrict__ alpha_mean, int *__restrict__ best_alpha_index,
                                                         float *__restrict__ best_alpha_mean)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int j = -1;
    float mean = __builtin_nanf("");
    if (pool_of[b] >= 0) {
        const int k = best[b];
        if (k >= 0) {
            j = alpha_index[row_ptr[b] + k];
            mean = alpha_mean[row_ptr[b] + k];
        }
    }
    best_alpha_index[b] = j;
    best_alpha_mean[b] = mean;
}

// Grid points per walk (J) by option slots per lane (A): as many as keep the form's registers at its neighbour's occupancy
// (k_estep_ambient's form of the same A) and out of scratch; the wide forms hold their slots' sums and bests and take one.
template <int A>
struct GridPoints {
    static constexpr int J = A == 1 ? 4 : A == 2 ? 2 : 1;
};

template <int A, int U>
void launch_one(hipStream_t st, const AmbientGridArgs &a, bool pairs, bool profile, bool marginal)
{
    constexpr int J = GridPoints<A>::J;
    const dim3 grid((unsigned)((a.pools.n_list + 3) / 4)), block(256);
    if (marginal && pairs)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, true, U, J, false, true>), grid, block, 0, st, a);
    else if (marginal)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, false, U, J, false, true>), grid, block, 0, st, a);
    else if (pairs && profile)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, true, U, J, true, false>), grid, block, 0, st, a);
    else if (pairs)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, true, U, J, false, false>), grid, block, 0, st, a);
    else if (profile)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, false, U, J, true, false>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_estep_ambient_grid<A, false, U, J, false, false>), grid, block, 0, st, a);
}

}  // namespace

hipError_t launch_estep_ambient_grid(hipStream_t st, const AmbientGridArgs &a, int slots, bool pairs, bool profile, bool marginal)
{
    if (a.pools.n_list == 0) return hipSuccess;
    if (a.n_alphas < 1 || a.n_alphas > aplan::MAX_ALPHAS || a.alpha_index == nullptr || (profile && a.profile == nullptr)) return hipErrorInvalidValue;
    if (marginal && (profile || a.log_weights == nullptr || a.alpha_mean == nullptr)) return hipErrorInvalidValue;
    return launch_pool_form(slots, [&](auto form) { launch_one<decltype(form)::A, decltype(form)::U>(st, a, pairs, profile, marginal); });
}

hipError_t launch_best_alpha_index(hipStream_t st, long long B, const int *pool_of, const long long *row_ptr, const int *best, const int *alpha_index,
                                   int *best_alpha_index)
{
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_best_alpha_index, dim3(scratch::grid_for(B)), dim3(256), 0, st, B, pool_of, row_ptr, best, alpha_index, best_alpha_index);
    return hipGetLastError();
}

hipError_t launch_best_alpha_mean(hipStream_t st, long long B, const int *pool_of, const long long *row_ptr, const int *best, const int *alpha_index,
                                  const float *alpha_mean, int *best_alpha_index, float *best_alpha_mean)
{
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_best_alpha_mean, dim3(scratch::grid_for(B)), dim3(256), 0, st, B, pool_of, row_ptr, best, alpha_index, alpha_mean,
                       best_alpha_index, best_alpha_mean);
    return hipGetLastError();
}

int run_estep_ambient_grid(dmx_ctx *c, const PoolsPlan &plan, const AmbientGridScoring &scoring)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const long long B = c->B, V = c->V;
    const hipStream_t st = c->stream;
    const std::vector<float> ones((size_t)B, 1.0f);  // (outlives the temporaries below, which synchronise before they go back)
    PoolsRunPtr run;
    DMX_TRY(prepare_estep_pools(c, plan, false, run));
    const PoolsLaunchView view = pools_launch_view(*run);
    const size_t n_values = B > 0 ? (size_t)plan.row_ptr[B] : 0;
    const bool marginal = scoring.marginal;
    const bool with_profile = !marginal && scoring.profile_out != nullptr;
    // the marginal's prior over the grid: absent means all 0, which adds nothing anywhere (x + 0.0f is x in every comparison and sum here)
    const std::vector<float> no_weights(marginal && !scoring.log_weights ? (size_t)scoring.n_alphas : 0, 0.0f);

    Scratch sc(c);
    float *d_soup = nullptr, *d_ones = nullptr, *d_alphas = nullptr, *d_terms = nullptr, *d_profile = nullptr;
    float *d_log_weights = nullptr, *d_alpha_mean = nullptr, *d_best_mean = nullptr;
    int *d_alpha_index = nullptr, *d_best_alpha = nullptr;
    DMX_TRY(soup_profile(c, sc, marginal ? "dmx_estep_ambient_grid_marginal" : "dmx_estep_ambient_grid", scoring.ambient, scoring.lo, scoring.hi, &d_soup));
    DMX_TRY(upload(sc, &d_ones, ones.data(), (size_t)B, st));
    DMX_TRY(upload(sc, &d_alphas, scoring.alphas, (size_t)scoring.n_alphas, st));
    DMX_TRY(sc.get(&d_terms, 2 * (size_t)c->n_pairs));  // 4 bytes per padded call
    DMX_TRY(sc.get(&d_alpha_index, n_values));
    DMX_TRY(sc.get(&d_best_alpha, (size_t)B));
    if (with_profile) DMX_TRY(sc.get(&d_profile, n_values * (size_t)scoring.n_alphas));
    if (marginal) {
        DMX_TRY(upload(sc, &d_log_weights, scoring.log_weights ? scoring.log_weights : no_weights.data(), (size_t)scoring.n_alphas, st));
        DMX_TRY(sc.get(&d_alpha_mean, n_values));
        DMX_TRY(sc.get(&d_best_mean, (size_t)B));
    }

    // the stream of ambient[v] beside the records: dmx_estep_ambient's prologue with a fraction of exactly 1
    const SoupTermArgs t = soup_term_args(c, view, d_ones, d_soup, d_terms);

    AmbientGridArgs a = {};
    a.pools = view.args;
    a.pools.dense = nullptr;
    a.soup = (const float2 *)d_terms;
    a.alphas = d_alphas;
    a.n_alphas = scoring.n_alphas;
    a.alpha_index = d_alpha_index;
    a.profile = d_profile;
    a.log_weights = d_log_weights;
    a.alpha_mean = d_alpha_mean;
    {
        TimerSpan ev{nullptr, nullptr};
        SpanGuard ev_guard{c, &ev};
        timer_begin(c, DMX_T_ESTEP, &ev);
        HIP_TRY(launch_soup_terms(st, t));
        for (int k = 0; k < POOL_BUCKETS; k++) {
            a.pools.list = view.lists[k];
            a.pools.n_list = view.n_lists[k];
            HIP_TRY(launch_estep_ambient_grid(st, a, pool_bucket_slots(k), view.with_doublets, with_profile, marginal));
        }
        if (marginal)
            HIP_TRY(launch_best_alpha_mean(st, B, view.args.pool_of, view.args.row_ptr, view.args.best, d_alpha_index, d_alpha_mean, d_best_alpha, d_best_mean));
        else
            HIP_TRY(launch_best_alpha_index(st, B, view.args.pool_of, view.args.row_ptr, view.args.best, d_alpha_index, d_best_alpha));
        timer_end(c, DMX_T_ESTEP, ev);
    }
    if (scoring.ambient_out && V) HIP_TRY(hipMemcpyAsync(scoring.ambient_out, d_soup, sizeof(float) * (size_t)V, hipMemcpyDeviceToHost, st));
    if (scoring.alpha_index && n_values) HIP_TRY(hipMemcpyAsync(scoring.alpha_index, d_alpha_index, sizeof(int) * n_values, hipMemcpyDeviceToHost, st));
    if (scoring.best_alpha_index && B) HIP_TRY(hipMemcpyAsync(scoring.best_alpha_index, d_best_alpha, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (marginal && scoring.alpha_mean && n_values) HIP_TRY(hipMemcpyAsync(scoring.alpha_mean, d_alpha_mean, sizeof(float) * n_values, hipMemcpyDeviceToHost, st));
    if (marginal && scoring.best_alpha_mean && B) HIP_TRY(hipMemcpyAsync(scoring.best_alpha_mean, d_best_mean, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (with_profile && n_values)
        HIP_TRY(hipMemcpyAsync(scoring.profile_out, d_profile, sizeof(float) * n_values * (size_t)scoring.n_alphas, hipMemcpyDeviceToHost, st));
    DMX_TRY(read_back_estep_pools(c, *run));  // (synchronises: the uploads read the caller's arrays, the downloads fill them)
    return keep_pools_run(c, *run, &sc, d_alpha_index, d_alpha_mean);
}

}  // namespace dmx
