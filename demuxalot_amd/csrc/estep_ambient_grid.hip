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
// a running log-sum-exp over j instead of a running maximum, by the frame of the grid-summed E-steps (estep_grid_device.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "estep_ambient.h"
#include "estep_ambient_grid.h"
#include "estep_epilogue.h"
#include "estep_grid.h"
#include "estep_grid_device.h"
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
// MARGINAL (dmx_estep_ambient_grid_marginal): the grid is summed, not only searched.  The state per (lane, slot), its
// fold at the close of a walk and its finish behind the last walk are the frame's (estep_grid_device.h).
template <int A, bool PAIRS, int U, int J, bool PROFILE, bool MARGINAL>
__global__ __launch_bounds__(256) void k_estep_ambient_grid(AmbientGridArgs args)
{
    static_assert(!(PROFILE && MARGINAL), "the profile is the max mode's");
    constexpr bool BEST_IN_LDS = A >= 4;
    __shared__ double lds_sum[BEST_IN_LDS ? 4 * A * 64 : 1];
    __shared__ int lds_j[BEST_IN_LDS ? 4 * A * 64 : 1];
    __shared__ GridSumState lds_state[BEST_IN_LDS && MARGINAL ? 4 * A * 64 : 1];  // (in place of lds_sum)
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
    const int mine = (wave * A) * 64 + lane;  // + 64 s: this lane's entry of slot s
    GridSums<A> sums;  // MARGINAL: in place of best_sum and best_j
    if constexpr (MARGINAL) sums.open(lds_state, lds_j, mine);
#pragma unroll
    for (int s = 0; s < A; s++) {
        best_sum[s] = __builtin_nan("");
        best_j[s] = -1;
        if (BEST_IN_LDS && !MARGINAL) {
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
            alpha[i] = grid_value(args.alphas, g0, i, n_points);
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
                if constexpr (MARGINAL) {
                    GridSumState st, next;
                    int jm, j_next;
                    sums.load(at, s, st, jm);
                    grid_fold(st, jm, pen, acc[i][s], args.log_weights, g0 + i, alpha[i], false, next, j_next);
                    sums.store(at, s, next, j_next);
                    continue;
                }
                const float lambda = (float)(pen + acc[i][s]);
                const int j_so_far = BEST_IN_LDS ? lds_j[at + 64 * s] : best_j[s];
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
#pragma unroll
        for (int s = 0; s < A; s++) {
            GridSumState st;
            int jm;
            sums.load(mine, s, st, jm);
            best_sum[s] = grid_finish(st, jm, args.log_weights, false, mean[s], best_j[s]);
        }
    }
    pool_row_close<A, PAIRS, false>(a, lane, row, best_sum);
    const long long first = a.row_ptr[row.b];
#pragma unroll
    for (int s = 0; s < A; s++)
        if (row.valid[s]) {
            args.alpha_index[first + row.kk[s]] = BEST_IN_LDS && !MARGINAL ? lds_j[mine + 64 * s] : best_j[s];
            if constexpr (MARGINAL) args.alpha_mean[first + row.kk[s]] = mean[s];
        }
}

template <int A, int U, bool PAIRS>
void launch_one(hipStream_t st, const AmbientGridArgs &a, bool profile, bool marginal)
{
    constexpr int J = GridPoints<A>::J;
    const dim3 grid((unsigned)((a.pools.n_list + 3) / 4)), block(256);
    if (marginal)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, PAIRS, U, J, false, true>), grid, block, 0, st, a);
    else if (profile)
        hipLaunchKernelGGL((k_estep_ambient_grid<A, PAIRS, U, J, true, false>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_estep_ambient_grid<A, PAIRS, U, J, false, false>), grid, block, 0, st, a);
}

}  // namespace

hipError_t launch_estep_ambient_grid(hipStream_t st, const AmbientGridArgs &a, int slots, bool pairs, bool profile, bool marginal)
{
    if (a.pools.n_list == 0) return hipSuccess;
    if (a.n_alphas < 1 || a.n_alphas > aplan::MAX_ALPHAS || a.alpha_index == nullptr || (profile && a.profile == nullptr)) return hipErrorInvalidValue;
    if (marginal && (profile || a.log_weights == nullptr || a.alpha_mean == nullptr)) return hipErrorInvalidValue;
    return launch_pool_form(slots, [&](auto form) {
        constexpr int A = decltype(form)::A, U = decltype(form)::U;
        pairs ? launch_one<A, U, true>(st, a, profile, marginal) : launch_one<A, U, false>(st, a, profile, marginal);
    });
}

int run_estep_ambient_grid(dmx_ctx *c, const PoolsPlan &plan, const AmbientGridScoring &scoring)
{
    using namespace dmx::scratch;
    const long long B = c->B, V = c->V;
    const hipStream_t st = c->stream;
    const std::vector<float> ones((size_t)B, 1.0f);  // (outlives the temporaries below, which synchronise before they go back)
    PoolsRunPtr run;
    DMX_TRY(prepare_estep_pools(c, plan, false, run));
    const PoolsLaunchView view = pools_launch_view(*run);
    const size_t n_values = B > 0 ? (size_t)plan.row_ptr[B] : 0;
    const bool marginal = scoring.marginal;
    const bool with_profile = !marginal && scoring.profile_out != nullptr;

    Scratch sc(c);
    float *d_soup = nullptr, *d_ones = nullptr, *d_alphas = nullptr, *d_terms = nullptr, *d_profile = nullptr, *d_log_weights = nullptr;
    GridOutputs out;
    DMX_TRY(soup_profile(c, sc, marginal ? "dmx_estep_ambient_grid_marginal" : "dmx_estep_ambient_grid", scoring.ambient, scoring.lo, scoring.hi, &d_soup));
    DMX_TRY(upload(sc, &d_ones, ones.data(), (size_t)B, st));
    DMX_TRY(upload(sc, &d_alphas, scoring.alphas, (size_t)scoring.n_alphas, st));
    DMX_TRY(sc.get(&d_terms, 2 * (size_t)c->n_pairs));  // 4 bytes per padded call
    DMX_TRY(out.get(sc, n_values, (size_t)B, marginal));
    if (with_profile) DMX_TRY(sc.get(&d_profile, n_values * (size_t)scoring.n_alphas));
    if (marginal) DMX_TRY(upload_log_weights(sc, &d_log_weights, scoring.log_weights, scoring.n_alphas, st));

    // the stream of ambient[v] beside the records: dmx_estep_ambient's prologue with a fraction of exactly 1
    const SoupTermArgs t = soup_term_args(c, view, d_ones, d_soup, d_terms);

    AmbientGridArgs a = {};
    a.soup = (const float2 *)d_terms;
    a.alphas = d_alphas;
    a.n_alphas = scoring.n_alphas;
    a.alpha_index = out.index;
    a.profile = d_profile;
    a.log_weights = d_log_weights;
    a.alpha_mean = out.mean;
    DMX_TRY(run_grid_estep(c, view, out, [&](hipStream_t s) { return launch_soup_terms(s, t); },
                           [&](hipStream_t s, const PoolEstepArgs &pools, int slots) {
                               a.pools = pools;
                               return launch_estep_ambient_grid(s, a, slots, view.with_doublets, with_profile, marginal);
                           }));
    if (scoring.ambient_out && V) HIP_TRY(hipMemcpyAsync(scoring.ambient_out, d_soup, sizeof(float) * (size_t)V, hipMemcpyDeviceToHost, st));
    DMX_TRY(out.download(st, n_values, (size_t)B, scoring.alpha_index, marginal ? scoring.alpha_mean : nullptr, scoring.best_alpha_index,
                         marginal ? scoring.best_alpha_mean : nullptr));
    if (with_profile && n_values)
        HIP_TRY(hipMemcpyAsync(scoring.profile_out, d_profile, sizeof(float) * n_values * (size_t)scoring.n_alphas, hipMemcpyDeviceToHost, st));
    DMX_TRY(read_back_estep_pools(c, *run));  // (synchronises: the uploads read the caller's arrays, the downloads fill them)
    return keep_pools_run(c, *run, &sc, out.index, out.mean);
}

}  // namespace dmx
