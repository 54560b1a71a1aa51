// estep_ambient.hip -- the pooled E-step under per-barcode ambient RNA fractions (include/demux_hip_debug.h: dmx_estep_ambient;
// DESIGN.md 4.7).  Every option k of a barcode's pool is scored as dmx_estep_pools scores it, with one change to a call's term:
//   m = q (1 - alpha[b]) + ambient[v] alpha[b],   logit[b, k] = f32( f64(pen) + sum over the calls in stored order of f64( log_f32(m keep + floor) ) )
// q the option's own term (estep_epilogue.h: estep_terms), the mixture dmx_ambient_profile's line (ambient_profile.hip), every
// operation rounded.  With alpha[b] == 0 the mixture IS q (q * 1 + a * 0), so the row is dmx_estep_pools' row bit for bit; a singlet's
// logit with penalty 0 is dmx_ambient_profile's L for that donor and that alpha.
// The two ends of a row are k_estep_pools' own (estep_pools_row.h), and so is the shape of the walk between them.  What the mixture
// adds per call is the same for all lanes: the second product ambient[v] alpha[b].  A 4-byte uniform request per call for
// ambient[v] is what bounded dmx_ambient_profile's first form at 1.7 x the exact E-step, so a prologue
// (k_soup_terms, a call per lane, vector loads) leaves that product as a stream beside the records, 8 bytes per CallPair, which the
// walk fetches with the record - contiguously, through the scalar cache.
#include <hip/hip_runtime.h>

#include "ambient_profile.h"
#include "device_scratch.h"
#include "estep_ambient.h"
#include "estep_epilogue.h"
#include "estep_pools_row.h"

namespace dmx {

namespace {

// One wavefront per barcode of a.order, lane l takes the calls l, l + 64, ... of the padded row: the record's row offset by a vector
// load, the profile's entry of that row, one product - the contract's second one, rounded once.  A padding record (keep 0, floor 1)
// points at row 0 and gets ambient[0] alpha[b]: finite, and multiplied by keep = 0 in the walk.
__global__ __launch_bounds__(256) void k_soup_terms(SoupTermArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.B) return;
    const int b = __builtin_amdgcn_readfirstlane(a.order[slot]);
    if (a.pool_of[b] < 0) return;  // (wave-uniform) nobody reads this row's terms
    const float alpha = a.alpha[b];
    const long long pbeg = a.pair_ptr[b];
    const int ncalls = 2 * (int)(a.pair_ptr[b + 1] - pbeg);
    const unsigned *__restrict__ words = (const unsigned *)(a.pairs + pbeg);  // a record: row_off[2], keep[2], floor[2], reserved[2]
    float *__restrict__ out = a.soup_term + 2 * pbeg;
    for (int call = lane; call < ncalls; call += 64) {
        const unsigned row_off = words[(size_t)(call >> 1) * 8 + (call & 1)];
        out[call] = a.ambient[aplan::row_of(row_off, a.row_shift, a.row_inverse)] * alpha;
    }
}

// estep_terms with the mixture in place of the option's own term: two packed operations per pair of calls more
template <int A, bool PAIRS, int H>
__device__ __forceinline__ void estep_terms_mixed(const npm::f32x2 (&p1)[H][A], const npm::f32x2 (&p2)[H][A], const npm::f32x2 (&keep)[H],
                                                  const npm::f32x2 (&flo)[H], const npm::f32x2 (&soup)[H], float w0, double (&acc)[A], int n_slots)
{
#pragma unroll
    for (int q = 0; q < H; q++) {
#pragma unroll
        for (int s = 0; s < A; s++) {
            if (A > 1 && s >= n_slots) continue;  // wave-uniform: slot entirely past the last option
            npm::f32x2 p = p1[q][s];
            if (PAIRS) p = (p + p2[q][s]) * 0.5f;
            const npm::f32x2 own = p * w0;  // two products, one sum, each rounded (-ffp-contract=off)
            const npm::f32x2 m = own + soup[q];
            npm::f32x2 t = m * keep[q];
            t = t + flo[q];
            const npm::f32x2 lp = npm::log_f32_hot2(t);
            acc[s] += (double)lp.x;  // call order preserved: 2q before 2q+1
            acc[s] += (double)lp.y;
        }
    }
}

// k_estep_pools (estep_pools.hip) with the mixture: w0 and the stream of the soup's terms beside the records.  DENSE: the close also
// leaves the singlet posteriors in a.dense, as k_estep_pools' dense form does (learning under ambient fractions: DESIGN.md 4.9)
template <int A, bool PAIRS, int U, bool DENSE>
__global__ __launch_bounds__(256) void k_estep_ambient(AmbientEstepArgs args)
{
    const PoolEstepArgs &a = args.pools;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long slot = (long long)blockIdx.x * 4 + wave;
    if (slot >= a.n_list) return;
    PoolRow<A> row;
    pool_row_open<A>(a, slot, lane, row);
    const float w0 = 1.0f - args.alpha[row.b];  // wave-uniform for the whole row
    double acc[A];
#pragma unroll
    for (int s = 0; s < A; s++) acc[s] = 0.0;

    const CallPair *__restrict__ recs = a.pairs + row.pbeg;
    const float2 *__restrict__ soup_terms = args.soup_term + row.pbeg;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.prob, 0, (int)a.prob_bytes, 0x00020000);
    constexpr int H = U / 2;
    static_assert(H == 1 || H == 2 || H == 4, "batches tile a row of whole 8-call groups");
    for (int j0 = 0; j0 < row.npairs; j0 += H) {
        RecBatch<A, H, PAIRS> x;
        load_batch<A, H, PAIRS>(x, recs, j0, rsrc, row.o1, row.o2, row.n_slots);
        const int j = __builtin_amdgcn_readfirstlane(j0);  // wave-uniform, as in load_batch: the terms come by scalar loads too
        npm::f32x2 soup[H];
#pragma unroll
        for (int q = 0; q < H; q++) {
            const float2 st = soup_terms[j + q];
            soup[q] = npm::f32x2{st.x, st.y};
        }
        estep_terms_mixed<A, PAIRS, H>(x.p1, x.p2, x.keep, x.flo, soup, w0, acc, row.n_slots);
    }
    // close reads a copy of the sums: handed `acc` itself, the array the walk's functions wrote through, the multi-slot kernels set
    // their sums up with other moves and k_estep_ambient<4, false, 2> took two registers more
    double sum[A];
#pragma unroll
    for (int s = 0; s < A; s++) sum[s] = acc[s];
    pool_row_close<A, PAIRS, DENSE>(a, lane, row, sum);
}

template <int A, int U>
void launch_one(hipStream_t st, const AmbientEstepArgs &a, bool pairs, bool dense)
{
    const dim3 grid((unsigned)((a.pools.n_list + 3) / 4)), block(256);
    if (pairs && dense)
        hipLaunchKernelGGL((k_estep_ambient<A, true, U, true>), grid, block, 0, st, a);
    else if (pairs)
        hipLaunchKernelGGL((k_estep_ambient<A, true, U, false>), grid, block, 0, st, a);
    else if (dense)
        hipLaunchKernelGGL((k_estep_ambient<A, false, U, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_estep_ambient<A, false, U, false>), grid, block, 0, st, a);
}

}  // namespace

hipError_t launch_soup_terms(hipStream_t st, const SoupTermArgs &a)
{
    if (a.B == 0) return hipSuccess;
    hipLaunchKernelGGL(k_soup_terms, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

SoupTermArgs soup_term_args(const dmx_ctx *c, const PoolsLaunchView &view, const float *d_alpha, const float *d_soup, float *d_terms)
{
    SoupTermArgs t = {};
    t.pair_ptr = c->d_pair_ptr.p;
    t.pairs = c->d_call_pairs.p;
    t.order = c->d_bc_order.p;
    t.B = c->B;
    t.pool_of = view.args.pool_of;
    t.alpha = d_alpha;
    t.ambient = d_soup;
    const aplan::RowDivide rows = aplan::row_divide((unsigned)c->G * 4u);
    t.row_shift = rows.shift;
    t.row_inverse = rows.inverse;
    t.soup_term = d_terms;
    return t;
}

hipError_t launch_estep_ambient(hipStream_t st, const AmbientEstepArgs &a, int slots, bool pairs, bool dense)
{
    if (a.pools.n_list == 0) return hipSuccess;
    if (dense && (a.pools.dense == nullptr || a.pools.G <= 0)) return hipErrorInvalidValue;
    return launch_pool_form(slots, [&](auto form) { launch_one<decltype(form)::A, decltype(form)::U>(st, a, pairs, dense); });
}

// what a call under ambient fractions keeps on the device between its parts (estep_ambient.h)
struct AmbientRun {
    scratch::Scratch sc;
    PoolsRunPtr pools;
    AmbientScoring scoring;
    SoupTermArgs t = {};
    AmbientEstepArgs a = {};
    float *d_soup = nullptr, *d_alpha = nullptr;
    bool dense = false;
    bool terms_done = false;
    AmbientRun(dmx_ctx *c, const AmbientScoring &s) : sc(c), scoring(s) {}
};

void AmbientRunDeleter::operator()(AmbientRun *run) const { delete run; }

int prepare_estep_ambient(dmx_ctx *c, const PoolsPlan &plan, const AmbientScoring &scoring, bool dense, AmbientRunPtr &run)
{
    using namespace dmx::scratch;
    using namespace dmx::host;
    const long long B = c->B;
    const hipStream_t st = c->stream;
    run.reset(new AmbientRun(c, scoring));
    AmbientRun &r = *run;
    r.dense = dense;
    DMX_TRY(prepare_estep_pools(c, plan, dense, r.pools));
    const PoolsLaunchView view = pools_launch_view(*r.pools);

    float *d_terms = nullptr;
    DMX_TRY(soup_profile(c, r.sc, scoring.who, scoring.ambient, scoring.lo, scoring.hi, &r.d_soup));
    DMX_TRY(upload(r.sc, &r.d_alpha, scoring.alpha, (size_t)B, st));
    DMX_TRY(r.sc.get(&d_terms, 2 * (size_t)c->n_pairs));  // 4 bytes per padded call

    r.t = soup_term_args(c, view, r.d_alpha, r.d_soup, d_terms);

    r.a.pools = view.args;
    r.a.pools.dense = nullptr;
    r.a.alpha = r.d_alpha;
    r.a.soup_term = (const float2 *)d_terms;
    return 0;
}

// The soup's terms depend on the fractions, the profile and the records, not on the table: the first pass of a run builds the stream
// (inside its span of the DMX_T_ESTEP slot), the later ones of an EM call find it - until ambient_run_replace_soup changes the profile.
int launch_estep_ambient_pass(dmx_ctx *c, AmbientRun &r, float power)
{
    using namespace dmx::host;
    const hipStream_t st = c->stream;
    const PoolsLaunchView view = pools_launch_view(*r.pools);
    AmbientEstepArgs a = r.a;
    a.pools.dense = r.dense ? c->d_post.p : nullptr;  // [B, G]: K = G
    TimerSpan ev{nullptr, nullptr};
    SpanGuard ev_guard{c, &ev};
    timer_begin(c, DMX_T_ESTEP, &ev);
    if (!r.terms_done) {
        HIP_TRY(launch_soup_terms(st, r.t));
        r.terms_done = true;
    }
    for (int k = 0; k < POOL_BUCKETS; k++) {
        a.pools.list = view.lists[k];
        a.pools.n_list = view.n_lists[k];
        HIP_TRY(launch_estep_ambient(st, a, pool_bucket_slots(k), view.with_doublets, r.dense));
    }
    if (r.dense) DMX_TRY(close_dense_pools_pass(c, power));
    timer_end(c, DMX_T_ESTEP, ev);
    return 0;
}

int read_back_estep_ambient(dmx_ctx *c, AmbientRun &r)
{
    const AmbientScoring &scoring = r.scoring;
    if (scoring.ambient_out && c->V)
        HIP_TRY(hipMemcpyAsync(scoring.ambient_out, r.d_soup, sizeof(float) * (size_t)c->V, hipMemcpyDeviceToHost, c->stream));
    return read_back_estep_pools(c, *r.pools);  // (synchronises: the uploads read the caller's arrays, the downloads fill them)
}

const float *ambient_run_alpha(const AmbientRun &run) { return run.d_alpha; }
const float *ambient_run_soup(const AmbientRun &run) { return run.d_soup; }

int ambient_run_replace_soup(dmx_ctx *c, AmbientRun &r, const float *d_profile)
{
    HIP_TRY(hipMemcpyAsync(r.d_soup, d_profile, sizeof(float) * ((size_t)c->V + 1), hipMemcpyDeviceToDevice, c->stream));
    r.terms_done = false;
    return 0;
}

int run_estep_ambient(dmx_ctx *c, const PoolsPlan &plan, const AmbientScoring &scoring)
{
    AmbientRunPtr run;
    DMX_TRY(prepare_estep_ambient(c, plan, scoring, false, run));
    DMX_TRY(launch_estep_ambient_pass(c, *run, 2.0f));
    DMX_TRY(read_back_estep_ambient(c, *run));
    return keep_pools_run(c, *run->pools);
}

}  // namespace dmx
