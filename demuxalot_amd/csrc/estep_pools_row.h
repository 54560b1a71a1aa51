// estep_pools_row.h -- the two ends of a pooled row, device code: what k_estep_pools (estep_pools.hip), k_estep_ambient
// (estep_ambient.hip) and k_estep_ambient_grid (estep_ambient_grid.hip) do before and after they walk a barcode's call records, and
// the table of their instantiations.  Included by those three files alone.  One wavefront per barcode.  Lane l, slot s takes option l + 64 s of the barcode's pool; slots entirely past
// the pool's last option are skipped wave-uniformly.  Everything about the row and the pool lives in SGPRs: records by scalar loads,
// a call's row offset as the scalar offset of the buffer loads on the table, the lane's two column offsets fixed for the whole row.
// A kernel is: the early return of a wavefront past the list (in the __global__ function itself), pool_row_open, its own walk over
// row.pbeg .. + row.npairs into acc[], pool_row_close.  The close is the bit-for-bit contract with the reference: the logit, the
// softmax as the exact forms evaluate it (estep_epilogue.h: numpy's exp, reg_row_sum, one division), the compact row, the read-outs.
#pragma once
#include <hip/hip_runtime.h>

#include "estep_epilogue.h"
#include "estep_pools.h"

namespace dmx {

// first maximum, NaN never wins (results.hip: better)
static __device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
constexpr int NO_OPTION = 0x7FFFFFFF;

// what a row keeps in registers between its ends
template <int A>
struct PoolRow {
    int b;                  // the barcode
    int K;                  // options of its pool, 1 .. 64 A
    int n_single;           // of which singlets: the first ones
    int n_slots;            // slots that hold an option
    float pen_pair;         // logit offset of the pair options
    long long pbeg;         // the barcode's records
    int npairs;             // a multiple of 4: rows are padded to 8 calls
    unsigned o1[A], o2[A];  // byte offsets of this lane's column(s) inside a table row
    int kk[A];
    bool valid[A];
};

// from the barcode of this wavefront's place in the list to the lane's option columns and the record range
template <int A>
static __device__ __forceinline__ void pool_row_open(const PoolEstepArgs &a, long long slot, int lane, PoolRow<A> &row)
{
    row.b = __builtin_amdgcn_readfirstlane(a.list[slot]);
    const int p = __builtin_amdgcn_readfirstlane(a.pool_of[row.b]);
    const long long obeg = a.opt_ptr[p];
    row.K = (int)(a.opt_ptr[p + 1] - obeg);
    row.n_single = a.pool_size[p];
    row.pen_pair = a.pair_penalty[p];
    const unsigned *__restrict__ opts = a.opts + obeg;
    row.n_slots = (row.K + 63) >> 6;
#pragma unroll
    for (int s = 0; s < A; s++) {
        const int k = lane + 64 * s;
        row.valid[s] = k < row.K;
        row.kk[s] = row.valid[s] ? k : row.K - 1;  // (a lane without an option repeats the last one: loads stay inside the table)
        const unsigned pr = opts[row.kk[s]];
        row.o1[s] = (pr & 0xFFFFu) * 4u;
        row.o2[s] = (pr >> 16) * 4u;
    }
    row.pbeg = a.pair_ptr[row.b];
    row.npairs = (int)(a.pair_ptr[row.b + 1] - row.pbeg);
}

// acc[s]: the float64 sum of the log terms of option kk[s] over the row's calls in stored order.
// DENSE: the lanes that hold the pool's singlet options also store their posterior at the donor's table column of the barcode's row
// of a.dense ([B, G]: what the M-step reads).  Nothing else of that row is written here - the other columns are the host's zeros.
// (`a` by value: through a reference the compiler orders the reads of a.best / a.best_prob / a.pair_mass behind the stores ahead of
// them; with a copy the single-slot singlet kernels are instruction for instruction what they are with this code in the kernel's body)
template <int A, bool PAIRS, bool DENSE>
static __device__ __forceinline__ void pool_row_close(const PoolEstepArgs a, int lane, const PoolRow<A> &row, const double (&acc)[A])
{
    const int b = row.b, K = row.K, n_single = row.n_single;
    float lg[A], x[A];
    float mx = -__builtin_inff();
#pragma unroll
    for (int s = 0; s < A; s++) {
        const float pen = row.kk[s] >= n_single ? row.pen_pair : 0.0f;
        lg[s] = (float)((double)pen + acc[s]);
        mx = row.valid[s] ? fmaxf(mx, lg[s]) : mx;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
#pragma unroll
    for (int s = 0; s < A; s++) x[s] = npm::exp_f32(lg[s] - mx);
    const float tot = reg_row_sum<64, A>(x, K, lane, 0);
    const long long out_row = a.row_ptr[b];
    float post[A];
    float bv = -__builtin_inff();
    int bi = NO_OPTION;
#pragma unroll
    for (int s = 0; s < A; s++) {
        post[s] = x[s] / tot;
        if (row.valid[s]) {
            a.logits[out_row + row.kk[s]] = lg[s];
            a.post[out_row + row.kk[s]] = post[s];
            if (better(post[s], row.kk[s], bv, bi)) {
                bv = post[s];
                bi = row.kk[s];
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
            if (row.valid[s] && row.kk[s] < n_single) out[row.o1[s] >> 2] = post[s];
    }
}

// The instantiations: option slots per lane (A) and calls per batch (U), the latter as k_estep_direct's exact 64-lane launches have
// them (kernels.hip: launch_estep).  `launch` is called with the one PoolForm of `slots`.
template <int A_, int U_>
struct PoolForm {
    static constexpr int A = A_, U = U_;
};
template <class Launch>
hipError_t launch_pool_form(int slots, Launch &&launch)
{
    switch (slots) {
    case 1: launch(PoolForm<1, 8>{}); break;
    case 2: launch(PoolForm<2, 4>{}); break;
    case 4: launch(PoolForm<4, 2>{}); break;
    case 8: launch(PoolForm<8, 2>{}); break;
    case 16: launch(PoolForm<16, 2>{}); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dmx
