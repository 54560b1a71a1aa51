// estep_grid_device.h -- device inlines of the pooled E-steps that sum every option over a grid (estep_ambient_grid.hip: the MARGINAL
// forms; estep_pair_shares.hip; the frame: DESIGN.md 4.16): the grid points of a walk, the state of a
// running log-sum-exp per (lane, slot) on registers or LDS, the fold of one grid point into it and its finish behind the last walk.
// A form supplies its term function, its kernel and its argument block.
#pragma once
#include <hip/hip_runtime.h>

#include "np_math.h"

namespace dmx {

// Grid points per walk (J) by option slots per lane (A): as many as keep the form's registers at its neighbour's occupancy
// (k_estep_ambient's form of the same A) and out of scratch; the wide forms hold their slots' sums and bests and take one.
template <int A>
struct GridPoints {
    static constexpr int J = A == 1 ? 4 : A == 2 ? 2 : 1;
};

// grid value i of the n_points the walk that starts at g0 takes (a point past the grid repeats the last one and is not used)
__device__ __forceinline__ float grid_value(const float *__restrict__ grid, int g0, int i, int n_points) { return grid[g0 + min(i, n_points - 1)]; }

// With t = lambda + log_weights[j] the state per (lane, slot) is the running maximum m of t with its grid point jm and float64 sum, and
// s = sum of exp(t - m), u = sum of grid[j] exp(t - m), both rescaled when the maximum moves - one exp_f32 per (slot, grid point), at
// the close of a walk.  m itself is not kept: it is formed again from the kept sum and log_weights[jm] exactly as it was formed first,
// so the state is 20 bytes per lane and slot and two blocks of the widest form still share a CU's LDS.
struct alignas(16) GridSumState {  // one 16-byte LDS access per (lane, slot) and direction; jm beside it
    double sum;  // NaN until a value has counted: the logit of an option whose every value is NaN
    float s, u;
};

// The state of a lane's A slots.  Registers for one and two slots.  From four slots on LDS, every lane its own entries, so no barrier:
// in registers the state would sit on top of the walk's sums and batch for the whole walk and halve the wide forms' occupancy.  In LDS
// it is one 16-byte entry and jm beside it, stored whether it changed or not: with four arrays and stores under a lane's own condition
// the 16-slot forms had so many LDS accesses that the compiler no longer proved the wave-uniform record loads unclobbered and made
// them vector loads.  The kernel declares the two arrays (4 A 64 entries each) and forms `at`, this lane's entry of slot 0.
template <int A>
struct GridSums {
    static constexpr bool IN_LDS = A >= 4;
    GridSumState st[IN_LDS ? 1 : A];
    int jm[IN_LDS ? 1 : A];
    GridSumState *lds_st;
    int *lds_jm;

    __device__ __forceinline__ GridSumState &state(int at, int s) { return IN_LDS ? lds_st[at + 64 * s] : st[IN_LDS ? 0 : s]; }
    __device__ __forceinline__ int &point(int at, int s) { return IN_LDS ? lds_jm[at + 64 * s] : jm[IN_LDS ? 0 : s]; }
    __device__ __forceinline__ void load(int at, int s, GridSumState &x, int &j)
    {
        j = point(at, s);
        x = state(at, s);
    }
    __device__ __forceinline__ void store(int at, int s, const GridSumState &x, int j)
    {
        state(at, s) = x;
        point(at, s) = j;
    }
    __device__ __forceinline__ void open(GridSumState *lds_state, int *lds_j, int at)
    {
        lds_st = lds_state;
        lds_jm = lds_j;
#pragma unroll
        for (int s = 0; s < A; s++) store(at, s, GridSumState{__builtin_nan(""), 1.0f, 0.0f}, -1);
    }
};

// Grid point j, of value `value`, folded into a slot's state `was` with its grid point j_was: acc is the slot's float64 sum of the walk,
// pen its penalty.  `alone`: the option knows no grid (a singlet among pairs) - its weight reads as 0 and only the grid's first point
// counts, so s stays 1.  (The next state beside the old one, not in its place: written through one reference the LDS forms took more
// registers.)
__device__ __forceinline__ void grid_fold(const GridSumState &was, int j_was, double pen, double acc, const float *log_weights, int j, float value,
                                          bool alone, GridSumState &next, int &j_next)
{
    const float lw = log_weights[j], lw_was = log_weights[max(j_was, 0)];  // (lw is wave-uniform: a scalar load)
    const float t = (float)(pen + acc) + (alone ? 0.0f : lw);
    const float m = (float)(pen + was.sum) + (alone ? 0.0f : lw_was);  // as it was formed when jm won
    const bool opens = j_was < 0, moves = opens || t > m;
    const bool counts = alone ? j == 0 : t == t;  // a NaN is skipped; a singlet's later points too
    // one exponential serves the three cases: the old sums shrink (t > m), the new term shrinks (t < m), neither
    // (t == m, -inf == -inf among them, where the difference is no number)
    const float e = t == m ? 1.0f : npm::exp_f32(moves ? m - t : t - m);
    const float s_moved = was.s * e + 1.0f, u_moved = was.u * e + value;
    const float s_stays = was.s + e, u_stays = was.u + value * e;
    next.s = !counts ? was.s : opens ? 1.0f : moves ? s_moved : s_stays;  // (stored whether it changed or not: no store under a lane's own condition)
    next.u = !counts ? was.u : opens ? value : moves ? u_moved : u_stays;
    next.sum = counts && moves ? acc : was.sum;
    j_next = counts && moves ? j : j_was;
}

// Behind the last walk, as every store is: the maximum's float64 sum plus the float32 correction log_weights[jm] + log(s) - what
// pool_row_close takes as the row's sum (NaN stays NaN: the state stayed empty) - with the posterior mean over the grid and the grid
// point of the maximum; NaN / -1 where nothing counted, and for an option `alone`, whose correction is 0 + log(1) = +0
__device__ __forceinline__ double grid_finish(const GridSumState &st, int jm, const float *log_weights, bool alone, float &mean, int &index)
{
    const float lw = log_weights[max(jm, 0)];
    const float correction = (alone ? 0.0f : lw) + npm::log_f32(st.s);
    mean = jm < 0 || alone ? __builtin_nanf("") : st.u / st.s;
    index = alone ? -1 : jm;
    return st.sum + (double)correction;
}

}  // namespace dmx
