// mstep_weighted.h -- the frame of the M-steps whose per-call weight reads the table of the iteration (mstep_weighted.hip; the forms:
// mstep_ambient.h, mstep_doublets.h, mstep_doublet_shares.h, mstep_soup.h): the argument block they share, the host steps around their launches, and the
// combining pass of the variants that span several work items.  What a form's weight reads comes behind this block in the form's own.
#pragma once
#include <functional>

#include <hip/hip_runtime.h>

#include "kernels.h"

struct dmx_ctx;

namespace dmx {

// the work items, the records, the posteriors and the bitmap of MstepArgs (float64 form: partial, item_variant, item_ptr, out32,
// redo_cap; nothing of the fixed-point or tile forms), the table, and the redo queue
struct WeightedMstepArgs {
    MstepArgs m;
    const float *prob;          // [V, G] the genotype table the E-step of these posteriors read
    long long V;
    unsigned long long *redo;   // [m.redo_cap] (variant << 16 | genotype) of the sums to be redone in call order
    unsigned *n_redo;           // [2] their number, and 0 (the context's two counters, zeroed by the launcher: dmx_get_redo_count adds them)
};

// The context's half of such an M-step: the codes are rebuilt first when they were written above live_floor_float64(power) (a
// fixed-point M-step may have asked the E-step for a higher floor), then `a` is filled from the context's posteriors (d_post, singlet
// columns; d_nz), records, work items and table (d_prob), with d_add as the result; the context's flags:
// ctx_state.h addition_written_by_other_form.  out (mstep_soup.hip): [V, G] of the caller's that takes the sums in
// place of d_add - the addition and its flags then stay as they are.
int begin_weighted_mstep(dmx_ctx *c, float power, WeightedMstepArgs &a, float *out = nullptr);

// k_mcombine_weighted over [V, G] behind the zeroing of the two counters; the form's redo over the queue follows it
hipError_t launch_mcombine_weighted(hipStream_t st, const WeightedMstepArgs &a);

// The launches of one M-step on the context's stream: `walk` counted in DMX_T_MSTEP; the combining pass and `redo` in DMX_T_MCOMBINE
// (the forms' launches: mstep_weighted_device.h, launch_walk and launch_by_power)
int run_weighted_mstep(dmx_ctx *c, const WeightedMstepArgs &a, const std::function<hipError_t(hipStream_t)> &walk,
                       const std::function<hipError_t(hipStream_t)> &redo);

}  // namespace dmx
