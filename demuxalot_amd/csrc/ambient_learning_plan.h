// ambient_learning_plan.h -- what dmx_estep_ambient_resident, dmx_mstep_ambient and dmx_em_ambient (mstep_ambient.hip,
// estep_ambient.hip) refuse, as pure functions of plain values.  Host only: nothing of HIP, nothing of dmx_ctx.
// dmx_steps.cpp asks them before anything is uploaded or launched; tests/ambient_learning_plan_check.cpp walks them on the CPU.
#pragma once
#include "ambient_scoring_plan.h"

namespace dmx {
namespace alplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using asplan::Facts;
using asplan::INVALID;
using asplan::OK;
using asplan::Pools;
using asplan::UNSUPPORTED;
using asplan::Verdict;

// a contribution power the M-step can raise to: finite and above 0 (NaN fails the comparison)
inline bool power_valid(float power) { return power > 0.0f && power <= 3.4028234663852886e38f; }

// dmx_em_ambient.  Facts::have_table: the PRIOR BETAS are set (dmx_set_betas / dmx_set_prior_betas) - the call's first step is a
// P-step.  The order is the order of the refusals: the loop's own arguments, then everything dmx_estep_ambient refuses
// (asplan::check: the context - a communicator among the rest -, the pools, the fractions of pooled barcodes, the profile).
inline Verdict check_em(const Facts &f, const Pools &p, int n_iterations, float power, const float *alpha, const float *ambient)
{
    if (n_iterations < 1) return {INVALID, "n_iterations must be >= 1", -1};
    if (!power_valid(power)) return {INVALID, "the contribution power must be finite and above 0", -1};
    return asplan::check(f, p, alpha, ambient);
}

// dmx_mstep_ambient.  Facts::have_table: the table of the last P-step (or dmx_set_probs); have_post: the posteriors of an E-step.
// No pools here: the fraction of EVERY barcode is read.
inline Verdict check_mstep(const Facts &f, bool have_post, float power, const float *alpha, const float *ambient)
{
    if (!f.have_problem) return {INVALID, "call order: a problem comes first", -1};
    if (!f.have_table) return {INVALID, "call order: genotype probabilities (dmx_probs_from_betas / dmx_set_probs) come first", -1};
    if (!have_post) return {INVALID, "call order: an E-step comes first", -1};
    if (f.attached || f.nranks > 1) return {UNSUPPORTED, "a context with a communicator attached is not supported", -1};
    if (!f.dense_table) return {UNSUPPORTED, "the genotype table is in a padded exchange layout", -1};
    if (!power_valid(power)) return {INVALID, "the contribution power must be finite and above 0", -1};
    if (f.B > 0 && !alpha) return {INVALID, "null alpha", -1};
    for (long long b = 0; b < f.B; b++)
        if (!aplan::unit_range(alpha[b])) return {INVALID, "alpha of a barcode is not finite or outside [0, 1]", b};
    return asplan::check_profile(f, ambient);
}

}  // namespace alplan
}  // namespace dmx
