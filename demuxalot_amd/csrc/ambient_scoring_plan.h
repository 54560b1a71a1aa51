// ambient_scoring_plan.h -- what dmx_estep_ambient (estep_ambient.hip) refuses, as one pure function of plain values:
// the contexts the pass does not run on, everything dmx_estep_pools refuses of the pools (pools_plan.h: the same check()), the
// per-barcode fractions, the soup's profile.  Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp: dmx_estep_ambient asks
// check() before anything is uploaded or launched; tests/ambient_scoring_plan_check.cpp walks it on the CPU.
#pragma once
#include <cstdint>

#include "ambient_plan.h"
#include "pools_plan.h"

namespace dmx {
namespace asplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using aplan::Facts;
using pplan::INVALID;
using pplan::OK;
using pplan::UNSUPPORTED;
using pplan::Pools;
using pplan::Verdict;
using pplan::options_of;

// The two ends of check(), which dmx_estep_ambient_grid's check (ambient_grid_plan.h) puts around its own refusals as well:
// the context and the pools as dmx_estep_pools walks them; the supplied profile.
inline Verdict check_context_and_pools(const Facts &f, const Pools &p)
{
    if (!f.have_problem || !f.have_table) return {INVALID, "call order: a problem and genotype probabilities (dmx_probs_from_betas / dmx_set_probs) come first", -1};
    if (f.attached || f.nranks > 1) return {UNSUPPORTED, "a context with a communicator attached is not supported", -1};
    if (!f.dense_table) return {UNSUPPORTED, "the genotype table is in a padded exchange layout", -1};
    return pplan::check(f.G, f.B, p);
}
inline Verdict check_profile(const Facts &f, const float *ambient)
{
    if (ambient)
        for (long long v = 0; v < f.V; v++)
            if (!aplan::unit_range(ambient[v])) return {INVALID, "an ambient value is not finite or outside [0, 1]", v};
    return {OK, "", -1};
}

// The first of n log weights of a prior over a grid that is not finite, -1: none (ambient_grid_plan.h: check_marginal; pair_shares_plan.h)
inline long long first_log_weight_not_finite(const float *log_weights, long long n)
{
    for (long long j = 0; j < n; j++)
        if (!(log_weights[j] - log_weights[j] == 0.0f)) return j;
    return -1;
}

// The order is the order of the refusals: the context, the pools as dmx_estep_pools walks them, the fractions, the profile.
// alpha[b] of a barcode in no pool is not looked at.
inline Verdict check(const Facts &f, const Pools &p, const float *alpha, const float *ambient)
{
    const Verdict pools = check_context_and_pools(f, p);
    if (pools.status != OK) return pools;
    if (f.B > 0 && !alpha) return {INVALID, "null alpha", -1};
    for (long long b = 0; b < f.B; b++)
        if (p.pool_of_barcode[b] >= 0 && !aplan::unit_range(alpha[b])) return {INVALID, "alpha of a barcode is not finite or outside [0, 1]", b};
    return check_profile(f, ambient);
}

}  // namespace asplan
}  // namespace dmx
