// ambient_grid_plan.h -- what dmx_estep_ambient_grid (estep_ambient_grid.hip) refuses, as one pure function of plain
// values.  The contexts the pass does not run on, everything dmx_estep_pools refuses of the pools and the supplied profile are not
// restated: they are ambient_scoring_plan.h's two ends (the same pplan::check inside).  What this header adds is the grid, under
// dmx_ambient_profile's rules: 1 .. 64 values, finite, in [0, 1], any order, duplicates allowed.  Host only: nothing of HIP, nothing
// of dmx_ctx.  dmx_steps.cpp: dmx_estep_ambient_grid asks check() before anything is uploaded or launched;
// tests/ambient_grid_plan_check.cpp walks it on the CPU.  check_marginal() is dmx_estep_ambient_grid_marginal's:
// check() and the rule for its log weights; tests/ambient_marginal_plan_check.cpp walks that.
#pragma once
#include "ambient_scoring_plan.h"

namespace dmx {
namespace agplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using aplan::Facts;
using aplan::MAX_ALPHAS;
using pplan::INVALID;
using pplan::OK;
using pplan::UNSUPPORTED;
using pplan::Pools;
using pplan::Verdict;

// The order is the order of the refusals: the context, the pools as dmx_estep_pools walks them, the grid, the profile.
inline Verdict check(const Facts &f, const Pools &p, long long n_alphas, const float *alphas, const float *ambient)
{
    const Verdict pools = asplan::check_context_and_pools(f, p);
    if (pools.status != OK) return pools;
    if (n_alphas < 1) return {INVALID, "the grid needs at least one value", n_alphas};
    static_assert(MAX_ALPHAS == 64, "the text below spells the limit out");
    if (n_alphas > MAX_ALPHAS) return {UNSUPPORTED, "the grid has more than 64 values", n_alphas};
    if (!alphas) return {INVALID, "null alphas", -1};
    for (long long j = 0; j < n_alphas; j++)
        if (!aplan::unit_range(alphas[j])) return {INVALID, "a grid value is not finite or outside [0, 1]", j};
    return asplan::check_profile(f, ambient);
}

// dmx_estep_ambient_grid_marginal: check() and the prior over the grid, log_weights - absent (all 0) or n_alphas finite values.  The
// weights come last: a call that check() refuses is refused with check()'s words.
inline Verdict check_marginal(const Facts &f, const Pools &p, long long n_alphas, const float *alphas, const float *ambient, const float *log_weights)
{
    const Verdict grid = check(f, p, n_alphas, alphas, ambient);
    if (grid.status != OK || !log_weights) return grid;
    const long long j = asplan::first_log_weight_not_finite(log_weights, n_alphas);
    return j < 0 ? grid : Verdict{INVALID, "a log weight is not finite", j};
}

}  // namespace agplan
}  // namespace dmx
