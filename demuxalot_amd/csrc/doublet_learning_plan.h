// doublet_learning_plan.h -- what dmx_em_doublets and dmx_mstep_doublets (mstep_doublets.hip) refuse, as pure functions
// of plain values.  Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp asks them before anything is uploaded or launched;
// tests/doublet_learning_plan_check.cpp walks them on the CPU.
#pragma once
#include "ambient_learning_plan.h"

namespace dmx {
namespace dlplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using alplan::power_valid;
using asplan::Facts;
using asplan::INVALID;
using asplan::OK;
using asplan::Pools;
using asplan::UNSUPPORTED;
using asplan::Verdict;

// a pair's posterior is credited at or above the threshold: finite and above 0 (NaN fails the comparison).  Above 1: no pair is.
inline bool threshold_valid(float min_pair_posterior) { return min_pair_posterior > 0.0f && min_pair_posterior <= 3.4028234663852886e38f; }

// dmx_em_doublets.  Facts::have_table: the PRIOR BETAS are set - the call's first step is a P-step.  The order is the order of the
// refusals: the loop's own arguments, then the context and everything the pooled entries refuse of the pools (pools_plan.h: check).
inline Verdict check_em(const Facts &f, const Pools &p, int n_iterations, float power, float min_pair_posterior)
{
    if (n_iterations < 1) return {INVALID, "n_iterations must be >= 1", -1};
    if (!power_valid(power)) return {INVALID, "the contribution power must be finite and above 0", -1};
    if (!threshold_valid(min_pair_posterior)) return {INVALID, "min_pair_posterior must be finite and above 0", -1};
    return asplan::check_context_and_pools(f, p);
}

// dmx_mstep_doublets.  Facts::have_table: the table of the last P-step (or dmx_set_probs); have_post: the dense singlet posteriors of
// an E-step.  rows [n_rows]: the compact posterior rows of that E-step, as the caller holds them.
inline Verdict check_mstep(const Facts &f, bool have_post, const Pools &p, float power, float min_pair_posterior, long long n_rows, const float *rows)
{
    if (!f.have_problem) return {INVALID, "call order: a problem comes first", -1};
    if (!f.have_table) return {INVALID, "call order: genotype probabilities (dmx_probs_from_betas / dmx_set_probs) come first", -1};
    if (!have_post) return {INVALID, "call order: an E-step comes first", -1};
    if (!power_valid(power)) return {INVALID, "the contribution power must be finite and above 0", -1};
    if (!threshold_valid(min_pair_posterior)) return {INVALID, "min_pair_posterior must be finite and above 0", -1};
    const Verdict pools = asplan::check_context_and_pools(f, p);
    if (pools.status != OK) return pools;
    if (n_rows != p.row_ptr[f.B]) return {INVALID, "the posterior rows have another length than row_ptr[B]", -1};
    if (n_rows > 0 && !rows) return {INVALID, "null posterior rows", -1};
    for (long long k = 0; k < n_rows; k++)
        if (!aplan::unit_range(rows[k])) return {INVALID, "a posterior of the rows is not finite or outside [0, 1]", k};
    return {OK, "", -1};
}

// how many list entries the live pairs of all barcodes can take: the pair options of every pooled barcode (pools that check() accepted)
inline long long pair_options(long long B, const Pools &p)
{
    long long total = 0;
    for (long long b = 0; b < B; b++) {
        const long long q = p.pool_of_barcode[b];
        if (q < 0) continue;
        const long long g = p.pool_start[q + 1] - p.pool_start[q];
        total += pplan::options_of(g, p.with_doublets != 0) - g;
    }
    return total;
}

}  // namespace dlplan
}  // namespace dmx
