// doublet_shares_learning_plan.h -- what dmx_em_doublet_shares, dmx_estep_pair_shares_resident and dmx_mstep_doublet_shares
// (estep_pair_shares.hip, mstep_doublet_shares.hip) refuse, as pure functions of plain values.  Nothing is restated:
// the grid of shares and the prior over it are pair_shares_plan.h's check, the loop's and the M-step's own arguments
// doublet_learning_plan.h's check_em / check_mstep, in that order and with their words.  What this header adds is the caller's
// share rows of the stateless M-step: present, and every PAIR entry finite and in [0, 1] - a singlet's entry (NaN, as the E-step
// leaves it) is not read.  Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp asks these before anything is uploaded or
// launched; tests/doublet_shares_learning_plan_check.cpp walks them on the CPU.
#pragma once
#include "doublet_learning_plan.h"
#include "pair_shares_plan.h"

namespace dmx {
namespace dslplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using dlplan::pair_options;
using pplan::INVALID;
using pplan::OK;
using pplan::UNSUPPORTED;
using pplan::Pools;
using pplan::Verdict;
using aplan::Facts;

// dmx_estep_pair_shares_resident: dmx_estep_pair_shares' refusals (the resident entries' contexts are the same: no communicator)
inline Verdict check_estep(const Facts &f, const Pools &p, long long n_shares, const float *shares, const float *log_weights)
{
    return psplan::check(f, p, n_shares, shares, log_weights);
}

// dmx_em_doublet_shares.  Facts::have_table: the PRIOR BETAS are set - the call's first step is a P-step.  The context, the pools and
// the grid first (pair_shares_plan.h), then the loop's own arguments (doublet_learning_plan.h, which finds the pools accepted).
inline Verdict check_em(const Facts &f, const Pools &p, long long n_shares, const float *shares, const float *log_weights, int n_iterations,
                        float power, float min_pair_posterior)
{
    const Verdict grid = psplan::check(f, p, n_shares, shares, log_weights);
    if (grid.status != OK) return grid;
    return dlplan::check_em(f, p, n_iterations, power, min_pair_posterior);
}

// dmx_mstep_doublet_shares: dmx_mstep_doublets' refusals, then the share rows [n_rows] beside the posterior rows
inline Verdict check_mstep(const Facts &f, bool have_post, const Pools &p, float power, float min_pair_posterior, long long n_rows,
                           const float *post_rows, const float *share_rows)
{
    const Verdict credited = dlplan::check_mstep(f, have_post, p, power, min_pair_posterior, n_rows, post_rows);
    if (credited.status != OK) return credited;
    if (!share_rows) return {INVALID, "null share rows", -1};  // (also with no rows: the caller always holds the array, empty or not)
    for (long long b = 0; b < f.B; b++) {
        const long long q = p.pool_of_barcode[b];
        if (q < 0) continue;
        const long long singlets = p.pool_start[q + 1] - p.pool_start[q];
        for (long long k = p.row_ptr[b] + singlets; k < p.row_ptr[b + 1]; k++)
            if (!aplan::unit_range(share_rows[k])) return {INVALID, "a pair's share of the rows is not finite or outside [0, 1]", k};
    }
    return {OK, "", -1};
}

}  // namespace dslplan
}  // namespace dmx
