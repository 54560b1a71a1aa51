// pair_shares_plan.h -- what dmx_estep_pair_shares (estep_pair_shares.hip) refuses, as one pure function of plain
// values.  The contexts the pass does not run on and everything dmx_estep_pools refuses of the pools are not restated: they are
// ambient_scoring_plan.h's check_context_and_pools (the same pplan::check inside), with its words.  What this header adds is the grid
// of mixing shares and the prior over it: at least one share, every share finite and in [0, 1], any order, duplicates allowed; the log
// weights absent (all 0) or n_shares finite values; at most 64 shares.  Host only: nothing of HIP, nothing of dmx_ctx.
// dmx_steps.cpp: dmx_estep_pair_shares asks check() before anything is uploaded or launched; tests/pair_shares_plan_check.cpp walks
// it on the CPU.
#pragma once
#include "ambient_scoring_plan.h"

namespace dmx {
namespace psplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using aplan::Facts;
using pplan::INVALID;
using pplan::OK;
using pplan::UNSUPPORTED;
using pplan::Pools;
using pplan::Verdict;

constexpr int MAX_SHARES = 64;

// The order is the order of the refusals: the context, the pools as dmx_estep_pools walks them, then what is invalid of the grid -
// its length, the shares, the weights, each value with its index - and last the length that is valid but not supported.  (A grid of
// more than 64 values is therefore read in full first: the caller says it has that many.)
inline Verdict check(const Facts &f, const Pools &p, long long n_shares, const float *shares, const float *log_weights)
{
    const Verdict pools = asplan::check_context_and_pools(f, p);
    if (pools.status != OK) return pools;
    if (n_shares < 1) return {INVALID, "the grid of shares needs at least one value", n_shares};
    if (!shares) return {INVALID, "null shares", -1};
    for (long long j = 0; j < n_shares; j++)
        if (!aplan::unit_range(shares[j])) return {INVALID, "a share is not finite or outside [0, 1]", j};
    const long long j = log_weights ? asplan::first_log_weight_not_finite(log_weights, n_shares) : -1;
    if (j >= 0) return {INVALID, "a log weight is not finite", j};
    static_assert(MAX_SHARES == 64, "the text below spells the limit out");
    if (n_shares > MAX_SHARES) return {UNSUPPORTED, "the grid of shares has more than 64 values", n_shares};
    return {OK, "", -1};
}

}  // namespace psplan
}  // namespace dmx
