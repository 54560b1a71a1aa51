// soup_learning_plan.h -- what dmx_mstep_soup and dmx_em_ambient_soup (mstep_soup.hip) refuse, as pure functions of
// plain values: the pseudo-count, and everything dmx_mstep_ambient and dmx_em_ambient refuse (ambient_learning_plan.h: the same
// check_mstep and check_em, with their codes and words).  Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp asks them
// before anything is uploaded or launched; tests/soup_learning_plan_check.cpp walks them on the CPU.
#pragma once
#include "ambient_learning_plan.h"

namespace dmx {
namespace slplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

using alplan::Facts;
using alplan::INVALID;
using alplan::OK;
using alplan::Pools;
using alplan::UNSUPPORTED;
using alplan::Verdict;

// the soup M-step's power: expected counts
constexpr float POWER = 1.0f;

// a pseudo-count every variant's total can take: finite and above 0 (NaN fails the comparison), so that no beta is 0
inline bool pseudo_count_valid(float pseudo_count) { return pseudo_count > 0.0f && pseudo_count <= 3.4028234663852886e38f; }

inline Verdict bad_pseudo_count() { return {INVALID, "the pseudo-count must be finite and above 0", -1}; }

// dmx_em_ambient_soup.  The order is the order of the refusals: the loop's own arguments - the iteration count, the power, the
// pseudo-count -, then everything dmx_em_ambient refuses behind its own two.
inline Verdict check_em(const Facts &f, const Pools &p, int n_iterations, float power, float pseudo_count, const float *alpha, const float *ambient)
{
    if (n_iterations >= 1 && alplan::power_valid(power) && !pseudo_count_valid(pseudo_count)) return bad_pseudo_count();
    return alplan::check_em(f, p, n_iterations, power, alpha, ambient);
}

// dmx_mstep_soup.  dmx_mstep_ambient's order with the pseudo-count where that has its power: the context first (what check_mstep
// says of a context without barcodes and without a supplied profile), then the pseudo-count, then EVERY barcode's fraction and the
// profile.
inline Verdict check_mstep(const Facts &f, bool have_post, float pseudo_count, const float *alpha, const float *ambient)
{
    Facts nobody = f;
    nobody.B = 0;
    const Verdict context = alplan::check_mstep(nobody, have_post, POWER, nullptr, nullptr);
    if (context.status != OK) return context;
    if (!pseudo_count_valid(pseudo_count)) return bad_pseudo_count();
    return alplan::check_mstep(f, have_post, POWER, alpha, ambient);
}

}  // namespace slplan
}  // namespace dmx
