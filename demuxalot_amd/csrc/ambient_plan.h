// ambient_plan.h -- what dmx_ambient_profile (ambient_profile.hip) decides on the host, as pure functions of plain
// values: the validation of a call, the grid's zero column, whether a call count is exact in float32, and the exact division that
// turns a record's row offset into a table row.  Host only: nothing of HIP, nothing of dmx_ctx.  dmx_steps.cpp: dmx_ambient_profile
// asks check() before anything is uploaded or launched; ambient_profile.hip uses the same row division on the device;
// tests/ambient_plan_check.cpp walks all of it on the CPU.
#pragma once

namespace dmx {
namespace aplan __attribute__((visibility("hidden"))) {  // (inline functions a translation unit keeps out of line are no exports of the library)

constexpr int MAX_ALPHAS = 64;                   // one grid point per lane of a wavefront
constexpr int OK = 0, INVALID = -1, UNSUPPORTED = -5;  // DMX_OK, DMX_ERR_INVALID, DMX_ERR_UNSUPPORTED (dmx_steps.cpp asserts the values)
constexpr unsigned long long EXACT_COUNTS = 1ull << 24;  // c + 1 is a float32 for every call count c below this

struct Facts {
    bool have_problem;  // dmx_set_problem or a device pack
    bool have_table;    // dmx_probs_from_betas / dmx_set_probs
    bool attached;      // a communicator (dmx_comm_init*)
    int nranks;
    bool dense_table;   // the table's rows are the variants, in order (no padded exchange layout)
    long long B, V;
    int G;
};

struct Verdict {
    int status;        // OK, INVALID, UNSUPPORTED
    const char *what;  // static text
    long long at;      // index the text speaks of, or -1
};

// finite and in [0, 1] (NaN fails every comparison)
inline bool unit_range(float x) { return x >= 0.0f && x <= 1.0f; }

// donor1 / donor2 of one barcode as table columns (donor_readout.column_donors): (-1, any) skipped, (d, -1) a singlet, d1 < d2 a pair
inline bool donors_valid(int d1, int d2, int G)
{
    if (d1 == -1) return true;
    if (d1 < 0 || d1 >= G) return false;
    return d2 == -1 || (d2 > d1 && d2 < G);
}

inline Verdict check(const Facts &f, long long n_alphas, const float *alphas, const int *donor1, const int *donor2, const float *ambient)
{
    if (!f.have_problem || !f.have_table) return {INVALID, "call order: a problem and genotype probabilities (dmx_probs_from_betas / dmx_set_probs) come first", -1};
    if (f.attached || f.nranks > 1) return {UNSUPPORTED, "a context with a communicator attached is not supported", -1};
    if (!f.dense_table) return {UNSUPPORTED, "the genotype table is in a padded exchange layout", -1};
    if (n_alphas < 1) return {INVALID, "the grid needs at least one value", n_alphas};
    if (n_alphas > MAX_ALPHAS) return {UNSUPPORTED, "the grid has more than 64 values", n_alphas};
    if (!alphas) return {INVALID, "null alphas", -1};
    if (f.B > 0 && (!donor1 || !donor2)) return {INVALID, "null donor1 / donor2", -1};
    for (long long j = 0; j < n_alphas; j++)
        if (!unit_range(alphas[j])) return {INVALID, "a grid value is not finite or outside [0, 1]", j};
    for (long long b = 0; b < f.B; b++)
        if (!donors_valid(donor1[b], donor2[b], f.G)) return {INVALID, "donor1 / donor2 of a barcode are neither (-1, .), (d, -1) nor 0 <= d1 < d2 < G", b};
    if (ambient)
        for (long long v = 0; v < f.V; v++)
            if (!unit_range(ambient[v])) return {INVALID, "an ambient value is not finite or outside [0, 1]", v};
    return {OK, "", -1};
}

// the first grid point whose value is 0 (the reference's own term: q * 1 + a * 0 == q), or -1
inline int zero_column(int n_alphas, const float *alphas)
{
    for (int j = 0; j < n_alphas; j++)
        if (alphas[j] == 0.0f) return j;
    return -1;
}

// (constexpr, as row_of below: the two the device code calls as well)
constexpr bool count_is_exact(unsigned long long calls) { return calls < EXACT_COUNTS; }

// A call record holds the byte offset of its variant's row, row * row_bytes (kernels.h: CallPair::row_off).  For a multiple of
// d = odd * 2^shift the quotient is (offset >> shift) * odd^-1 modulo 2^32: a shift and a multiplication where the division
// by a run-time value takes a sequence of twenty instructions per call.
struct RowDivide {
    unsigned shift, inverse;
};
inline RowDivide row_divide(unsigned row_bytes)  // row_bytes > 0
{
    RowDivide d{0u, 1u};
    while (!(row_bytes & 1u)) row_bytes >>= 1, d.shift++;
    unsigned x = row_bytes;  // correct to 3 bits (odd * odd = 1 mod 8); every Newton step doubles them
    for (int i = 0; i < 5; i++) x *= 2u - row_bytes * x;
    d.inverse = x;
    return d;
}
constexpr unsigned row_of(unsigned row_off, unsigned shift, unsigned inverse) { return (row_off >> shift) * inverse; }

}  // namespace aplan
}  // namespace dmx
