// read_columns.h -- the columns of a dmx_decoded_reads as the read passes (count_reads.hip, coverage.hip, resident_reads.hip)
// hand them to kernels and fill them: the pointer structs beside dmx_ctx.h's ReadColumns (same member names, listed by
// each_read_column there), the adapter for the caller's struct, and what every pass asks of a read's ranges.
#pragma once
#include <climits>

#include "device_scratch.h"

namespace dmx {
namespace reads {

using namespace dmx::scratch;

// The reads as the kernels take them, by value: ReadsView.  A coverage pass leaves the counting-only columns null.
// The same shape over the caller's host arrays is a type of its own (HostReads), so that neither is taken for the other.
template <bool OnDevice>
struct ReadPointers : ReadCounts {
    const int *start, *cb, *ub, *score, *n_cigar, *l_seq;
    const double *p_misaligned;
    const long long *cigar_begin, *seq_begin;
    const unsigned *cigar;
    const unsigned char *seq, *qual;
};
typedef ReadPointers<true> ReadsView;
typedef ReadPointers<false> HostReads;

// device columns to be written: the destinations of uploads, copies and gathers
struct ReadsOut {
    int *start, *cb, *ub, *score, *n_cigar, *l_seq;
    double *p_misaligned;
    long long *cigar_begin, *seq_begin;
    unsigned *cigar;
    unsigned char *seq, *qual;
};

// the caller's struct under the common names (int64_t is long here, the kernels count in long long)
inline HostReads host_reads(const dmx_decoded_reads *h)
{
    HostReads r;
    r.n = h->n_reads, r.n_ops = h->n_cigar_ops, r.n_bases = h->n_bases;
    r.start = h->reference_start, r.cb = h->compressed_cb, r.ub = h->compressed_ub, r.p_misaligned = h->p_misaligned;
    r.score = h->alignment_score, r.cigar_begin = (const long long *)h->cigar_begin, r.n_cigar = h->n_cigar;
    r.seq_begin = (const long long *)h->seq_begin, r.l_seq = h->l_seq, r.cigar = h->cigar, r.seq = h->seq, r.qual = h->qual;
    return r;
}

// What every entry point refuses of host arrays before it uploads them.  A set that serves coverage only may come without
// the counting-only columns.
inline int check_reads(const dmx_decoded_reads *reads, const char *who, bool counting_optional)
{
    if (reads->n_reads < 0 || reads->n_reads > INT_MAX) return fail(DMX_ERR_INVALID, "%s: n_reads must be 0 .. 2^31 - 1", who);
    if (reads->n_cigar_ops < 0 || reads->n_bases < 0 || (reads->n_cigar_ops && !reads->cigar) || (reads->n_bases && (!reads->seq || !reads->qual)))
        return fail(DMX_ERR_INVALID, "%s: bad cigar / seq / qual arrays", who);
    const bool counting_missing = !reads->compressed_cb || !reads->compressed_ub || !reads->p_misaligned || !reads->alignment_score;
    if (reads->n_reads && ((counting_missing && !counting_optional) || !reads->reference_start || !reads->cigar_begin || !reads->n_cigar ||
                           !reads->seq_begin || !reads->l_seq))
        return fail(DMX_ERR_INVALID, "%s: null per-read array", who);
    return 0;
}

// held columns as destinations (those not held: null)
inline ReadsOut out_of(const ReadColumns &cols)
{
    ReadsOut out;
    (void)each_read_column([](ReadExtent, bool, auto &p, const auto &b) { return p = b.p, 0; }, out, cols);
    return out;
}

// `out` moved on by `by` elements of each extent.  Every column of `out` is held.
inline ReadsOut offset(ReadsOut out, const ReadCounts &by)
{
    (void)each_read_column([&](ReadExtent e, bool, auto &p) { return p += by.of(e), 0; }, out);
    return out;
}

// the columns just written, to be read
inline ReadsView view_of(const ReadsOut &out, const ReadCounts &counts)
{
    ReadsView R;
    static_cast<ReadCounts &>(R) = counts;
    (void)each_read_column([](ReadExtent, bool, auto &v, auto *p) { return v = p, 0; }, R, out);
    return R;
}

// Reads [first, first + n) of held columns: the per-read columns move, cigar / seq / qual stay whole (cigar_begin / seq_begin
// count from the set's own arrays).  The counting-only columns are taken where asked for and held, and are null otherwise:
// no pointer is formed from a buffer that is not there.
inline ReadsView view_of(const ReadColumns &cols, long long first, long long n, bool with_counting)
{
    ReadsView R;
    R.n = n, R.n_ops = cols.n_ops, R.n_bases = cols.n_bases;
    (void)each_read_column(
        [&](ReadExtent e, bool counting, auto &v, const auto &b) {
            v = !b.p || (counting && !with_counting) ? nullptr : b.p + (e == PER_READ ? first : 0);
            return 0;
        },
        R, cols);
    return R;
}

// host arrays into device columns of as many elements: the counting-only columns only where asked for
inline int copy_in(const ReadsOut &out, const HostReads &h, bool with_counting, hipStream_t st)
{
    return each_read_column(
        [&](ReadExtent e, bool counting, auto *to, auto *from) {
            if (h.of(e) && (with_counting || !counting)) HIP_TRY(hipMemcpyAsync(to, from, h.of(e) * sizeof(*to), hipMemcpyHostToDevice, st));
            return 0;
        },
        out, h);
}

// host arrays into temporaries of the call; *R views them
inline int upload_reads(Scratch &sc, const HostReads &h, bool with_counting, ReadsView *R, hipStream_t st)
{
    ReadsOut out = {};
    DMX_TRY(each_read_column([&](ReadExtent e, bool counting, auto &p) { return counting && !with_counting ? 0 : sc.get(&p, h.of(e)); }, out));
    DMX_TRY(copy_in(out, h, with_counting, st));
    *R = view_of(out, h);
    return 0;
}

// does [begin, begin + length) leave an array of `total` elements: asked of a read's cigar range and of its seq range
__device__ __forceinline__ bool outside(long long begin, long long length, long long total)
{
    return length < 0 || begin < 0 || begin > total || length > total - begin;
}

}  // namespace reads
}  // namespace dmx
