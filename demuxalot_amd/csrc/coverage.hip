// coverage.hip -- candidate SNP positions from decoded reads: stage 1 of the reference's detect_snps_for_chromosome
// (demuxalot/snp_detection.py:32-57; include/demux_hip.h "Coverage"; the contract: DESIGN.md "Coverage and candidates").
//
//   1 walk        one lane per read: CIGAR -> reference_end, error bits
//   2 window      reads are sorted by start, so the prefix maximum of reference_end is monotone: the reads that can reach
//                 [lo, hi) are those from the first one whose prefix maximum is above lo up to the first one that starts at
//                 hi or later (two binary searches; the trick of the "molecules" stage of count_reads.hip)
//   3 accumulate  one wavefront per read, one lane per aligned base of the operation at hand: counts[base][position] += 1.
//                 Two forms with identical output (the counts are integers):
//                   atomic  no-return global atomics straight into the dense window
//                   tiled   a workgroup owns TILE positions whose 4 x TILE counters sit in LDS, adds with LDS atomics over the
//                           reads that reach the tile and stores the tile once; a tile that more than CHUNK reads reach is
//                           split over several workgroups that flush their non-zero counters with global atomics
//   4 filter      one lane per position: total, ref, alt, the four comparisons in float64; scan + compaction
//   5 top-n       only when more positions qualify than the cap: stable sort by alt, the tail, sorted back by position
//
// The aligned pairs are pysam's (count_coverage): H and P move NEITHER cursor.  count_reads.hip differs on purpose: it
// repeats the reference's own walker (snp_counter.py), which moves the read cursor on H and P.
// Nothing traps: malformed input sets a flag word the host reads before anything is accumulated.  The state (the counts of
// the last window, its candidates) lives in dmx_ctx::d_cov_*, which nothing else touches; dmx_release_problem and dmx_destroy
// free it.
#include <climits>
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device_scratch.h"
#include "dmx_host.h"
#include "read_columns.h"

namespace {

using dmx::host::bind;
using namespace dmx::scratch;
using namespace dmx::reads;

constexpr int WAVE = 64, BLOCK = 256, WAVES = BLOCK / WAVE;
constexpr int READS_PER_WAVE = 4;  // atomic form: consecutive reads one wavefront takes
constexpr int TILE = 2048;         // tiled form: positions per tile (4 x TILE x 4 bytes = 32 KB of LDS)
constexpr int CHUNK = 1024;        // tiled form: reads one workgroup takes of a tile at most
// flag word
constexpr int F_UNSORTED = 1, F_LAYOUT = 2, F_OP = 4, F_INDEX = 8;

typedef StageClock<dmx::COVERAGE_STAGES> Clock;

__device__ __forceinline__ ull biased(int v) { return (ull)((unsigned)v ^ 0x80000000u); }

// Stage 1.  Everything the later stages rely on is checked here, for every read of the input whatever the window: they run
// only when no flag was raised, and then no index they form lies outside cigar / seq.
__global__ __launch_bounds__(256) void k_cov_walk(ReadsView R, int *__restrict__ end, ull *__restrict__ reach_in, int *flags)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n) return;
    const long long start = R.start[i];
    if (i > 0 && start < R.start[i - 1]) atomicOr(flags, F_UNSORTED);
    long long c0 = R.cigar_begin[i], nc = R.n_cigar[i];
    const long long s0 = R.seq_begin[i], ls = R.l_seq[i];
    if (outside(c0, nc, R.n_ops) || outside(s0, ls, R.n_bases)) {
        atomicOr(flags, F_LAYOUT);
        nc = 0;
    }
    long long ref = start, rd = 0;
    unsigned e = 0;
    for (long long k = 0; k < nc; k++) {
        const unsigned c = R.cigar[c0 + k];
        const unsigned op = c & 15u;
        const long long len = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            if (rd + len > ls) e |= F_INDEX;  // a pair (q, r) with q >= l_seq
            ref += len;
            rd += len;
        } else if (op == 2 || op == 3) {
            ref += len;
        } else if (op == 1 || op == 4) {
            rd += len;
        } else if (op > 8) {
            e |= F_OP;
        }  // 5 (H), 6 (P): neither cursor moves
    }
    if (ref > INT_MAX) {
        e |= F_LAYOUT;
        ref = INT_MAX;
    }
    if (e) atomicOr(flags, (int)e);
    end[i] = (int)ref;
    reach_in[i] = biased((int)ref);
}

// first read whose prefix maximum of reference_end is above x (biased values, non-decreasing)
__device__ __forceinline__ long long first_reaching(const ull *__restrict__ reach, long long n, long long x)
{
    const ull bx = biased((int)x);
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (reach[mid] > bx)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// first read that starts at x or later
__device__ __forceinline__ long long first_starting(const int *__restrict__ start, long long n, long long x)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (start[mid] >= x)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// Stage 2.  Tile t covers [w_lo + t * width, min(.. + width, w_hi)): its reads [first, last) and the workgroups it takes.
__global__ __launch_bounds__(256) void k_cov_tiles(const ull *__restrict__ reach, const int *__restrict__ start, long long n, long long w_lo,
                                                   long long w_hi, long long width, long long n_tiles, long long chunk,
                                                   long long *__restrict__ first, long long *__restrict__ last, ull *__restrict__ groups)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const long long lo = w_lo + t * width, hi = lo + width < w_hi ? lo + width : w_hi;
    const long long a = first_reaching(reach, n, lo);
    long long b = first_starting(start, n, hi);
    if (b < a) b = a;
    first[t] = a;
    last[t] = b;
    groups[t] = (ull)((b - a + chunk - 1) / chunk);
}

// Stage 3: the aligned bases of read i inside [lo, hi), one lane per base of an operation; dst[code * stride + (r - lo)] += 1.
// All lanes of the wavefront hold the same i.  LDS or global counters: the same atomic add, never returning.
__device__ __forceinline__ void add_read(const ReadsView &R, long long i, int lane, long long lo, long long hi, int *dst, long long stride,
                                         unsigned quality_threshold)
{
    const long long c0 = R.cigar_begin[i], nc = R.n_cigar[i], s0 = R.seq_begin[i];
    long long ref = R.start[i], rd = 0;
    for (long long k = 0; k < nc && ref < hi; k++) {
        const unsigned c = R.cigar[c0 + k];
        const unsigned op = c & 15u;
        const long long len = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            const long long a = ref > lo ? ref : lo, b = ref + len < hi ? ref + len : hi;
            for (long long r = a + lane; r < b; r += WAVE) {
                const long long q = s0 + rd + (r - ref);
                const unsigned char letter = R.seq[q];
                const int code = letter == 'A' ? 0 : letter == 'C' ? 1 : letter == 'G' ? 2 : letter == 'T' ? 3 : -1;
                if (code >= 0 && R.qual[q] >= quality_threshold) atomicAdd(&dst[code * stride + (r - lo)], 1);
            }
            ref += len;
            rd += len;
        } else if (op == 2 || op == 3) {
            ref += len;
        } else if (op == 1 || op == 4) {
            rd += len;
        }
    }
}

// the reads of [first, last) that end beyond lo, 64 at a time: one lane looks at one read's end, the wavefront then takes
// the reads that passed one after the other (a read far before the tile is inside the prefix-maximum bound when an earlier
// read with a long N skip reaches over it)
__device__ __forceinline__ void add_reads(const ReadsView &R, const int *__restrict__ end, long long first, long long last, long long step, int lane,
                                          long long lo, long long hi, int *dst, long long stride, unsigned quality_threshold)
{
    for (long long base = first; base < last; base += step) {
        const long long mine = base + lane;
        ull mask = __ballot(mine < last && end[mine] > lo);
        while (mask) {
            const int bit = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            add_read(R, base + bit, lane, lo, hi, dst, stride, quality_threshold);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_cov_atomic(ReadsView R, const int *__restrict__ end, long long first, long long last, long long w_lo,
                                                      long long w_hi, int *__restrict__ counts, unsigned quality_threshold)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long r0 = first + ((long long)blockIdx.x * WAVES + wave) * READS_PER_WAVE;
    const long long r1 = r0 + READS_PER_WAVE < last ? r0 + READS_PER_WAVE : last;
    if (r0 < r1) add_reads(R, end, r0, r1, WAVE, lane, w_lo, w_hi, counts, w_hi - w_lo, quality_threshold);
}

// workgroup g takes chunk (g - groups before its tile) of the tile whose inclusive group count is the first above g
__global__ __launch_bounds__(BLOCK) void k_cov_tiled(ReadsView R, const int *__restrict__ end, const long long *__restrict__ first,
                                                     const long long *__restrict__ last, const ull *__restrict__ groups_at, long long n_tiles,
                                                     long long w_lo, long long w_hi, int *__restrict__ counts, unsigned quality_threshold)
{
    __shared__ int tile[4 * TILE];
    const ull g = blockIdx.x;
    long long a = 0, b = n_tiles;
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (groups_at[mid] > g)
            b = mid;
        else
            a = mid + 1;
    }
    const long long t = a;
    if (t >= n_tiles) return;
    const ull before = t ? groups_at[t - 1] : 0ull;
    const bool alone = groups_at[t] - before == 1;
    const long long lo = w_lo + t * TILE, hi = lo + TILE < w_hi ? lo + TILE : w_hi, width = hi - lo, W = w_hi - w_lo;
    const long long r0 = first[t] + (long long)(g - before) * CHUNK, r1 = r0 + CHUNK < last[t] ? r0 + CHUNK : last[t];
    for (int k = threadIdx.x; k < 4 * TILE; k += BLOCK) tile[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    add_reads(R, end, r0 + (long long)wave * WAVE, r1, (long long)WAVES * WAVE, lane, lo, hi, tile, TILE, quality_threshold);
    __syncthreads();
    int *out = counts + (lo - w_lo);
    for (int code = 0; code < 4; code++)
        for (long long k = threadIdx.x; k < width; k += BLOCK) {
            const int v = tile[code * TILE + k];
            if (alone)
                out[code * W + k] = v;  // (tiles no read reaches keep the zeros the window was cleared to)
            else if (v)
                atomicAdd(&out[code * W + k], v);
        }
}

// Stage 4 (snp_detection.py:44-50).  Integers below 2^53 are exact in float64, so every comparison is; the two products are
// rounded once (the library is built with -ffp-contract=off).
__global__ __launch_bounds__(256) void k_cov_filter(const int *__restrict__ counts, long long W, double minimum_coverage,
                                                    double minimum_alternative_fraction, double minimum_alternative_coverage,
                                                    double minimum_fraction_of_ref_and_alt, ull *__restrict__ is_candidate,
                                                    unsigned *__restrict__ alt_of)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W) return;
    long long total = 0, ref = -1, alt = -1;  // the largest and the second largest of the four, as values
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const long long v = counts[b * W + p];
        total += v;
        if (v > ref) {
            alt = ref;
            ref = v;
        } else if (v > alt) {
            alt = v;
        }
    }
    const double both = (double)(ref + alt);
    bool ok = both > minimum_coverage;
    ok = ok && both > minimum_fraction_of_ref_and_alt * (double)total;
    ok = ok && (double)alt > minimum_alternative_coverage;
    ok = ok && (double)alt > (double)ref * minimum_alternative_fraction;
    is_candidate[p] = ok ? 1ull : 0ull;
    alt_of[p] = (unsigned)alt;
}

__global__ __launch_bounds__(256) void k_cov_compact(const ull *__restrict__ is_candidate, const ull *__restrict__ at, const unsigned *__restrict__ alt_of,
                                                     long long W, unsigned *__restrict__ index, unsigned *__restrict__ alt)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W || !is_candidate[p]) return;
    index[at[p] - 1] = (unsigned)p;
    alt[at[p] - 1] = alt_of[p];
}

__global__ __launch_bounds__(256) void k_cov_emit(const unsigned *__restrict__ index, long long n, const int *__restrict__ counts, long long W,
                                                  long long w_lo, int *__restrict__ positions, int *__restrict__ cand_counts)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long p = index[j];
    positions[j] = (int)(w_lo + p);
#pragma unroll
    for (int b = 0; b < 4; b++) cand_counts[j * 4 + b] = counts[b * W + p];
}

int flag_error(int flags)
{
    if (flags & F_LAYOUT) return fail(DMX_ERR_INVALID, "coverage: a read's cigar / seq range lies outside the arrays, or its reference_end is beyond 2^31");
    if (flags & F_UNSORTED) return fail(DMX_ERR_INVALID, "coverage: reference_start must be non-decreasing in read order");
    if (flags & F_OP) return fail(DMX_ERR_INVALID, "coverage: unknown CIGAR operation (codes 0 .. 8 are known)");
    if (flags & F_INDEX) return fail(DMX_ERR_INVALID, "coverage: an aligned base lies beyond l_seq");
    return 0;
}

// Stages 1 to 3 on the reads R (device arrays the caller placed: uploaded into sc, or a resident set's own), after the
// "upload" stage, which also clears the window.
int coverage_window(dmx_ctx *c, Scratch &sc, Clock &clock, const ReadsView &R, long long w_lo, long long w_hi, unsigned quality_threshold)
{
    hipStream_t st = c->stream;
    const long long n = R.n, W = w_hi - w_lo;
    const int *d_start = R.start;
    int *flags;
    DMX_TRY(sc.get(&flags, 1));
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int), st));
    DMX_TRY(dev_alloc(c, c->d_cov_counts, (size_t)(4 * W)));
    HIP_TRY(hipMemsetAsync(c->d_cov_counts.p, 0, dev_bytes(c->d_cov_counts), st));
    DMX_TRY(clock.tick(st));

    // ---- 1 walk
    int *end;
    ull *reach_in, *reach, top = 0;
    DMX_TRY(sc.get(&end, (size_t)n));
    DMX_TRY(sc.get(&reach_in, (size_t)n));
    DMX_TRY(sc.get(&reach, (size_t)n));
    if (n) hipLaunchKernelGGL(k_cov_walk, dim3(grid_for(n)), dim3(256), 0, st, R, end, reach_in, flags);
    DMX_TRY(launched("k_cov_walk"));
    DMX_TRY(inclusive_scan_total(sc, reach_in, reach, (size_t)n, &top, rocprim::maximum<ull>(), st));
    int h_flags = 0;
    HIP_TRY(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's arrays are free to change from here on)
    DMX_TRY(flag_error(h_flags));
    DMX_TRY(clock.tick(st));

    // ---- 2 window: one tile of the window's width (atomic form) or tiles of TILE positions
    const bool tiled = c->coverage_form == DMX_COVERAGE_TILED;
    const long long width = tiled ? TILE : (W ? W : 1), n_tiles = (W + width - 1) / width;
    long long *first, *last;
    ull *groups, *groups_at, n_groups = 0;
    DMX_TRY(sc.get(&first, (size_t)n_tiles));
    DMX_TRY(sc.get(&last, (size_t)n_tiles));
    DMX_TRY(sc.get(&groups, (size_t)n_tiles));
    DMX_TRY(sc.get(&groups_at, (size_t)n_tiles));
    if (n && n_tiles) {
        hipLaunchKernelGGL(k_cov_tiles, dim3(grid_for(n_tiles)), dim3(256), 0, st, reach, d_start, n, w_lo, w_hi, width, n_tiles,
                           (long long)CHUNK, first, last, groups);
        DMX_TRY(launched("k_cov_tiles"));
        DMX_TRY(sum_scan(sc, groups, groups_at, (size_t)n_tiles, &n_groups, st));
    }
    long long window[2] = {0, 0};  // atomic form: the reads of the one tile
    if (!tiled && n_groups) {
        HIP_TRY(hipMemcpyAsync(&window[0], first, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&window[1], last, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    DMX_TRY(clock.tick(st));

    // ---- 3 accumulate
    if (n_groups > 0x7FFFFFFFull) return fail(DMX_ERR_UNSUPPORTED, "coverage: %llu workgroups in one call: count a smaller window", n_groups);
    if (tiled && n_groups) {
        hipLaunchKernelGGL(k_cov_tiled, dim3((unsigned)n_groups), dim3(BLOCK), 0, st, R, end, first, last, groups_at, n_tiles, w_lo, w_hi,
                           c->d_cov_counts.p, quality_threshold);
        DMX_TRY(launched("k_cov_tiled"));
    } else if (window[1] > window[0]) {
        const long long per_block = (long long)WAVES * READS_PER_WAVE, blocks = (window[1] - window[0] + per_block - 1) / per_block;
        hipLaunchKernelGGL(k_cov_atomic, dim3((unsigned)blocks), dim3(BLOCK), 0, st, R, end, window[0], window[1], w_lo, w_hi, c->d_cov_counts.p,
                           quality_threshold);
        DMX_TRY(launched("k_cov_atomic"));
    }
    DMX_TRY(clock.tick(st));
    HIP_TRY(hipStreamSynchronize(st));
    for (double &ms : c->cov_stage_ms) ms = 0.0;
    DMX_TRY(clock.read(c->cov_stage_ms, 0));
    return 0;
}

int coverage_count(dmx_ctx *c, const dmx_decoded_reads *h, long long w_lo, long long w_hi, unsigned quality_threshold)
{
    hipStream_t st = c->stream;
    Scratch sc(c);
    Clock clock;
    DMX_TRY(clock.tick(st));

    // ---- upload (the counting-only columns are not read)
    ReadsView R;
    DMX_TRY(upload_reads(sc, host_reads(h), false, &R, st));
    c->reads_upload_bytes += dmx::host::decoded_reads_bytes(h->n_reads, h->n_cigar_ops, h->n_bases, false);
    return coverage_window(c, sc, clock, R, w_lo, w_hi, quality_threshold);
}

// dmx_coverage_count on a resident set: the stages read the set's buffers in place
int coverage_count_resident(dmx_ctx *c, const ResidentReads &set, long long w_lo, long long w_hi, unsigned quality_threshold)
{
    Scratch sc(c);
    Clock clock;
    DMX_TRY(clock.tick(c->stream));
    return coverage_window(c, sc, clock, view_of(set.columns, 0, set.columns.n, false), w_lo, w_hi, quality_threshold);
}

// what both entry points do around the pass: the previous window goes, a failed pass leaves none
template <typename Pass>
int count_window(dmx_ctx *c, int32_t start, int32_t stop, int32_t *coverage_out, Pass pass)
{
    dmx::host::release_coverage(c);
    const int rc = pass();
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_coverage(c);
        return rc;
    }
    c->cov_W = (long long)stop - start;
    c->cov_start = start;
    if (coverage_out && c->cov_W) {
        HIP_TRY(hipMemcpyAsync(coverage_out, c->d_cov_counts.p, (size_t)c->cov_W * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int coverage_candidates(dmx_ctx *c, double minimum_coverage, double minimum_alternative_fraction, double minimum_alternative_coverage,
                        double minimum_fraction_of_ref_and_alt, long long cap, long long *n_out)
{
    hipStream_t st = c->stream;
    const long long W = c->cov_W;
    Scratch sc(c);
    Clock clock;
    DMX_TRY(clock.tick(st));

    // ---- 4 filter
    ull *is_candidate, *at, n_candidates = 0;
    unsigned *alt_of, *index, *alt;
    DMX_TRY(sc.get(&is_candidate, (size_t)W));
    DMX_TRY(sc.get(&at, (size_t)W));
    DMX_TRY(sc.get(&alt_of, (size_t)W));
    if (W) hipLaunchKernelGGL(k_cov_filter, dim3(grid_for(W)), dim3(256), 0, st, c->d_cov_counts.p, W, minimum_coverage, minimum_alternative_fraction,
                              minimum_alternative_coverage, minimum_fraction_of_ref_and_alt, is_candidate, alt_of);
    DMX_TRY(launched("k_cov_filter"));
    DMX_TRY(sum_scan(sc, is_candidate, at, (size_t)W, &n_candidates, st));
    DMX_TRY(sc.get(&index, (size_t)n_candidates));
    DMX_TRY(sc.get(&alt, (size_t)n_candidates));
    if (n_candidates) hipLaunchKernelGGL(k_cov_compact, dim3(grid_for(W)), dim3(256), 0, st, is_candidate, at, alt_of, W, index, alt);
    DMX_TRY(launched("k_cov_compact"));
    DMX_TRY(clock.tick(st));

    // ---- 5 top-n: the tail of a stable ascending sort by alt (a tie at the cut goes to the higher position), by position again
    long long kept = (long long)n_candidates;
    const unsigned *kept_index = index;
    if (kept > cap) {
        unsigned *alt_sorted, *by_alt, *by_position, *unused;
        DMX_TRY(sc.get(&alt_sorted, (size_t)n_candidates));
        DMX_TRY(sc.get(&by_alt, (size_t)n_candidates));
        DMX_TRY(sc.get(&by_position, (size_t)cap));
        DMX_TRY(sc.get(&unused, (size_t)cap));
        DMX_TRY(sort_pairs(sc, alt, alt_sorted, index, by_alt, (size_t)n_candidates, 32u, st));
        const unsigned *tail = by_alt + (n_candidates - (ull)cap);
        DMX_TRY(sort_pairs(sc, tail, by_position, tail, unused, (size_t)cap, (unsigned)bits_for((ull)W), st));
        kept = cap;
        kept_index = by_position;
    }
    DMX_TRY(dev_alloc(c, c->d_cov_cand_pos, (size_t)kept));
    DMX_TRY(dev_alloc(c, c->d_cov_cand_counts, (size_t)kept * 4));
    if (kept) hipLaunchKernelGGL(k_cov_emit, dim3(grid_for(kept)), dim3(256), 0, st, kept_index, kept, c->d_cov_counts.p, W, c->cov_start,
                                 c->d_cov_cand_pos.p, c->d_cov_cand_counts.p);
    DMX_TRY(launched("k_cov_emit"));
    DMX_TRY(clock.tick(st));
    HIP_TRY(hipStreamSynchronize(st));
    DMX_TRY(clock.read(c->cov_stage_ms, dmx::COVERAGE_STAGES - 2));
    *n_out = kept;
    return 0;
}

}  // namespace

extern "C" {

int dmx_coverage_count(dmx_ctx *c, const dmx_decoded_reads *reads, int32_t start, int32_t stop, int32_t quality_threshold, int32_t *coverage_out)
{
    DMX_TRY(bind(c));
    if (!reads) return fail(DMX_ERR_INVALID, "coverage: null argument");
    if (reads->n_reads < 0 || reads->n_reads > INT_MAX) return fail(DMX_ERR_INVALID, "coverage: n_reads must be 0 .. 2^31 - 1");
    if (start < 0 || stop < start) return fail(DMX_ERR_INVALID, "coverage: the window must satisfy 0 <= start <= stop");
    if (quality_threshold < 0 || quality_threshold > 255) return fail(DMX_ERR_INVALID, "coverage: quality_threshold must be 0 .. 255");
    if (reads->n_cigar_ops < 0 || reads->n_bases < 0 || (reads->n_cigar_ops && !reads->cigar) || (reads->n_bases && (!reads->seq || !reads->qual)))
        return fail(DMX_ERR_INVALID, "coverage: bad cigar / seq / qual arrays");
    if (reads->n_reads && (!reads->reference_start || !reads->cigar_begin || !reads->n_cigar || !reads->seq_begin || !reads->l_seq))
        return fail(DMX_ERR_INVALID, "coverage: null per-read array");
    return count_window(c, start, stop, coverage_out, [&] { return coverage_count(c, reads, start, stop, (unsigned)quality_threshold); });
}

int dmx_coverage_count_resident(dmx_ctx *c, int64_t handle, int32_t start, int32_t stop, int32_t quality_threshold, int32_t *coverage_out)
{
    DMX_TRY(bind(c));
    if (start < 0 || stop < start) return fail(DMX_ERR_INVALID, "coverage: the window must satisfy 0 <= start <= stop");
    if (quality_threshold < 0 || quality_threshold > 255) return fail(DMX_ERR_INVALID, "coverage: quality_threshold must be 0 .. 255");
    ResidentReads *set = nullptr;
    DMX_TRY(dmx::host::find_resident_reads(c, handle, "coverage_count_resident", &set));
    return count_window(c, start, stop, coverage_out, [&] { return coverage_count_resident(c, *set, start, stop, (unsigned)quality_threshold); });
}

int dmx_coverage_candidates(dmx_ctx *c, double minimum_coverage, double minimum_alternative_fraction, double minimum_alternative_coverage,
                            double minimum_fraction_of_ref_and_alt, int64_t max_snp_candidates, int64_t *n_candidates)
{
    DMX_TRY(bind(c));
    if (!n_candidates) return fail(DMX_ERR_INVALID, "coverage_candidates: null n_candidates");
    *n_candidates = 0;
    if (c->cov_W < 0) return fail(DMX_ERR_INVALID, "call order: dmx_coverage_count before dmx_coverage_candidates");
    if (!std::isfinite(minimum_coverage) || !std::isfinite(minimum_alternative_fraction) || !std::isfinite(minimum_alternative_coverage) ||
        !std::isfinite(minimum_fraction_of_ref_and_alt))
        return fail(DMX_ERR_INVALID, "coverage_candidates: the thresholds must be finite");
    if (minimum_coverage < 0 || minimum_alternative_coverage < 0)
        return fail(DMX_ERR_INVALID, "coverage_candidates: minimum_coverage and minimum_alternative_coverage must be >= 0");
    if (max_snp_candidates < 1) return fail(DMX_ERR_INVALID, "coverage_candidates: max_snp_candidates must be >= 1");
    dev_free(c, c->d_cov_cand_pos);
    dev_free(c, c->d_cov_cand_counts);
    c->cov_candidates = -1;
    long long n = 0;
    const int rc = coverage_candidates(c, minimum_coverage, minimum_alternative_fraction, minimum_alternative_coverage,
                                       minimum_fraction_of_ref_and_alt, max_snp_candidates, &n);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(c, c->d_cov_cand_pos);
        dev_free(c, c->d_cov_cand_counts);
        return rc;
    }
    c->cov_candidates = n;
    *n_candidates = n;
    return 0;
}

int dmx_coverage_fetch_candidates(dmx_ctx *c, int32_t *positions_out, int32_t *counts_out)
{
    DMX_TRY(bind(c));
    if (c->cov_candidates < 0) return fail(DMX_ERR_INVALID, "call order: dmx_coverage_candidates before dmx_coverage_fetch_candidates");
    if (c->cov_candidates && !positions_out) return fail(DMX_ERR_INVALID, "coverage_fetch_candidates: null positions_out");
    if (c->cov_candidates) {
        const size_t n = (size_t)c->cov_candidates;
        HIP_TRY(hipMemcpyAsync(positions_out, c->d_cov_cand_pos.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, c->d_cov_cand_counts.p, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int dmx_set_coverage_form(dmx_ctx *c, int form)
{
    DMX_TRY(bind(c));
    if (form != DMX_COVERAGE_ATOMIC && form != DMX_COVERAGE_TILED) return fail(DMX_ERR_INVALID, "coverage form must be DMX_COVERAGE_ATOMIC or DMX_COVERAGE_TILED");
    c->coverage_form = form;
    return 0;
}

int dmx_get_coverage_timings(dmx_ctx *c, double *stage_ms)
{
    DMX_TRY(bind(c));
    if (!stage_ms) return fail(DMX_ERR_INVALID, "null stage_ms");
    if (c->cov_W < 0) return fail(DMX_ERR_INVALID, "call order: dmx_coverage_count before dmx_get_coverage_timings");
    for (int s = 0; s < dmx::COVERAGE_STAGES; s++) stage_ms[s] = c->cov_stage_ms[s];
    return 0;
}

}  // extern "C"
