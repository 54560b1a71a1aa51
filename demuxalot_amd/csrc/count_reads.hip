// count_reads.hip -- SNP call containers from decoded reads: the compute half of the reference's count_snps
// (demuxalot/snp_counter.py:37-69, 142-276; include/demux_hip.h "Read counting"; the contract: DESIGN.md "Read counting").
//
//   1 walk     one lane per read: CIGAR -> reference_end, number of observations (binary search over the positions),
//              error bits, event flag; the events (reads that enter another 1000-base segment) are compacted
//   2 groups   reads sorted by (cb, ub, index) with rocPRIM; a max-scan gives the reach of every (cb, ub) run up to a read
//              (earlier molecules of a run end below the later ones, so the run's prefix maximum IS the open molecule's);
//              one lane per read finds the event that would flush the molecule after it by binary search (thresholds are
//              monotone) and compares it with the run's next read: molecule boundaries, flushing events
//   3 dups     reads sorted by (molecule, start | end, score), stable: a read equal to its predecessor is a duplicate.
//              A UMI of thousands of PCR duplicates costs its share of two sorts, no lane walks it.
//              p_group_misaligned: one lane per molecule over its compacted non-duplicate reads, float64, in read order
//   4 emit     observations of the non-duplicate reads (count -> scan -> emit), sorted by (molecule, position), stable
//   5 fold     one lane per (molecule, position): float64 products per base in read order, the 1000x rule.  A position
//              covered by thousands of molecules is thousands of independent lanes.
//   6 order    molecules by (flushing event, first read), calls by (molecule, first read that saw the position, position);
//              packed records of MOLECULE_DTYPE / SNP_CALL_DTYPE
//
// The CIGAR walk is the reference's own (snp_counter.py:37-69): H and P move the read cursor, as I and S do.  coverage.hip differs
// on purpose: it repeats pysam's aligned pairs (count_coverage), where H and P move neither cursor.
// The per-molecule and per-(molecule, position) products are sequential on purpose: their order fixes the float64 bits.
// Nothing traps: malformed input sets a flag word the host reads.  The state (the records of the last call) lives in
// dmx_ctx::d_cr_*, which nothing else touches; dmx_release_problem and dmx_destroy free it.
//
// Streaming (dmx_count_reads_begin / _push / _end, include/demux_hip_debug.h; DESIGN.md "Read counting", "Streaming"): a push runs the same six stages on
// carry + chunk.  The carry, the reads of the molecules no event has flushed yet, stays on the device between pushes
// (dmx_ctx::crs_carry, a ReadColumns).  Carried reads are never events; molecules whose flushing event is "none" are left out of stages 3 to 6
// of a push that is not final, and their reads are compacted into the next carry.
#include <climits>
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

constexpr int MOLECULE_BYTES = 12, SNP_CALL_BYTES = 13, SEGMENT = 1000, QUALITY_CAP = 40;
// flag word
constexpr int F_UNSORTED = 1, F_LAYOUT = 2, F_OP = 4, F_INDEX = 8, F_LETTER = 16, F_POSITIONS = 32;

typedef StageClock<dmx::COUNT_READS_STAGES> Clock;

__device__ __forceinline__ long long segment_of(long long start)  // Python's start // 1000
{
    return start >= 0 ? start / SEGMENT : -((-start + SEGMENT - 1) / SEGMENT);
}

// first index whose position is >= x
__device__ __forceinline__ long long lower_bound(const int *__restrict__ positions, long long P, long long x)
{
    long long lo = 0, hi = P;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (positions[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_cr_positions(const int *__restrict__ positions, long long P, int *flags)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P || i == 0) return;
    if (positions[i] <= positions[i - 1]) atomicOr(flags, F_POSITIONS);
}

// Stage 1.  A read whose arrays do not lie inside cigar / seq is flagged and treated as empty: nothing is read out of bounds.
__global__ __launch_bounds__(256) void k_cr_walk(ReadsView R, const int *__restrict__ positions, long long P, int *__restrict__ end, ull *__restrict__ n_obs, unsigned char *__restrict__ err,
                                                 ull *__restrict__ is_event, ull *__restrict__ key, unsigned *__restrict__ idx, int *flags,
                                                 long long n_carry, int has_previous, long long previous_start)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n) return;
    const long long start = R.start[i];
    // a stream's carried reads (the first n_carry) are never events; the first read behind them is compared with the last read
    // of the previous chunk, which need not be among them
    bool event = false;
    if (i == n_carry && !has_previous) {
        event = true;  // the first read of a chromosome
    } else if (i > 0 || i == n_carry) {
        const long long before = i == n_carry ? previous_start : R.start[i - 1];
        if (start < before) atomicOr(flags, F_UNSORTED);
        event = i >= n_carry && segment_of(start) != segment_of(before);
    }
    is_event[i] = event ? 1ull : 0ull;
    long long c0 = R.cigar_begin[i], nc = R.n_cigar[i];
    const long long s0 = R.seq_begin[i], ls = R.l_seq[i];
    if (outside(c0, nc, R.n_ops) || outside(s0, ls, R.n_bases)) {
        atomicOr(flags, F_LAYOUT);
        nc = 0;
    }
    long long ref = start, rd = 0, found = 0;
    unsigned e = 0;
    for (long long k = 0; k < nc; k++) {
        const unsigned c = R.cigar[c0 + k];
        const unsigned op = c & 15u;
        const long long len = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            const long long lo = lower_bound(positions, P, ref), hi = lower_bound(positions, P, ref + len);
            if (hi > lo) {
                found += hi - lo;
                if (rd + (positions[hi - 1] - ref) >= ls) e |= F_INDEX;  // the largest read index of the block
            }
            ref += len;
            rd += len;
        } else if (op == 2 || op == 3) {
            ref += len;
        } else if (op == 1 || op == 4 || op == 5 || op == 6) {
            rd += len;
        } else {
            e |= F_OP;
        }
    }
    if (ref > INT_MAX) {
        atomicOr(flags, F_LAYOUT);
        ref = INT_MAX;
    }
    end[i] = (int)ref;
    n_obs[i] = (ull)found;
    err[i] = (unsigned char)e;
    key[i] = (ull)((unsigned)R.cb[i] ^ 0x80000000u) << 32 | ((unsigned)R.ub[i] ^ 0x80000000u);
    idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void k_cr_events(const int *__restrict__ start, const ull *__restrict__ is_event, const ull *__restrict__ rank,
                                                   long long n, long long *__restrict__ threshold, unsigned *__restrict__ event_read)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !is_event[i]) return;
    threshold[rank[i] - 1] = (long long)start[i] - SEGMENT;
    event_read[rank[i] - 1] = (unsigned)i;
}

__global__ __launch_bounds__(256) void k_cr_heads(const ull *__restrict__ sorted, long long n, ull *__restrict__ head)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    head[j] = (j == 0 || sorted[j] != sorted[j - 1]) ? 1ull : 0ull;
}

// run number << 32 | biased reference_end: the prefix maximum of these is (this run, the run's reach so far)
__global__ __launch_bounds__(256) void k_cr_reach_in(const ull *__restrict__ run, const unsigned *__restrict__ idx, const int *__restrict__ end,
                                                     long long n, ull *__restrict__ out)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    out[j] = run[j] << 32 | ((unsigned)end[idx[j]] ^ 0x80000000u);
}

// Stage 2.  Read j of the sorted order is the last of its molecule when its (cb, ub) run ends with it, or when the first
// event after it that flushes the molecule (threshold above the reach) comes before the run's next read.
__global__ __launch_bounds__(256) void k_cr_bounds(const ull *__restrict__ key, const unsigned *__restrict__ idx, const ull *__restrict__ reach,
                                                   const ull *__restrict__ event_rank, const long long *__restrict__ threshold,
                                                   const unsigned *__restrict__ event_read, long long n_events, long long n,
                                                   ull *__restrict__ head, unsigned char *__restrict__ last, unsigned *__restrict__ flush)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned r = idx[j];
    const long long m = (long long)(int)((unsigned)reach[j] ^ 0x80000000u);
    long long lo = (long long)event_rank[r], hi = n_events;  // events after read r: numbers event_rank[r] ..
    while (lo < hi) {                                        // the first of them whose threshold is above m
        const long long mid = (lo + hi) >> 1;
        if (threshold[mid] > m)
            hi = mid;
        else
            lo = mid + 1;
    }
    const bool run_goes_on = j + 1 < n && key[j + 1] == key[j];
    const bool is_last = !run_goes_on || (lo < n_events && event_read[lo] < idx[j + 1]);
    last[j] = is_last ? 1 : 0;
    flush[j] = (unsigned)lo;  // n_events: the final flush
    if (j == 0) head[0] = 1ull;
    if (j + 1 < n) head[j + 1] = is_last ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_cr_groups(const ull *__restrict__ key, const unsigned *__restrict__ idx, const ull *__restrict__ head,
                                                   const ull *__restrict__ group_at, const unsigned char *__restrict__ last,
                                                   const unsigned *__restrict__ flush, const int *__restrict__ start, long long n,
                                                   unsigned *__restrict__ group_of_read, unsigned *__restrict__ g_first, unsigned *__restrict__ g_head,
                                                   unsigned *__restrict__ g_flush, ull *__restrict__ g_key, ull *__restrict__ span_head)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned g = (unsigned)(group_at[j] - 1), r = idx[j];
    group_of_read[r] = g;
    if (head[j]) {
        g_first[g] = r;
        g_head[g] = (unsigned)j;
        g_key[g] = key[j];
    }
    if (last[j]) g_flush[g] = flush[j];
    // reads of one molecule with one start are neighbours here (the input is sorted by start): spans of (molecule, start)
    span_head[j] = (head[j] || start[r] != start[idx[j - 1]]) ? 1ull : 0ull;
}

// Stage 3
__global__ __launch_bounds__(256) void k_cr_dup_keys(const unsigned *__restrict__ idx, const int *__restrict__ end, const int *__restrict__ score,
                                                     long long n, ull *__restrict__ key, unsigned *__restrict__ at)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned r = idx[j];
    key[j] = (ull)(unsigned)end[r] << 32 | (unsigned)score[r];
    at[j] = (unsigned)j;
}

__global__ __launch_bounds__(256) void k_cr_span_of(const unsigned *__restrict__ at, const ull *__restrict__ span_at, long long n,
                                                    unsigned *__restrict__ span)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    span[t] = (unsigned)(span_at[at[t]] - 1);
}

// after the two stable sorts: spans in order, inside a span (end, score) ascending, equal reads by index
__global__ __launch_bounds__(256) void k_cr_dups(const unsigned *__restrict__ span, const unsigned *__restrict__ at, const unsigned *__restrict__ idx,
                                                 const int *__restrict__ end, const int *__restrict__ score, long long n,
                                                 unsigned char *__restrict__ dup)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned r = idx[at[t]];
    bool d = false;
    if (t > 0 && span[t] == span[t - 1]) {
        const unsigned q = idx[at[t - 1]];
        d = end[q] == end[r] && score[q] == score[r];
    }
    dup[r] = d ? 1 : 0;
}

// per read: the observations it will emit, its error bits if it counts; per sorted read: is it kept
// (a read of an open molecule of a stream neither observes nor errs in this push: it is judged when its molecule is emitted)
__global__ __launch_bounds__(256) void k_cr_kept(const unsigned char *__restrict__ dup, const unsigned char *__restrict__ err,
                                                 const unsigned char *__restrict__ open, const unsigned *__restrict__ idx, long long n,
                                                 ull *__restrict__ n_obs, ull *__restrict__ kept, int *flags)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (dup[j] || open[j])
        n_obs[j] = 0ull;
    else if (err[j])
        atomicOr(flags, (int)err[j]);
    kept[j] = dup[idx[j]] ? 0ull : 1ull;
}

__global__ __launch_bounds__(256) void k_cr_kept_list(const ull *__restrict__ kept, const ull *__restrict__ kept_at, const unsigned *__restrict__ idx,
                                                      long long n, unsigned *__restrict__ list)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !kept[j]) return;
    list[kept_at[j] - 1] = idx[j];
}

// float64 product of p_misaligned over the molecule's kept reads, in read order, rounded once
__global__ __launch_bounds__(256) void k_cr_group_p(const unsigned *__restrict__ g_head, const ull *__restrict__ kept_at, const unsigned *__restrict__ list,
                                                    long long n_kept, const unsigned *__restrict__ group_of_read, const double *__restrict__ p,
                                                    long long G, float *__restrict__ g_p)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    long long k = (long long)kept_at[g_head[g]] - 1;  // a molecule's first read is never a duplicate
    double product = 1.0;
    for (; k < n_kept; k++) {
        const unsigned r = list[k];
        if (group_of_read[r] != (unsigned)g) break;
        product = product * p[r];
    }
    g_p[g] = (float)product;
}

// Stage 4: key (molecule << position_bits | position rank), value (read << 11 | base << 8 | quality), in (read, position) order
__global__ __launch_bounds__(256) void k_cr_emit(ReadsView R, const int *__restrict__ positions, long long P, const ull *__restrict__ n_obs, const ull *__restrict__ obs_at,
                                                 const unsigned *__restrict__ group_of_read, int position_bits, ull *__restrict__ key,
                                                 ull *__restrict__ value, int *flags)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n || n_obs[i] == 0) return;
    ull at = obs_at[i] - n_obs[i];
    const ull stop = obs_at[i];
    const long long c0 = R.cigar_begin[i], nc = R.n_cigar[i], s0 = R.seq_begin[i], ls = R.l_seq[i];
    const ull g = group_of_read[i];
    long long ref = R.start[i], rd = 0;
    for (long long k = 0; k < nc; k++) {
        const unsigned c = R.cigar[c0 + k];
        const unsigned op = c & 15u;
        const long long len = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            const long long lo = lower_bound(positions, P, ref), hi = lower_bound(positions, P, ref + len);
            for (long long q = lo; q < hi && at < stop; q++) {
                const long long b = rd + (positions[q] - ref);
                unsigned code = 0, quality = 0;
                if (b >= 0 && b < ls) {  // (otherwise F_INDEX is set already)
                    const unsigned char letter = R.seq[s0 + b];
                    quality = R.qual[s0 + b];
                    code = letter == 'A' ? 0 : letter == 'C' ? 1 : letter == 'G' ? 2 : letter == 'T' ? 3 : letter == 'N' ? 4 : 5;
                    if (code == 5) {
                        atomicOr(flags, F_LETTER);
                        code = 0;
                    }
                }
                key[at] = g << position_bits | (ull)q;
                value[at] = (ull)i << 11 | code << 8 | quality;
                at++;
            }
            ref += len;
            rd += len;
        } else if (op == 2 || op == 3) {
            ref += len;
        } else if (op == 1 || op == 4 || op == 5 || op == 6) {
            rd += len;
        }
    }
}

// Stage 5: the first observation of every (molecule, position) folds the run
__global__ __launch_bounds__(256) void k_cr_fold(const ull *__restrict__ key, const ull *__restrict__ value, long long n,
                                                 const double *__restrict__ table, int position_bits, ull *__restrict__ emits,
                                                 unsigned *__restrict__ c_group, unsigned *__restrict__ c_first, unsigned char *__restrict__ c_base,
                                                 float *__restrict__ c_p, unsigned char *__restrict__ has_call)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const ull k = key[t];
    if (t > 0 && key[t - 1] == k) {
        emits[t] = 0ull;
        return;
    }
    double product[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
    unsigned seen = 0;
    for (long long u = t; u < n && key[u] == k; u++) {
        const unsigned v = (unsigned)value[u] & 0x7FFu;
        const unsigned code = v >> 8, quality = v & 0xFFu;
        const double p_wrong = table[quality < QUALITY_CAP ? quality : QUALITY_CAP];
#pragma unroll
        for (unsigned b = 0; b < 5; b++)
            if (b == code) product[b] = product[b] * p_wrong;
        seen |= 1u << code;
    }
    int left = 0, base = 0;
    if (__popc(seen) > 1) {
        double best = 0.0;
        bool any = false;
#pragma unroll
        for (int b = 0; b < 5; b++)
            if ((seen >> b & 1u) && (!any || product[b] < best)) {
                best = product[b];
                any = true;
            }
        const double limit = best * 1000.0;
#pragma unroll
        for (int b = 0; b < 5; b++)
            if ((seen >> b & 1u) && product[b] <= limit) {
                left++;
                base = b;
            }
    } else {
        left = 1;
        base = __ffs((int)seen) - 1;
    }
    emits[t] = left == 1 ? 1ull : 0ull;
    if (left != 1) return;
    double p = product[0];
#pragma unroll
    for (int b = 1; b < 5; b++)
        if (b == base) p = product[b];
    const unsigned g = (unsigned)(k >> position_bits);
    c_group[t] = g;
    c_first[t] = (unsigned)(value[t] >> 11);  // the run is in read order: its first observation is the first read's
    c_base[t] = (unsigned char)base;
    c_p[t] = (float)p;
    has_call[g] = 1;
}

// Stage 6
__global__ __launch_bounds__(256) void k_cr_group_keys(const unsigned *__restrict__ g_flush, const unsigned *__restrict__ g_first, long long G,
                                                       ull *__restrict__ key, unsigned *__restrict__ value)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    key[g] = (ull)g_flush[g] << 32 | g_first[g];
    value[g] = (unsigned)g;
}

__global__ __launch_bounds__(256) void k_cr_group_flags(const unsigned *__restrict__ order, const unsigned char *__restrict__ has_call, long long G,
                                                        ull *__restrict__ flag)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= G) return;
    flag[k] = has_call[order[k]] ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_cr_molecules(const unsigned *__restrict__ order, const ull *__restrict__ flag, const ull *__restrict__ at,
                                                      long long G, const ull *__restrict__ g_key, const float *__restrict__ g_p,
                                                      unsigned *__restrict__ molecule_of_group, unsigned char *__restrict__ records)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= G || !flag[k]) return;
    const unsigned g = order[k];
    const ull m = at[k] - 1;
    molecule_of_group[g] = (unsigned)m;
    const int cb = (int)((unsigned)(g_key[g] >> 32) ^ 0x80000000u), ub = (int)((unsigned)g_key[g] ^ 0x80000000u);
    int *record = (int *)(records + m * MOLECULE_BYTES);  // 12-byte records: 4-byte aligned
    record[0] = cb;
    record[1] = ub;
    record[2] = __float_as_int(g_p[g]);
}

__global__ __launch_bounds__(256) void k_cr_call_keys(const ull *__restrict__ emits, const ull *__restrict__ at, long long n,
                                                      const unsigned *__restrict__ c_group, const unsigned *__restrict__ c_first,
                                                      const unsigned *__restrict__ molecule_of_group, ull *__restrict__ key,
                                                      unsigned *__restrict__ source)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n || !emits[t]) return;
    const ull o = at[t] - 1;
    key[o] = (ull)molecule_of_group[c_group[t]] << 32 | c_first[t];
    source[o] = (unsigned)t;
}

__global__ __launch_bounds__(256) void k_cr_calls(const ull *__restrict__ key, const unsigned *__restrict__ source, long long n_calls,
                                                  const ull *__restrict__ obs_key, int position_bits, const int *__restrict__ positions,
                                                  const unsigned char *__restrict__ c_base, const float *__restrict__ c_p,
                                                  long long molecule_base, unsigned char *__restrict__ records)
{
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_calls) return;
    const unsigned t = source[o];
    const int molecule = (int)(molecule_base + (long long)(key[o] >> 32));  // (a stream counts its molecules on across pushes)
    const int position = positions[obs_key[t] & ((1ull << position_bits) - 1)];
    const float p = c_p[t];
    unsigned char *record = records + o * SNP_CALL_BYTES;  // packed 13-byte records: bytes
    __builtin_memcpy(record, &molecule, 4);
    __builtin_memcpy(record + 4, &position, 4);
    record[8] = c_base[t];
    __builtin_memcpy(record + 9, &p, 4);
}

// ---- streaming: the combined input of a push, the open molecules, the next carry

// The chunk's reads lie behind the carry's in the combined arrays: their cigar_begin / seq_begin move by the carry's lengths.
// A begin outside the chunk's own arrays is flagged and pinned to the chunk's end (the walk then sees an empty or flagged read).
__global__ __launch_bounds__(256) void k_cr_rebase(long long *__restrict__ cigar_begin, long long *__restrict__ seq_begin, long long n_carry,
                                                   long long n, long long carry_ops, long long carry_bases, long long chunk_ops,
                                                   long long chunk_bases, int *flags)
{
    const long long i = n_carry + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long c0 = cigar_begin[i], s0 = seq_begin[i];
    if (c0 < 0 || c0 > chunk_ops || s0 < 0 || s0 > chunk_bases) {
        atomicOr(flags, F_LAYOUT);
        c0 = chunk_ops;
        s0 = chunk_bases;
    }
    cigar_begin[i] = c0 + carry_ops;
    seq_begin[i] = s0 + carry_bases;
}

// per read: does its molecule stay open (no event of this push flushes it)
__global__ __launch_bounds__(256) void k_cr_open(const unsigned *__restrict__ group_of_read, const unsigned *__restrict__ g_flush,
                                                 long long n_events, long long n, unsigned char *__restrict__ open)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    open[i] = (long long)g_flush[group_of_read[i]] == n_events ? 1 : 0;
}

// what every read adds to the next carry (run once the walk's layout flag was read: the lengths are valid)
__global__ __launch_bounds__(256) void k_cr_carry_sizes(const unsigned char *__restrict__ open, const int *__restrict__ n_cigar,
                                                        const int *__restrict__ l_seq, long long n, ull *__restrict__ reads,
                                                        ull *__restrict__ ops, ull *__restrict__ bases)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool o = open[i] != 0;
    reads[i] = o ? 1ull : 0ull;
    ops[i] = o ? (ull)n_cigar[i] : 0ull;
    bases[i] = o ? (ull)l_seq[i] : 0ull;
}

// the nine per-read columns of the open reads, in read order; cigar_begin / seq_begin count from the carry's own start
__global__ __launch_bounds__(256) void k_cr_carry_reads(ReadsView R, const unsigned char *__restrict__ open, const ull *__restrict__ read_at,
                                                        const ull *__restrict__ ops_at, const ull *__restrict__ bases_at, ReadsOut out,
                                                        long long *__restrict__ old_cigar_begin, long long *__restrict__ old_seq_begin)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n || !open[i]) return;
    const long long k = (long long)read_at[i] - 1;
    out.start[k] = R.start[i];
    out.cb[k] = R.cb[i];
    out.ub[k] = R.ub[i];
    out.score[k] = R.score[i];
    out.n_cigar[k] = R.n_cigar[i];
    out.l_seq[k] = R.l_seq[i];
    out.p_misaligned[k] = R.p_misaligned[i];
    out.cigar_begin[k] = (long long)ops_at[i] - R.n_cigar[i];
    out.seq_begin[k] = (long long)bases_at[i] - R.l_seq[i];
    old_cigar_begin[k] = R.cigar_begin[i];
    old_seq_begin[k] = R.seq_begin[i];
}

// the carried read that owns element e of the carry's cigar / seq: the last one whose begin is <= e (reads without elements
// share their begin with the read behind them, which is then the one found)
__device__ __forceinline__ long long owner_of(const long long *__restrict__ begin, long long n, long long e)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (begin[mid] <= e)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

// One lane per element, not one per read: a molecule held open by a long N-skip rides through many pushes, and a read's
// bases are copied by as many lanes as it has bases.
__global__ __launch_bounds__(256) void k_cr_carry_ops(const long long *__restrict__ begin, const long long *__restrict__ old_begin,
                                                      long long n_reads, long long n_ops, const unsigned *__restrict__ cigar,
                                                      unsigned *__restrict__ out)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ops) return;
    const long long k = owner_of(begin, n_reads, e);
    out[e] = cigar[old_begin[k] + (e - begin[k])];
}

__global__ __launch_bounds__(256) void k_cr_carry_bases(const long long *__restrict__ begin, const long long *__restrict__ old_begin,
                                                        long long n_reads, long long n_bases, const unsigned char *__restrict__ seq,
                                                        const unsigned char *__restrict__ qual, unsigned char *__restrict__ seq_out,
                                                        unsigned char *__restrict__ qual_out)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_bases) return;
    const long long k = owner_of(begin, n_reads, e);
    const long long from = old_begin[k] + (e - begin[k]);
    seq_out[e] = seq[from];
    qual_out[e] = qual[from];
}

int flag_error(int flags)
{
    if (flags & F_POSITIONS) return fail(DMX_ERR_INVALID, "count_reads: positions must be strictly ascending");
    if (flags & F_LAYOUT) return fail(DMX_ERR_INVALID, "count_reads: a read's cigar / seq range lies outside the arrays, or its reference_end is beyond 2^31");
    if (flags & F_UNSORTED) return fail(DMX_ERR_INVALID, "count_reads: reference_start must be non-decreasing in read order");
    if (flags & F_OP) return fail(DMX_ERR_INVALID, "count_reads: unknown CIGAR operation (codes 0 .. 8 are known)");
    if (flags & F_INDEX) return fail(DMX_ERR_INVALID, "count_reads: a SNP position falls on a base beyond l_seq");
    if (flags & F_LETTER) return fail(DMX_ERR_INVALID, "count_reads: a base other than A, C, G, T, N at a SNP position");
    return 0;
}

// what a pass over carry + chunk knows of its stream (the one-shot call: the defaults)
struct Pass {
    long long n_carry = 0, previous_start = 0, molecule_base = 0;
    bool has_previous = false;  // a read came before the chunk's first: previous_start is the last one's start
    bool keep_open = false;     // not the final push: molecules no event flushes stay behind as the next carry
    size_t resident_bytes = 0;  // the stream's positions and table (the peak meter counts the input whole)
};

// ---- the gather: the reads flagged in open[] out of a view, in read order, into columns whose cigar / seq / qual segments
// lie behind one another.  The next carry of a push is one (the open molecules' reads), a range of a resident set another
// (every read flagged).  The plan finds the sizes, for the destination to be allocated by; the run copies.
struct Gather {
    const unsigned char *open = nullptr;
    ull *read_at = nullptr, *ops_at = nullptr, *bases_at = nullptr;  // inclusive scans over the reads of what the flagged ones hold
    ReadCounts total;
};

// work: six arrays of R.n elements the caller has free (the three scans stay in them until the run).  R's lengths are valid.
int gather_plan(Scratch &sc, const ReadsView &R, const unsigned char *open, ull *const work[6], Gather *g, hipStream_t st)
{
    ull n_reads = 0, n_ops = 0, n_bases = 0;
    g->open = open, g->read_at = work[3], g->ops_at = work[4], g->bases_at = work[5];
    hipLaunchKernelGGL(k_cr_carry_sizes, dim3(grid_for(R.n)), dim3(256), 0, st, open, R.n_cigar, R.l_seq, R.n, work[0], work[1], work[2]);
    DMX_TRY(launched("k_cr_carry_sizes"));
    DMX_TRY(sum_scan(sc, work[0], g->read_at, (size_t)R.n, &n_reads, st));
    if (n_reads) {
        DMX_TRY(sum_scan(sc, work[1], g->ops_at, (size_t)R.n, &n_ops, st));
        DMX_TRY(sum_scan(sc, work[2], g->bases_at, (size_t)R.n, &n_bases, st));
    }
    g->total.n = (long long)n_reads, g->total.n_ops = (long long)n_ops, g->total.n_bases = (long long)n_bases;
    return 0;
}

// out: room for g.total; its cigar_begin / seq_begin count from out's own cigar / seq
int gather_run(Scratch &sc, const ReadsView &R, const Gather &g, const ReadsOut &out, hipStream_t st)
{
    if (!g.total.n) return 0;
    long long *old_cigar_begin, *old_seq_begin;
    DMX_TRY(sc.get(&old_cigar_begin, g.total.of(PER_READ)));
    DMX_TRY(sc.get(&old_seq_begin, g.total.of(PER_READ)));
    hipLaunchKernelGGL(k_cr_carry_reads, dim3(grid_for(R.n)), dim3(256), 0, st, R, g.open, g.read_at, g.ops_at, g.bases_at, out, old_cigar_begin,
                       old_seq_begin);
    DMX_TRY(launched("k_cr_carry_reads"));
    if (g.total.n_ops) hipLaunchKernelGGL(k_cr_carry_ops, dim3(grid_for(g.total.n_ops)), dim3(256), 0, st, out.cigar_begin, old_cigar_begin,
                                          g.total.n, g.total.n_ops, R.cigar, out.cigar);
    DMX_TRY(launched("k_cr_carry_ops"));
    if (g.total.n_bases) hipLaunchKernelGGL(k_cr_carry_bases, dim3(grid_for(g.total.n_bases)), dim3(256), 0, st, out.seq_begin, old_seq_begin,
                                            g.total.n, g.total.n_bases, R.seq, R.qual, out.seq, out.qual);
    DMX_TRY(launched("k_cr_carry_bases"));
    return 0;
}

// The six stages on the reads R (device arrays; the first pass.n_carry are a stream's carry) and the P positions, then the
// next carry.
int count_pass(dmx_ctx *c, Scratch &sc, Clock &clock, const ReadsView &R, const int *d_positions, long long P, int *flags, const double *d_table,
               const Pass &pass, long long *n_molecules, long long *n_calls)
{
    hipStream_t st = c->stream;
    const long long n = R.n;

    // ---- 1 walk
    int *end;
    ull *n_obs, *is_event, *event_rank, *key;
    unsigned char *err;
    unsigned *idx;
    DMX_TRY(sc.get(&end, (size_t)n));
    DMX_TRY(sc.get(&n_obs, (size_t)n));
    DMX_TRY(sc.get(&is_event, (size_t)n));
    DMX_TRY(sc.get(&event_rank, (size_t)n));
    DMX_TRY(sc.get(&key, (size_t)n));
    DMX_TRY(sc.get(&err, (size_t)n));
    DMX_TRY(sc.get(&idx, (size_t)n));
    hipLaunchKernelGGL(k_cr_walk, dim3(grid_for(n)), dim3(256), 0, st, R, d_positions, P, end, n_obs, err, is_event, key, idx, flags,
                       pass.n_carry,
                       pass.has_previous ? 1 : 0, pass.previous_start);
    DMX_TRY(launched("k_cr_walk"));
    ull n_events = 0;
    DMX_TRY(sum_scan(sc, is_event, event_rank, (size_t)n, &n_events, st));  // (the caller's arrays are free to change from here on)
    long long *threshold;
    unsigned *event_read;
    DMX_TRY(sc.get(&threshold, (size_t)n_events));
    DMX_TRY(sc.get(&event_read, (size_t)n_events));
    hipLaunchKernelGGL(k_cr_events, dim3(grid_for(n)), dim3(256), 0, st, R.start, is_event, event_rank, n, threshold, event_read);
    DMX_TRY(launched("k_cr_events"));
    DMX_TRY(clock.tick(st));

    // ---- 2 groups
    ull *skey, *head, *run, *reach_in, *reach, *group_at, *span_head, *span_at;
    unsigned *sidx, *flush;
    unsigned char *last;
    DMX_TRY(sc.get(&skey, (size_t)n));
    DMX_TRY(sc.get(&sidx, (size_t)n));
    DMX_TRY(sc.get(&head, (size_t)n));
    DMX_TRY(sc.get(&run, (size_t)n));
    DMX_TRY(sc.get(&reach_in, (size_t)n));
    DMX_TRY(sc.get(&reach, (size_t)n));
    DMX_TRY(sc.get(&group_at, (size_t)n));
    DMX_TRY(sc.get(&span_head, (size_t)n));
    DMX_TRY(sc.get(&span_at, (size_t)n));
    DMX_TRY(sc.get(&flush, (size_t)n));
    DMX_TRY(sc.get(&last, (size_t)n));
    DMX_TRY(sort_pairs(sc, key, skey, idx, sidx, (size_t)n, 64u, st));
    hipLaunchKernelGGL(k_cr_heads, dim3(grid_for(n)), dim3(256), 0, st, skey, n, head);
    DMX_TRY(launched("k_cr_heads"));
    ull n_runs = 0, top = 0, G = 0, n_spans = 0;
    DMX_TRY(sum_scan(sc, head, run, (size_t)n, &n_runs, st));
    hipLaunchKernelGGL(k_cr_reach_in, dim3(grid_for(n)), dim3(256), 0, st, run, sidx, end, n, reach_in);
    DMX_TRY(launched("k_cr_reach_in"));
    DMX_TRY(inclusive_scan_total(sc, reach_in, reach, (size_t)n, &top, rocprim::maximum<ull>(), st));
    hipLaunchKernelGGL(k_cr_bounds, dim3(grid_for(n)), dim3(256), 0, st, skey, sidx, reach, event_rank, threshold, event_read,
                       (long long)n_events, n, head, last, flush);
    DMX_TRY(launched("k_cr_bounds"));
    DMX_TRY(sum_scan(sc, head, group_at, (size_t)n, &G, st));
    unsigned *group_of_read, *g_first, *g_head, *g_flush;
    ull *g_key;
    float *g_p;
    DMX_TRY(sc.get(&group_of_read, (size_t)n));
    DMX_TRY(sc.get(&g_first, (size_t)G));
    DMX_TRY(sc.get(&g_head, (size_t)G));
    DMX_TRY(sc.get(&g_flush, (size_t)G));
    DMX_TRY(sc.get(&g_key, (size_t)G));
    DMX_TRY(sc.get(&g_p, (size_t)G));
    hipLaunchKernelGGL(k_cr_groups, dim3(grid_for(n)), dim3(256), 0, st, skey, sidx, head, group_at, last, flush, R.start, n, group_of_read,
                       g_first, g_head, g_flush, g_key, span_head);
    DMX_TRY(launched("k_cr_groups"));
    // a stream's open molecules: no event of this push flushes them (a final push and the one-shot call flush everything)
    unsigned char *open;
    DMX_TRY(sc.get(&open, (size_t)n));
    if (pass.keep_open) {
        hipLaunchKernelGGL(k_cr_open, dim3(grid_for(n)), dim3(256), 0, st, group_of_read, g_flush, (long long)n_events, n, open);
        DMX_TRY(launched("k_cr_open"));
    } else {
        HIP_TRY(hipMemsetAsync(open, 0, (size_t)n, st));
    }
    DMX_TRY(clock.tick(st));

    // ---- 3 duplicates, p_group_misaligned
    DMX_TRY(sum_scan(sc, span_head, span_at, (size_t)n, &n_spans, st));
    ull *dkey = reach_in, *dkey_sorted = reach;  // (their contents are no longer needed)
    unsigned *at, *at_sorted, *span, *span_sorted, *at_final;
    unsigned char *dup;
    DMX_TRY(sc.get(&at, (size_t)n));
    DMX_TRY(sc.get(&at_sorted, (size_t)n));
    DMX_TRY(sc.get(&span, (size_t)n));
    DMX_TRY(sc.get(&span_sorted, (size_t)n));
    DMX_TRY(sc.get(&at_final, (size_t)n));
    DMX_TRY(sc.get(&dup, (size_t)n));
    hipLaunchKernelGGL(k_cr_dup_keys, dim3(grid_for(n)), dim3(256), 0, st, sidx, end, R.score, n, dkey, at);
    DMX_TRY(launched("k_cr_dup_keys"));
    DMX_TRY(sort_pairs(sc, dkey, dkey_sorted, at, at_sorted, (size_t)n, 64u, st));
    hipLaunchKernelGGL(k_cr_span_of, dim3(grid_for(n)), dim3(256), 0, st, at_sorted, span_at, n, span);
    DMX_TRY(launched("k_cr_span_of"));
    DMX_TRY(sort_pairs(sc, span, span_sorted, at_sorted, at_final, (size_t)n, (unsigned)bits_for(n_spans), st));
    hipLaunchKernelGGL(k_cr_dups, dim3(grid_for(n)), dim3(256), 0, st, span_sorted, at_final, sidx, end, R.score, n, dup);
    DMX_TRY(launched("k_cr_dups"));
    ull *kept = run, *kept_at = head, *obs_at = is_event, n_kept = 0, n_observations = 0;
    hipLaunchKernelGGL(k_cr_kept, dim3(grid_for(n)), dim3(256), 0, st, dup, err, open, sidx, n, n_obs, kept, flags);
    DMX_TRY(launched("k_cr_kept"));
    DMX_TRY(sum_scan(sc, kept, kept_at, (size_t)n, &n_kept, st));
    unsigned *kept_list;
    DMX_TRY(sc.get(&kept_list, (size_t)n_kept));
    hipLaunchKernelGGL(k_cr_kept_list, dim3(grid_for(n)), dim3(256), 0, st, kept, kept_at, sidx, n, kept_list);
    DMX_TRY(launched("k_cr_kept_list"));
    hipLaunchKernelGGL(k_cr_group_p, dim3(grid_for((long long)G)), dim3(256), 0, st, g_head, kept_at, kept_list, (long long)n_kept, group_of_read,
                       R.p_misaligned, (long long)G, g_p);
    DMX_TRY(launched("k_cr_group_p"));
    DMX_TRY(clock.tick(st));

    // ---- 4 observations
    DMX_TRY(sum_scan(sc, n_obs, obs_at, (size_t)n, &n_observations, st));
    int h_flags = 0;
    HIP_TRY(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    DMX_TRY(flag_error(h_flags));
    const int position_bits = bits_for((ull)P), group_bits = bits_for(G);
    if (position_bits + group_bits > 64) return fail(DMX_ERR_UNSUPPORTED, "count_reads: %llu molecules x %lld positions do not fit a 64-bit key", G, P);
    if (n_observations >= (1ull << 32)) return fail(DMX_ERR_UNSUPPORTED, "count_reads: %llu observations in one call (at most 2^32 - 1): split the chromosome", n_observations);
    const long long n_o = (long long)n_observations;
    ull *okey, *oval, *okey_sorted, *oval_sorted;
    DMX_TRY(sc.get(&okey, (size_t)n_o));
    DMX_TRY(sc.get(&oval, (size_t)n_o));
    DMX_TRY(sc.get(&okey_sorted, (size_t)n_o));
    DMX_TRY(sc.get(&oval_sorted, (size_t)n_o));
    hipLaunchKernelGGL(k_cr_emit, dim3(grid_for(n)), dim3(256), 0, st, R, d_positions, P, n_obs, obs_at, group_of_read, position_bits, okey,
                       oval, flags);
    DMX_TRY(launched("k_cr_emit"));
    DMX_TRY(sort_pairs(sc, okey, okey_sorted, oval, oval_sorted, (size_t)n_o, (unsigned)(position_bits + group_bits), st));
    DMX_TRY(clock.tick(st));

    // ---- 5 fold
    ull *emits = okey, *emit_at = oval, n_c = 0;  // (the unsorted observations are no longer needed)
    unsigned *c_group, *c_first;
    unsigned char *c_base, *has_call;
    float *c_p;
    DMX_TRY(sc.get(&c_group, (size_t)n_o));
    DMX_TRY(sc.get(&c_first, (size_t)n_o));
    DMX_TRY(sc.get(&c_base, (size_t)n_o));
    DMX_TRY(sc.get(&c_p, (size_t)n_o));
    DMX_TRY(sc.get(&has_call, (size_t)G));
    HIP_TRY(hipMemsetAsync(has_call, 0, (size_t)(G ? G : 1), st));
    if (n_o) hipLaunchKernelGGL(k_cr_fold, dim3(grid_for(n_o)), dim3(256), 0, st, okey_sorted, oval_sorted, n_o, d_table, position_bits, emits,
                                c_group, c_first, c_base, c_p, has_call);
    DMX_TRY(launched("k_cr_fold"));
    DMX_TRY(sum_scan(sc, emits, emit_at, (size_t)n_o, &n_c, st));
    HIP_TRY(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    DMX_TRY(flag_error(h_flags));
    DMX_TRY(clock.tick(st));

    // ---- 6 order, records
    ull *gkey, *gkey_sorted, *gflag, *gflag_at, n_m = 0;
    unsigned *gval, *gorder, *molecule_of_group;
    DMX_TRY(sc.get(&gkey, (size_t)G));
    DMX_TRY(sc.get(&gkey_sorted, (size_t)G));
    DMX_TRY(sc.get(&gflag, (size_t)G));
    DMX_TRY(sc.get(&gflag_at, (size_t)G));
    DMX_TRY(sc.get(&gval, (size_t)G));
    DMX_TRY(sc.get(&gorder, (size_t)G));
    DMX_TRY(sc.get(&molecule_of_group, (size_t)G));
    hipLaunchKernelGGL(k_cr_group_keys, dim3(grid_for((long long)G)), dim3(256), 0, st, g_flush, g_first, (long long)G, gkey, gval);
    DMX_TRY(launched("k_cr_group_keys"));
    DMX_TRY(sort_pairs(sc, gkey, gkey_sorted, gval, gorder, (size_t)G, (unsigned)(32 + bits_for(n_events + 1)), st));
    hipLaunchKernelGGL(k_cr_group_flags, dim3(grid_for((long long)G)), dim3(256), 0, st, gorder, has_call, (long long)G, gflag);
    DMX_TRY(launched("k_cr_group_flags"));
    DMX_TRY(sum_scan(sc, gflag, gflag_at, (size_t)G, &n_m, st));
    if (pass.molecule_base + (long long)n_m > INT_MAX)
        return fail(DMX_ERR_UNSUPPORTED, "count_reads: more than 2^31 - 1 molecules in one stream");
    DMX_TRY(dev_alloc(c, c->d_cr_molecules, (size_t)n_m * MOLECULE_BYTES));
    DMX_TRY(dev_alloc(c, c->d_cr_calls, (size_t)n_c * SNP_CALL_BYTES));
    hipLaunchKernelGGL(k_cr_molecules, dim3(grid_for((long long)G)), dim3(256), 0, st, gorder, gflag, gflag_at, (long long)G, g_key, g_p,
                       molecule_of_group, c->d_cr_molecules.p);
    DMX_TRY(launched("k_cr_molecules"));
    if (n_c) {
        ull *ckey, *ckey_sorted;
        unsigned *csrc, *csrc_sorted;
        DMX_TRY(sc.get(&ckey, (size_t)n_c));
        DMX_TRY(sc.get(&ckey_sorted, (size_t)n_c));
        DMX_TRY(sc.get(&csrc, (size_t)n_c));
        DMX_TRY(sc.get(&csrc_sorted, (size_t)n_c));
        hipLaunchKernelGGL(k_cr_call_keys, dim3(grid_for(n_o)), dim3(256), 0, st, emits, emit_at, n_o, c_group, c_first, molecule_of_group, ckey, csrc);
        DMX_TRY(launched("k_cr_call_keys"));
        DMX_TRY(sort_pairs(sc, ckey, ckey_sorted, csrc, csrc_sorted, (size_t)n_c, (unsigned)(32 + bits_for(n_m)), st));
        hipLaunchKernelGGL(k_cr_calls, dim3(grid_for((long long)n_c)), dim3(256), 0, st, ckey_sorted, csrc_sorted, (long long)n_c, okey_sorted,
                           position_bits, d_positions, c_base, c_p, pass.molecule_base, c->d_cr_calls.p);
        DMX_TRY(launched("k_cr_calls"));
    }
    // ---- the next carry: the open molecules' reads in read order, their cigar / seq / qual segments behind one another
    if (pass.keep_open) {
        ull *const free_now[6] = {span_head, span_at, group_at, reach_in, reach, skey};
        Gather open_reads;
        DMX_TRY(gather_plan(sc, R, open, free_now, &open_reads, st));
        if (open_reads.total.n) DMX_TRY(alloc_read_columns(c, c->crs_carry, open_reads.total, true));
        DMX_TRY(gather_run(sc, R, open_reads, out_of(c->crs_carry), st));
    }
    DMX_TRY(clock.tick(st));
    HIP_TRY(hipStreamSynchronize(st));
    DMX_TRY(clock.read(c->cr_stage_ms, 0));
    c->cr_molecules = (long long)n_m;
    c->cr_calls = (long long)n_c;
    c->cr_peak_bytes = (int64_t)(sc.held + pass.resident_bytes + read_columns_bytes(c->crs_carry));
    *n_molecules = (long long)n_m;
    *n_calls = (long long)n_c;
    return 0;
}

// dmx_count_reads and dmx_count_reads_resident: place() gives the reads, uploaded into the call's temporaries or a resident
// set's own buffers, which the six stages then read in place
template <typename Place>
int count_reads(dmx_ctx *c, Place place, const int32_t *positions, long long P, const double *table, long long *n_molecules, long long *n_calls)
{
    hipStream_t st = c->stream;
    dmx::host::release_count_reads(c);
    Scratch sc(c);
    Clock clock;
    DMX_TRY(clock.tick(st));
    ReadsView R;
    DMX_TRY(place(sc, &R));
    int *d_positions, *flags;
    double *d_table;
    DMX_TRY(upload(sc, &d_positions, positions, (size_t)P, st));
    DMX_TRY(upload(sc, &d_table, table, (size_t)QUALITY_CAP + 1, st));
    DMX_TRY(sc.get(&flags, 1));
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int), st));
    DMX_TRY(clock.tick(st));
    if (P) hipLaunchKernelGGL(k_cr_positions, dim3(grid_for(P)), dim3(256), 0, st, d_positions, P, flags);
    DMX_TRY(launched("k_cr_positions"));
    return count_pass(c, sc, clock, R, d_positions, P, flags, d_table, Pass(), n_molecules, n_calls);
}

// ---- streaming

enum { STREAM_NONE = 0, STREAM_OPEN = 1, STREAM_FINISHED = 2, STREAM_DEAD = 3 };  // dmx_ctx::crs_state

// A chunk of host arrays: its sizes are the caller's, its columns are uploaded behind the carry's; cigar_begin / seq_begin
// count from the chunk's own arrays (k_cr_rebase moves them).
struct HostChunk {
    const dmx_decoded_reads *h;
    size_t n() const { return h ? (size_t)h->n_reads : 0; }
    int ends(dmx_ctx *, int *first, int *last) const
    {
        *first = h->reference_start[0];
        *last = h->reference_start[h->n_reads - 1];
        return 0;
    }
    int measure(dmx_ctx *, Scratch &, int *, Gather *g) const
    {
        if (h) g->total = host_reads(h);
        return 0;
    }
    int place(dmx_ctx *c, Scratch &, const Gather &, const ReadsOut &out) const
    {
        if (!h) return 0;
        DMX_TRY(copy_in(out, host_reads(h), true, c->stream));
        c->reads_upload_bytes += dmx::host::decoded_reads_bytes(h->n_reads, h->n_cigar_ops, h->n_bases, true);
        return 0;
    }
};

// per read of a range of a resident set: do its cigar / seq ranges lie inside the set's arrays (what the gather relies on)
__global__ __launch_bounds__(256) void k_rr_check_range(ReadsView R, int *flags)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n) return;
    const long long c0 = R.cigar_begin[i], nc = R.n_cigar[i], s0 = R.seq_begin[i], ls = R.l_seq[i];
    if (outside(c0, nc, R.n_ops) || outside(s0, ls, R.n_bases)) atomicOr(flags, F_LAYOUT);
}

// A range of a countable resident set.  cigar_begin and seq_begin of a set are arbitrary offsets, so the range is no contiguous
// range of operations or bases: it is gathered behind the carry the way the carry itself is placed, every read flagged.
struct ResidentChunk {
    const ResidentReads *set;
    long long first, count;
    size_t n() const { return (size_t)count; }
    ReadsView reads() const { return view_of(set->columns, first, count, true); }
    int ends(dmx_ctx *c, int *lo, int *hi) const
    {
        const int *start = set->columns.start.p + first;
        HIP_TRY(hipMemcpyAsync(lo, start, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hi, start + count - 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    }
    int measure(dmx_ctx *c, Scratch &sc, int *flags, Gather *g) const
    {
        hipStream_t st = c->stream;
        if (!count) return 0;
        hipLaunchKernelGGL(k_rr_check_range, dim3(grid_for(count)), dim3(256), 0, st, reads(), flags);
        DMX_TRY(launched("k_rr_check_range"));
        int h_flags = 0;
        HIP_TRY(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        DMX_TRY(flag_error(h_flags));  // (the lengths are valid from here on)
        unsigned char *every;
        ull *work[6];
        DMX_TRY(sc.get(&every, (size_t)count));
        for (ull *&w : work) DMX_TRY(sc.get(&w, (size_t)count));
        HIP_TRY(hipMemsetAsync(every, 1, (size_t)count, st));
        return gather_plan(sc, reads(), every, work, g, st);
    }
    int place(dmx_ctx *c, Scratch &sc, const Gather &g, const ReadsOut &out) const
    {
        return count ? gather_run(sc, reads(), g, out, c->stream) : 0;  // (begins from the chunk's own start: k_cr_rebase moves them)
    }
};

template <typename Chunk>
int stream_push(dmx_ctx *c, const Chunk &chunk, bool final, long long *n_molecules, long long *n_calls)
{
    hipStream_t st = c->stream;
    dmx::host::release_count_reads(c);
    const size_t n_chunk = chunk.n();
    const ReadCounts carry = c->crs_carry;
    if (carry.of(PER_READ) + n_chunk > (size_t)INT_MAX)
        return fail(DMX_ERR_UNSUPPORTED, "count_reads_push: %zu carried reads + %zu reads of the chunk (at most 2^31 - 1 in one push)",
                    carry.of(PER_READ), n_chunk);
    int first_start = 0, last_start = 0;
    if (n_chunk) DMX_TRY(chunk.ends(c, &first_start, &last_start));
    if (n_chunk && c->crs_has_previous && first_start < c->crs_previous_start)
        return fail(DMX_ERR_INVALID, "count_reads_push: the chunk starts at %d, below the previous chunk's last reference_start %lld",
                    first_start, c->crs_previous_start);
    Pass pass;
    pass.n_carry = carry.n, pass.previous_start = c->crs_previous_start, pass.has_previous = c->crs_has_previous;
    pass.molecule_base = c->crs_molecules, pass.keep_open = !final;
    pass.resident_bytes = dev_bytes(c->d_crs_positions) + dev_bytes(c->d_crs_table);
    long long n_m = 0, n_c = 0;
    if (carry.of(PER_READ) + n_chunk == 0) {  // nothing to count: no records (a first or a final push without reads)
        c->cr_molecules = c->cr_calls = 0;
        for (double &ms : c->cr_stage_ms) ms = 0.0;
        c->cr_peak_bytes = (int64_t)pass.resident_bytes;
    } else {
        Scratch sc(c);
        Clock clock;
        DMX_TRY(clock.tick(st));
        int *flags;
        DMX_TRY(sc.get(&flags, 1));
        HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int), st));
        Gather measured;
        DMX_TRY(chunk.measure(c, sc, flags, &measured));
        const ReadCounts in = measured.total;
        ReadCounts all;
        all.n = carry.n + in.n, all.n_ops = carry.n_ops + in.n_ops, all.n_bases = carry.n_bases + in.n_bases;
        // the columns of carry + chunk: room for both, the carry copied device to device, the chunk placed behind it
        ReadsOut d;
        DMX_TRY(each_read_column(
            [&](ReadExtent e, bool, auto &to, const auto &held) {
                DMX_TRY(sc.get(&to, all.of(e)));
                if (carry.of(e)) HIP_TRY(hipMemcpyAsync(to, held.p, carry.of(e) * sizeof(*to), hipMemcpyDeviceToDevice, st));
                return 0;
            },
            d, c->crs_carry));
        DMX_TRY(chunk.place(c, sc, measured, offset(d, carry)));
        dmx::host::release_count_reads_carry(c);  // (stream order: the copies above read the blocks before anything re-uses them)
        if (n_chunk) hipLaunchKernelGGL(k_cr_rebase, dim3(grid_for(in.n)), dim3(256), 0, st, d.cigar_begin, d.seq_begin, carry.n, all.n, carry.n_ops,
                                        carry.n_bases, in.n_ops, in.n_bases, flags);
        DMX_TRY(launched("k_cr_rebase"));
        DMX_TRY(clock.tick(st));
        DMX_TRY(count_pass(c, sc, clock, view_of(d, all), c->d_crs_positions.p, c->crs_P, flags, c->d_crs_table.p, pass, &n_m, &n_c));
    }
    if (n_chunk) {
        c->crs_previous_start = last_start;
        c->crs_has_previous = true;
    }
    c->crs_molecules += n_m;
    c->cr_carried = c->crs_carry.n;
    *n_molecules = n_m;
    *n_calls = n_c;
    return 0;
}

int stream_begin(dmx_ctx *c, const int32_t *positions, long long P, const double *table)
{
    hipStream_t st = c->stream;
    Scratch sc(c);
    int *flags, h_flags = 0;
    DMX_TRY(dev_alloc(c, c->d_crs_positions, (size_t)P));
    DMX_TRY(dev_alloc(c, c->d_crs_table, (size_t)QUALITY_CAP + 1));
    if (P) HIP_TRY(hipMemcpyAsync(c->d_crs_positions.p, positions, (size_t)P * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->d_crs_table.p, table, ((size_t)QUALITY_CAP + 1) * sizeof(double), hipMemcpyHostToDevice, st));
    DMX_TRY(sc.get(&flags, 1));
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int), st));
    if (P) hipLaunchKernelGGL(k_cr_positions, dim3(grid_for(P)), dim3(256), 0, st, c->d_crs_positions.p, P, flags);
    DMX_TRY(launched("k_cr_positions"));
    HIP_TRY(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    DMX_TRY(flag_error(h_flags));
    c->crs_P = P;
    return 0;
}

bool bad_positions(const int32_t *positions, int64_t n_positions) { return n_positions < 0 || n_positions > INT_MAX || (n_positions && !positions); }

// What both one-shot entry points do around the pass.  input() looks at the reads the call names and says how many they are;
// pass() counts them.  Without reads there are no records; a failed pass leaves none.
template <typename Input, typename CountPass>
int count_once(dmx_ctx *c, const char *who, bool null_input, const int32_t *positions, int64_t n_positions, const double *qual_table41,
               int64_t *n_molecules, int64_t *n_calls, Input input, CountPass pass)
{
    DMX_TRY(bind(c));
    if (null_input || !n_molecules || !n_calls || !qual_table41) return fail(DMX_ERR_INVALID, "%s: null argument", who);
    if (c->crs_state != STREAM_NONE) return fail(DMX_ERR_INVALID, "call order: a read-counting stream is open on this context (dmx_count_reads_end first)");
    if (bad_positions(positions, n_positions)) return fail(DMX_ERR_INVALID, "%s: bad positions", who);
    long long n_reads = 0;
    DMX_TRY(input(&n_reads));
    *n_molecules = *n_calls = 0;
    if (n_reads == 0) {
        dmx::host::release_count_reads(c);
        c->cr_molecules = c->cr_calls = 0;
        c->cr_peak_bytes = 0;
        for (double &ms : c->cr_stage_ms) ms = 0.0;
        return 0;
    }
    long long n_m = 0, n_c = 0;
    const int rc = pass(&n_m, &n_c);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_count_reads(c);
        return rc;
    }
    *n_molecules = n_m;
    *n_calls = n_c;
    return 0;
}

// What both push entry points do around the push.  input() looks at arguments that, when they are bad, leave the stream
// open; whatever push() refuses kills it: its carry goes, the records of its earlier pushes stand for nothing.
template <typename Input, typename Push>
int push_once(dmx_ctx *c, const char *who, int final, int64_t *n_molecules, int64_t *n_calls, Input input, Push push)
{
    DMX_TRY(bind(c));
    if (!n_molecules || !n_calls) return fail(DMX_ERR_INVALID, "%s: null argument", who);
    *n_molecules = *n_calls = 0;
    if (c->crs_state == STREAM_NONE) return fail(DMX_ERR_INVALID, "call order: dmx_count_reads_begin before dmx_%s", who);
    if (c->crs_state == STREAM_FINISHED) return fail(DMX_ERR_INVALID, "call order: dmx_%s after the final push", who);
    if (c->crs_state == STREAM_DEAD) return fail(DMX_ERR_INVALID, "call order: a push of this stream failed (dmx_count_reads_end is what is left to do)");
    DMX_TRY(input());
    long long n_m = 0, n_c = 0;
    const int rc = push(&n_m, &n_c);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_count_reads(c);
        dmx::host::release_count_reads_carry(c);
        c->crs_state = STREAM_DEAD;
        return rc;
    }
    if (final) c->crs_state = STREAM_FINISHED;
    *n_molecules = n_m;
    *n_calls = n_c;
    return 0;
}

// the countable set behind a handle
int find_countable(dmx_ctx *c, int64_t handle, const char *who, ResidentReads **set)
{
    DMX_TRY(dmx::host::find_resident_reads(c, handle, who, set));
    if (!(*set)->countable)
        return fail(DMX_ERR_INVALID, "%s: the set was uploaded without compressed_cb / compressed_ub / p_misaligned / alignment_score: it serves coverage only", who);
    return 0;
}

}  // namespace

extern "C" {

int dmx_count_reads(dmx_ctx *c, const dmx_decoded_reads *reads, const int32_t *positions, int64_t n_positions, const double *qual_table41,
                    int64_t *n_molecules, int64_t *n_calls)
{
    return count_once(
        c, "count_reads", !reads, positions, n_positions, qual_table41, n_molecules, n_calls,
        [&](long long *n_reads) {
            *n_reads = reads->n_reads;
            return check_reads(reads, "count_reads", false);
        },
        [&](long long *n_m, long long *n_c) {
            const auto upload_them = [&](Scratch &sc, ReadsView *R) {
                DMX_TRY(upload_reads(sc, host_reads(reads), true, R, c->stream));
                c->reads_upload_bytes += dmx::host::decoded_reads_bytes(reads->n_reads, reads->n_cigar_ops, reads->n_bases, true);
                return 0;
            };
            return count_reads(c, upload_them, positions, n_positions, qual_table41, n_m, n_c);
        });
}

int dmx_count_reads_resident(dmx_ctx *c, int64_t handle, const int32_t *positions, int64_t n_positions, const double *qual_table41,
                             int64_t *n_molecules, int64_t *n_calls)
{
    ResidentReads *set = nullptr;
    return count_once(
        c, "count_reads_resident", false, positions, n_positions, qual_table41, n_molecules, n_calls,
        [&](long long *n_reads) {
            DMX_TRY(find_countable(c, handle, "count_reads_resident", &set));
            *n_reads = set->columns.n;
            return 0;
        },
        [&](long long *n_m, long long *n_c) {
            const auto in_place = [&](Scratch &, ReadsView *R) { return *R = view_of(set->columns, 0, set->columns.n, true), 0; };
            return count_reads(c, in_place, positions, n_positions, qual_table41, n_m, n_c);
        });
}

int dmx_count_reads_begin(dmx_ctx *c, const int32_t *positions, int64_t n_positions, const double *qual_table41)
{
    DMX_TRY(bind(c));
    if (!qual_table41) return fail(DMX_ERR_INVALID, "count_reads_begin: null argument");
    if (c->crs_state != STREAM_NONE) return fail(DMX_ERR_INVALID, "call order: a read-counting stream is open on this context (dmx_count_reads_end first)");
    if (bad_positions(positions, n_positions)) return fail(DMX_ERR_INVALID, "count_reads_begin: bad positions");
    dmx::host::release_count_reads(c);
    const int rc = stream_begin(c, positions, n_positions, qual_table41);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_count_reads_stream(c);
        return rc;
    }
    c->crs_state = STREAM_OPEN;
    return 0;
}

int dmx_count_reads_push(dmx_ctx *c, const dmx_decoded_reads *chunk, int final, int64_t *n_molecules, int64_t *n_calls)
{
    return push_once(
        c, "count_reads_push", final, n_molecules, n_calls, [] { return 0; },
        [&](long long *n_m, long long *n_c) {
            if (chunk) DMX_TRY(check_reads(chunk, "count_reads_push", false));
            return stream_push(c, HostChunk{chunk}, final != 0, n_m, n_c);
        });
}

int dmx_count_reads_push_resident(dmx_ctx *c, int64_t handle, int64_t first_read, int64_t last_read, int final, int64_t *n_molecules,
                                  int64_t *n_calls)
{
    ResidentReads *set = nullptr;
    return push_once(
        c, "count_reads_push_resident", final, n_molecules, n_calls,
        [&] {  // the arguments are looked at before the stream is: a bad handle or range leaves it open
            DMX_TRY(find_countable(c, handle, "count_reads_push_resident", &set));
            if (first_read < 0 || last_read < first_read || last_read > set->columns.n)
                return fail(DMX_ERR_INVALID, "count_reads_push_resident: the range [%lld, %lld) must satisfy 0 <= first_read <= last_read <= %lld reads",
                            (long long)first_read, (long long)last_read, set->columns.n);
            return 0;
        },
        [&](long long *n_m, long long *n_c) { return stream_push(c, ResidentChunk{set, first_read, last_read - first_read}, final != 0, n_m, n_c); });
}

int dmx_count_reads_end(dmx_ctx *c)
{
    DMX_TRY(bind(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    dmx::host::release_count_reads_stream(c);  // (the records of the last push stay for dmx_count_reads_fetch)
    return 0;
}

int dmx_count_reads_fetch(dmx_ctx *c, void *molecules_out, void *snp_calls_out)
{
    DMX_TRY(bind(c));
    if (c->cr_molecules < 0) return fail(DMX_ERR_INVALID, "call order: dmx_count_reads or dmx_count_reads_push before dmx_count_reads_fetch");
    if ((c->cr_molecules && !molecules_out) || (c->cr_calls && !snp_calls_out)) return fail(DMX_ERR_INVALID, "count_reads_fetch: null output");
    if (c->cr_molecules)
        HIP_TRY(hipMemcpyAsync(molecules_out, c->d_cr_molecules.p, (size_t)c->cr_molecules * MOLECULE_BYTES, hipMemcpyDeviceToHost, c->stream));
    if (c->cr_calls)
        HIP_TRY(hipMemcpyAsync(snp_calls_out, c->d_cr_calls.p, (size_t)c->cr_calls * SNP_CALL_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->calls_transfer_bytes[1] += dmx::host::call_record_bytes(c->cr_molecules, c->cr_calls);
    return 0;
}

int dmx_get_count_reads_timings(dmx_ctx *c, double *stage_ms)
{
    DMX_TRY(bind(c));
    if (!stage_ms) return fail(DMX_ERR_INVALID, "null stage_ms");
    if (c->cr_molecules < 0) return fail(DMX_ERR_INVALID, "call order: dmx_count_reads before dmx_get_count_reads_timings");
    for (int s = 0; s < dmx::COUNT_READS_STAGES; s++) stage_ms[s] = c->cr_stage_ms[s];
    return 0;
}

int dmx_get_count_reads_carry(dmx_ctx *c, int64_t *n_reads)
{
    DMX_TRY(bind(c));
    if (!n_reads) return fail(DMX_ERR_INVALID, "null n_reads");
    *n_reads = c->crs_state == STREAM_NONE ? 0 : c->cr_carried;
    return 0;
}

int dmx_get_count_reads_peak_bytes(dmx_ctx *c, int64_t *bytes)
{
    DMX_TRY(bind(c));
    if (!bytes) return fail(DMX_ERR_INVALID, "null bytes");
    if (c->cr_molecules < 0) return fail(DMX_ERR_INVALID, "call order: dmx_count_reads or dmx_count_reads_push before dmx_get_count_reads_peak_bytes");
    *bytes = c->cr_peak_bytes;
    return 0;
}

}  // extern "C"
