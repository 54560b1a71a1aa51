// snp_detect.hip -- scoring and selection of new SNPs from the calls at candidate positions (the compute half of the
// reference's detect_snps_positions, demuxalot/snp_detection.py:78-125, 218-227; include/demux_hip.h "SNP detection"):
//
//   dmx_snp_count   containers + barcode -> donor map  ->  int32 counts[position, donor, base]
//                   kept calls: p_base_wrong < threshold (float32), base_index < 4, barcode assigned;
//                   key (position rank, base, donor, barcode) sorted with rocPRIM, min(run, cap) per key added up
//   dmx_snp_score   counts -> ref / alt bases, base totals, float64 importance[position, donor] (one lane per position)
//   dmx_snp_select  top n per donor (stable descending), overall ranking by numpy's pairwise row sum with the cut of
//                   :223-225, union -> selected position indices, ascending
//
// Positions are numbered in the canonical order: container `chrom` value, then position ascending.  Every ranking
// is stable in that order (ties go to the earlier position).  The state lives in buffers of its own (dmx_ctx::d_sd_*),
// which nothing else reads or writes; dmx_release_problem and dmx_destroy free them.
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device_scratch.h"
#include "pairwise_sum.h"

namespace {

using dmx::host::bind;
using namespace dmx::scratch;

constexpr int SNP_CALL_BYTES = 13, MOLECULE_BYTES = 12;
constexpr int COUNT_CHUNK = 16;  // sorted keys per lane of the count accumulation

// ---------------------------------------------------------------------------------------------------------------
// count
// ---------------------------------------------------------------------------------------------------------------
// One container's records: keep flag, position key (chrom << 32 | biased position) and (base << 30 | barcode).
// bad: 1 = molecule_index outside the molecule table, 2 = compressed_cb outside [0, B).
__global__ __launch_bounds__(256) void k_sd_calls(const unsigned char *__restrict__ snp_calls, long long n,
                                                  const unsigned char *__restrict__ molecules, long long n_molecules, int chrom,
                                                  const int *__restrict__ donor_of_barcode, long long B, float threshold,
                                                  unsigned long long *__restrict__ keep, unsigned long long *__restrict__ pos_key,
                                                  unsigned *__restrict__ base_cb, int *bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char *r = snp_calls + i * SNP_CALL_BYTES;
    int mol, pos;
    float p;
    __builtin_memcpy(&mol, r, 4);
    __builtin_memcpy(&pos, r + 4, 4);
    __builtin_memcpy(&p, r + 9, 4);
    const unsigned base = r[8];
    bool kept = false;
    if (mol < 0 || mol >= n_molecules) {
        atomicOr(bad, 1);
    } else {
        int cb;
        __builtin_memcpy(&cb, molecules + (long long)mol * MOLECULE_BYTES, 4);
        if (cb < 0 || cb >= B) {
            atomicOr(bad, 2);
        } else if (p < threshold && base < 4u && donor_of_barcode[cb] >= 0) {  // NaN fails the comparison, as in numpy
            kept = true;
            pos_key[i] = (unsigned long long)(unsigned)chrom << 32 | (unsigned)(pos ^ (int)0x80000000);
            base_cb[i] = base << 30 | (unsigned)cb;
        }
    }
    keep[i] = kept ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_sd_compact(const unsigned long long *__restrict__ keep, const unsigned long long *__restrict__ at,
                                                    long long n, const unsigned long long *__restrict__ pos_key,
                                                    const unsigned *__restrict__ base_cb, unsigned long long *__restrict__ out_key,
                                                    unsigned *__restrict__ out_base_cb)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const unsigned long long o = at[i] - 1;
    out_key[o] = pos_key[i];
    out_base_cb[o] = base_cb[i];
}

__global__ __launch_bounds__(256) void k_sd_heads(const unsigned long long *__restrict__ sorted, long long n, unsigned long long *__restrict__ head)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_sd_unique(const unsigned long long *__restrict__ sorted, const unsigned long long *__restrict__ head,
                                                   const unsigned long long *__restrict__ at, long long n, unsigned long long *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    out[at[i] - 1] = sorted[i];
}

// key = ((rank << 2 | base) << donor_bits | donor) << barcode_bits | barcode
__global__ __launch_bounds__(256) void k_sd_keys(const unsigned long long *__restrict__ pos_key, const unsigned *__restrict__ base_cb, long long n,
                                                 const unsigned long long *__restrict__ positions, long long P,
                                                 const int *__restrict__ donor_of_barcode, int donor_bits, int barcode_bits,
                                                 unsigned long long *__restrict__ key)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = pos_key[i];
    long long lo = 0, hi = P;  // first position >= k (it is there)
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (positions[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    const unsigned bc = base_cb[i];
    const unsigned cb = bc & 0x3FFFFFFFu;
    const unsigned long long donor = (unsigned)donor_of_barcode[cb];
    key[i] = ((((unsigned long long)lo << 2 | (bc >> 30)) << donor_bits | donor) << barcode_bits) | cb;
}

// Every call whose index within its run of equal keys is below the cap adds one: min(run, cap) per (barcode, position,
// base).  A lane walks COUNT_CHUNK consecutive sorted keys and adds what it found for one (position, base, donor) cell
// with one atomic when the cell changes, so that a position covered by millions of calls is spread over many lanes.
__global__ __launch_bounds__(256) void k_sd_accumulate(const unsigned long long *__restrict__ key, long long n, long long cap, int donor_bits,
                                                       int barcode_bits, int D, int *__restrict__ counts)
{
    const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * COUNT_CHUNK;
    if (i0 >= n) return;
    const long long i1 = i0 + COUNT_CHUNK < n ? i0 + COUNT_CHUNK : n;
    unsigned long long cell = ~0ull;
    int acc = 0;
    for (long long i = i0; i < i1; i++) {
        const unsigned long long k = key[i];
        const int take = (i < cap || key[i - cap] != k) ? 1 : 0;
        const unsigned long long c = k >> barcode_bits;
        if (c != cell) {
            if (acc) {
                const unsigned long long donor = cell & ((1ull << donor_bits) - 1), rb = cell >> donor_bits;
                atomicAdd(counts + ((rb >> 2) * (unsigned long long)D + donor) * 4 + (rb & 3), acc);
            }
            cell = c;
            acc = 0;
        }
        acc += take;
    }
    if (acc) {
        const unsigned long long donor = cell & ((1ull << donor_bits) - 1), rb = cell >> donor_bits;
        atomicAdd(counts + ((rb >> 2) * (unsigned long long)D + donor) * 4 + (rb & 3), acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// score (snp_detection.py:78-97), one lane per position, in the reference's operation order
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sd_score(const int *__restrict__ counts, long long P, int D, double reg,
                                                  double *__restrict__ importance, unsigned char *__restrict__ bases,
                                                  long long *__restrict__ totals)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int *c = counts + p * D * 4;
    long long tot[4] = {0, 0, 0, 0};
    for (int d = 0; d < D; d++)
        for (int b = 0; b < 4; b++) tot[b] += c[d * 4 + b];
    // alt, ref = argsort(totals)[-2:] with a stable ascending sort: ref = largest (total, base), alt = the next
    int ref = 0;
    for (int b = 1; b < 4; b++)
        if (tot[b] >= tot[ref]) ref = b;
    int alt = ref == 0 ? 1 : 0;
    for (int b = alt + 1; b < 4; b++)
        if (b != ref && tot[b] >= tot[alt]) alt = b;
    bases[2 * p] = (unsigned char)ref;
    bases[2 * p + 1] = (unsigned char)alt;
    totals[2 * p] = tot[ref];
    totals[2 * p + 1] = tot[alt];
    // count_0, count_1 = (counts[:, (alt, ref)] + 1e-4).sum(axis=0): row after row
    double s0 = 0.0, s1 = 0.0;
    for (int d = 0; d < D; d++) {
        const double c0 = (double)c[d * 4 + alt] + 1e-4, c1 = (double)c[d * 4 + ref] + 1e-4;
        s0 = d ? s0 + c0 : c0;
        s1 = d ? s1 + c1 : c1;
    }
    const double p_avg = s1 / (s1 + s0);
    for (int d = 0; d < D; d++) {
        const double c0 = (double)c[d * 4 + alt] + 1e-4, c1 = (double)c[d * 4 + ref] + 1e-4;
        const double p1 = (c1 + p_avg * reg) / ((c0 + c1) + reg);
        const double diff = p_avg - p1;
        importance[p * D + d] = diff * diff;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// select (snp_detection.py:218-227)
// ---------------------------------------------------------------------------------------------------------------
// radix key of a descending order of float64 values: larger first, NaN last (where argsort(-x) puts it), -0 == +0
__device__ __forceinline__ unsigned long long descending_key(double x)
{
    if (x != x) return ~0ull;
    const unsigned long long bits = x == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(x);
    const unsigned long long ascending = bits >> 63 ? ~bits : bits | (1ull << 63);
    return ~ascending;
}

// the overall ranking's row sum: np.sum of a row of importances, bit for bit, for every n_donors up to MAX_DONORS (pairwise_sum.h)
using dmx::rowsum::MAX_DONORS;

// column-major keys of the per-donor rankings: entry d * P + p
__global__ __launch_bounds__(256) void k_sd_donor_keys(const double *__restrict__ importance, long long P, int D,
                                                       unsigned long long *__restrict__ key, unsigned *__restrict__ idx)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P * D) return;
    const long long d = j / P, p = j - d * P;
    key[j] = descending_key(importance[p * D + d]);
    idx[j] = (unsigned)j;
}

__global__ __launch_bounds__(256) void k_sd_donor_of(const unsigned *__restrict__ idx, long long n, long long P, unsigned *__restrict__ donor)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    donor[j] = (unsigned)(idx[j] / P);
}

// after the two stable sorts every donor's segment lists its positions best first: the first n_best are members
__global__ __launch_bounds__(256) void k_sd_members(const unsigned *__restrict__ idx, long long P, int D, long long n_best,
                                                    unsigned char *__restrict__ member)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P * D) return;
    if (j % P < n_best) member[idx[j] % P] = 1;
}

__global__ __launch_bounds__(256) void k_sd_row_keys(const double *__restrict__ importance, long long P, int D,
                                                     unsigned long long *__restrict__ key, unsigned *__restrict__ idx)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    key[p] = descending_key(dmx::rowsum::pairwise_sum(importance + p * D, D));
    idx[p] = (unsigned)p;
}

__global__ __launch_bounds__(256) void k_sd_new_flags(const unsigned *__restrict__ order, long long P, const unsigned char *__restrict__ member,
                                                      unsigned long long *__restrict__ is_new)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    is_new[k] = member[order[k]] ? 0ull : 1ull;
}

// best_snps_overall[:searchsorted(cumsum(is_new), n_add, side='right')]: the ranking up to the (n_add + 1)-th new
// position, exclusive (cut stays P when there are not that many)
__global__ __launch_bounds__(256) void k_sd_cut(const unsigned long long *__restrict__ is_new, const unsigned long long *__restrict__ cum,
                                                long long P, long long n_add, long long *__restrict__ cut)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    if (is_new[k] && (long long)cum[k] == n_add + 1) *cut = k;
}

__global__ __launch_bounds__(256) void k_sd_mark_overall(const unsigned *__restrict__ order, long long P, const long long *__restrict__ cut,
                                                         unsigned char *__restrict__ member)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P || k >= *cut) return;
    member[order[k]] = 1;
}

__global__ __launch_bounds__(256) void k_sd_flags(const unsigned char *__restrict__ member, long long P, unsigned long long *__restrict__ flag)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    flag[p] = member[p] ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_sd_gather(const unsigned char *__restrict__ member, const unsigned long long *__restrict__ at, long long P,
                                                   long long *__restrict__ selected)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !member[p]) return;
    selected[at[p] - 1] = p;
}

// on_device: the parts' pointers are device memory already (views of resident call sets): nothing of them is uploaded
int snp_count(dmx_ctx *c, const dmx_call_container *parts, int n_parts, bool on_device, const int32_t *donor_of_barcode, long long B, int D,
              float threshold, long long cap, long long *n_positions)
{
    hipStream_t st = c->stream;
    dmx::host::release_snp_detection(c);
    Scratch sc(c);
    long long n = 0;
    for (int k = 0; k < n_parts; k++) {
        if (parts[k].n_snp_calls < 0 || parts[k].n_molecules < 0) return fail(DMX_ERR_INVALID, "negative container sizes");
        if (parts[k].chrom < 0) return fail(DMX_ERR_INVALID, "container chrom must be >= 0");
        if ((parts[k].n_snp_calls && !parts[k].snp_calls) || (parts[k].n_molecules && !parts[k].molecules))
            return fail(DMX_ERR_INVALID, "null container records");
        n += parts[k].n_snp_calls;
    }
    int *d_donor = nullptr, *bad = nullptr;
    DMX_TRY(upload(sc, &d_donor, donor_of_barcode, (size_t)B, st));
    DMX_TRY(sc.get(&bad, 1));
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
    unsigned long long *keep, *pos_key;
    unsigned *base_cb;
    DMX_TRY(sc.get(&keep, (size_t)n));
    DMX_TRY(sc.get(&pos_key, (size_t)n));
    DMX_TRY(sc.get(&base_cb, (size_t)n));
    long long at = 0;
    for (int k = 0; k < n_parts; k++) {
        const dmx_call_container &part = parts[k];
        if (part.n_snp_calls == 0) continue;
        const unsigned char *d_calls = (const unsigned char *)part.snp_calls, *d_molecules = (const unsigned char *)part.molecules;
        if (!on_device) {
            unsigned char *up_calls, *up_molecules;
            DMX_TRY(upload(sc, &up_calls, d_calls, (size_t)part.n_snp_calls * SNP_CALL_BYTES, st));
            DMX_TRY(upload(sc, &up_molecules, d_molecules, (size_t)part.n_molecules * MOLECULE_BYTES, st));
            d_calls = up_calls, d_molecules = up_molecules;
            c->calls_transfer_bytes[0] += dmx::host::call_record_bytes(part.n_molecules, part.n_snp_calls);
        }
        hipLaunchKernelGGL(k_sd_calls, dim3(grid_for(part.n_snp_calls)), dim3(256), 0, st, d_calls, part.n_snp_calls, d_molecules,
                           part.n_molecules, part.chrom, d_donor, B, threshold, keep + at, pos_key + at, base_cb + at, bad);
        DMX_TRY(launched("k_sd_calls"));
        at += part.n_snp_calls;
    }
    int h_bad = 0;
    HIP_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // also: the caller's buffers are free to change from here on
    if (h_bad & 1) return fail(DMX_ERR_INVALID, "molecule_index outside the molecule table");
    if (h_bad & 2) return fail(DMX_ERR_INVALID, "compressed_cb outside [0, n_barcodes)");

    // kept calls, compacted in input order
    unsigned long long *at_keep, m = 0;
    DMX_TRY(sc.get(&at_keep, (size_t)n));
    DMX_TRY(sum_scan(sc, keep, at_keep, (size_t)n, &m, st));
    unsigned long long *kept_key, *sorted;
    unsigned *kept_base_cb;
    DMX_TRY(sc.get(&kept_key, (size_t)m));
    DMX_TRY(sc.get(&kept_base_cb, (size_t)m));
    DMX_TRY(sc.get(&sorted, (size_t)m));
    if (n) hipLaunchKernelGGL(k_sd_compact, dim3(grid_for(n)), dim3(256), 0, st, keep, at_keep, n, pos_key, base_cb, kept_key, kept_base_cb);
    DMX_TRY(launched("k_sd_compact"));

    // distinct positions, canonical order
    DMX_TRY(sort_keys(sc, kept_key, sorted, (size_t)m, 64u, st));
    unsigned long long *head, *at_head, P = 0;
    DMX_TRY(sc.get(&head, (size_t)m));
    DMX_TRY(sc.get(&at_head, (size_t)m));
    if (m) hipLaunchKernelGGL(k_sd_heads, dim3(grid_for(m)), dim3(256), 0, st, sorted, (long long)m, head);
    DMX_TRY(launched("k_sd_heads"));
    DMX_TRY(sum_scan(sc, head, at_head, (size_t)m, &P, st));
    const int donor_bits = bits_for((unsigned long long)D), barcode_bits = bits_for((unsigned long long)B);
    const int key_bits = bits_for(P) + 2 + donor_bits + barcode_bits;
    if (key_bits > 64) return fail(DMX_ERR_UNSUPPORTED, "%llu positions x %d donors x %lld barcodes do not fit a 64-bit key", P, D, B);
    DMX_TRY(dev_alloc(c, c->d_sd_pos, (size_t)P));
    DMX_TRY(dev_alloc(c, c->d_sd_counts, (size_t)P * D * 4));
    if (m) hipLaunchKernelGGL(k_sd_unique, dim3(grid_for(m)), dim3(256), 0, st, sorted, head, at_head, (long long)m, c->d_sd_pos.p);
    DMX_TRY(launched("k_sd_unique"));
    HIP_TRY(hipMemsetAsync(c->d_sd_counts.p, 0, dev_bytes(c->d_sd_counts), st));

    // (position, base, donor, barcode) keys, sorted: runs of one barcode at one position and base
    if (m) {
        unsigned long long *key = head, *key_sorted = at_head;  // (their contents are no longer needed)
        hipLaunchKernelGGL(k_sd_keys, dim3(grid_for(m)), dim3(256), 0, st, kept_key, kept_base_cb, (long long)m, c->d_sd_pos.p,
                           (long long)P, d_donor, donor_bits, barcode_bits, key);
        DMX_TRY(launched("k_sd_keys"));
        DMX_TRY(sort_keys(sc, key, key_sorted, (size_t)m, (unsigned)key_bits, st));
        hipLaunchKernelGGL(k_sd_accumulate, dim3(grid_for(((long long)m + COUNT_CHUNK - 1) / COUNT_CHUNK)), dim3(256), 0, st, key_sorted,
                           (long long)m, cap, donor_bits, barcode_bits, D, c->d_sd_counts.p);
        DMX_TRY(launched("k_sd_accumulate"));
    }
    HIP_TRY(hipStreamSynchronize(st));
    c->sd_P = (long long)P;
    c->sd_D = D;
    *n_positions = (int64_t)P;
    return 0;
}

}  // namespace

extern "C" {

// what dmx_snp_count and dmx_snp_count_device share: the arguments, the pass, its clean-up
static int snp_count_entry(dmx_ctx *c, const dmx_call_container *containers, int32_t n_containers, bool on_device, const int32_t *donor_of_barcode,
                           int64_t n_barcodes, int32_t n_donors, float p_threshold, int32_t cap, int64_t *n_positions)
{
    DMX_TRY(bind(c));
    if (n_containers < 0 || (n_containers && !containers)) return fail(DMX_ERR_INVALID, "bad container list");
    if (n_barcodes < 0 || (n_barcodes && !donor_of_barcode)) return fail(DMX_ERR_INVALID, "bad donor_of_barcode");
    if (n_barcodes >= (1ll << 30)) return fail(DMX_ERR_UNSUPPORTED, "at most 2^30 barcodes");
    if (n_donors < 1 || n_donors > MAX_DONORS) return fail(DMX_ERR_INVALID, "n_donors must be 1..%d", MAX_DONORS);
    if (cap < 0) return fail(DMX_ERR_INVALID, "cap must be >= 0");
    if (!n_positions) return fail(DMX_ERR_INVALID, "null n_positions");
    for (int64_t b = 0; b < n_barcodes; b++)
        if (donor_of_barcode[b] < -1 || donor_of_barcode[b] >= n_donors) return fail(DMX_ERR_INVALID, "donor_of_barcode[%lld] out of range", (long long)b);
    long long P = 0;
    if (on_device) DMX_TRY(dmx::host::check_device_containers(c, containers, n_containers, "snp_count_device"));
    const int rc = snp_count(c, containers, n_containers, on_device, donor_of_barcode, n_barcodes, n_donors, p_threshold, cap, &P);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_snp_detection(c);
        return rc;
    }
    *n_positions = P;
    return 0;
}

int dmx_snp_count(dmx_ctx *c, const dmx_call_container *containers, int32_t n_containers, const int32_t *donor_of_barcode,
                  int64_t n_barcodes, int32_t n_donors, float p_threshold, int32_t cap, int64_t *n_positions)
{
    return snp_count_entry(c, containers, n_containers, false, donor_of_barcode, n_barcodes, n_donors, p_threshold, cap, n_positions);
}

int dmx_snp_count_device(dmx_ctx *c, const dmx_call_container *views, int32_t n_views, const int32_t *donor_of_barcode,
                         int64_t n_barcodes, int32_t n_donors, float p_threshold, int32_t cap, int64_t *n_positions)
{
    return snp_count_entry(c, views, n_views, true, donor_of_barcode, n_barcodes, n_donors, p_threshold, cap, n_positions);
}

int dmx_snp_score(dmx_ctx *c, double regularization, int32_t *chrom, int32_t *pos, int32_t *counts, double *importances,
                  uint8_t *bases, int64_t *base_totals)
{
    DMX_TRY(bind(c));
    if (c->sd_P < 0) return fail(DMX_ERR_INVALID, "call order: dmx_snp_count before dmx_snp_score");
    hipStream_t st = c->stream;
    const long long P = c->sd_P;
    const int D = c->sd_D;
    dev_free(c, c->d_sd_imp);
    c->sd_scored = false;
    DMX_TRY(dev_alloc(c, c->d_sd_imp, (size_t)P * D));
    Scratch sc(c);
    unsigned char *d_bases;
    long long *d_totals;
    DMX_TRY(sc.get(&d_bases, (size_t)P * 2));
    DMX_TRY(sc.get(&d_totals, (size_t)P * 2));
    if (P) hipLaunchKernelGGL(k_sd_score, dim3(grid_for(P)), dim3(256), 0, st, c->d_sd_counts.p, P, D, regularization, c->d_sd_imp.p,
                              d_bases, d_totals);
    DMX_TRY(launched("k_sd_score"));
    std::vector<unsigned long long> keys;
    if (chrom || pos) {
        keys.resize((size_t)P);
        if (P) HIP_TRY(hipMemcpyAsync(keys.data(), c->d_sd_pos.p, (size_t)P * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    if (counts && P) HIP_TRY(hipMemcpyAsync(counts, c->d_sd_counts.p, (size_t)P * D * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (importances && P) HIP_TRY(hipMemcpyAsync(importances, c->d_sd_imp.p, (size_t)P * D * sizeof(double), hipMemcpyDeviceToHost, st));
    if (bases && P) HIP_TRY(hipMemcpyAsync(bases, d_bases, (size_t)P * 2, hipMemcpyDeviceToHost, st));
    if (base_totals && P) HIP_TRY(hipMemcpyAsync(base_totals, d_totals, (size_t)P * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (long long p = 0; p < (long long)keys.size(); p++) {
        if (chrom) chrom[p] = (int32_t)(keys[p] >> 32);
        if (pos) pos[p] = (int32_t)((unsigned)keys[p] ^ 0x80000000u);
    }
    c->sd_scored = true;
    return 0;
}

int dmx_snp_select(dmx_ctx *c, int64_t n_best_per_donor, int64_t n_additional, int64_t *selected, int64_t *n_selected)
{
    DMX_TRY(bind(c));
    if (!c->sd_scored) return fail(DMX_ERR_INVALID, "call order: dmx_snp_score before dmx_snp_select");
    if (n_best_per_donor < 0 || n_additional < 0) return fail(DMX_ERR_INVALID, "n_best_per_donor and n_additional must be >= 0");
    if (!n_selected) return fail(DMX_ERR_INVALID, "null n_selected");
    hipStream_t st = c->stream;
    const long long P = c->sd_P, PD = P * c->sd_D;
    const int D = c->sd_D;
    *n_selected = 0;
    if (P == 0) return 0;
    if (PD >= (1ll << 32)) return fail(DMX_ERR_UNSUPPORTED, "positions x donors must stay below 2^32");
    Scratch sc(c);
    unsigned char *member;
    DMX_TRY(sc.get(&member, (size_t)P));
    HIP_TRY(hipMemsetAsync(member, 0, (size_t)P, st));
    // per donor: argsort(-importances, axis=0)[:n_best], stable (a sort on the value, then a stable one on the donor)
    if (n_best_per_donor > 0) {
        unsigned long long *key, *key_sorted;
        unsigned *idx, *idx_sorted, *donor, *donor_sorted;
        DMX_TRY(sc.get(&key, (size_t)PD));
        DMX_TRY(sc.get(&key_sorted, (size_t)PD));
        DMX_TRY(sc.get(&idx, (size_t)PD));
        DMX_TRY(sc.get(&idx_sorted, (size_t)PD));
        DMX_TRY(sc.get(&donor, (size_t)PD));
        DMX_TRY(sc.get(&donor_sorted, (size_t)PD));
        hipLaunchKernelGGL(k_sd_donor_keys, dim3(grid_for(PD)), dim3(256), 0, st, c->d_sd_imp.p, P, D, key, idx);
        DMX_TRY(launched("k_sd_donor_keys"));
        DMX_TRY(sort_pairs(sc, key, key_sorted, idx, idx_sorted, (size_t)PD, 64u, st));
        hipLaunchKernelGGL(k_sd_donor_of, dim3(grid_for(PD)), dim3(256), 0, st, idx_sorted, PD, P, donor);
        DMX_TRY(launched("k_sd_donor_of"));
        DMX_TRY(sort_pairs(sc, donor, donor_sorted, idx_sorted, idx, (size_t)PD, (unsigned)std::max(1, bits_for((unsigned long long)D)), st));
        hipLaunchKernelGGL(k_sd_members, dim3(grid_for(PD)), dim3(256), 0, st, idx, P, D, (long long)n_best_per_donor, member);
        DMX_TRY(launched("k_sd_members"));
    }
    // overall: argsort(-importances.sum(axis=1)), stable, cut after n_additional positions that are not members yet
    unsigned long long *row_key, *row_key_sorted, *is_new, *cum, *flag, *at;
    unsigned *order_in, *order;
    long long *cut, *d_selected;
    DMX_TRY(sc.get(&row_key, (size_t)P));
    DMX_TRY(sc.get(&row_key_sorted, (size_t)P));
    DMX_TRY(sc.get(&order_in, (size_t)P));
    DMX_TRY(sc.get(&order, (size_t)P));
    DMX_TRY(sc.get(&is_new, (size_t)P));
    DMX_TRY(sc.get(&cum, (size_t)P));
    DMX_TRY(sc.get(&flag, (size_t)P));
    DMX_TRY(sc.get(&at, (size_t)P));
    DMX_TRY(sc.get(&cut, 1));
    DMX_TRY(sc.get(&d_selected, (size_t)P));
    hipLaunchKernelGGL(k_sd_row_keys, dim3(grid_for(P)), dim3(256), 0, st, c->d_sd_imp.p, P, D, row_key, order_in);
    DMX_TRY(launched("k_sd_row_keys"));
    DMX_TRY(sort_pairs(sc, row_key, row_key_sorted, order_in, order, (size_t)P, 64u, st));
    hipLaunchKernelGGL(k_sd_new_flags, dim3(grid_for(P)), dim3(256), 0, st, order, P, member, is_new);
    DMX_TRY(launched("k_sd_new_flags"));
    unsigned long long n_new = 0;
    DMX_TRY(sum_scan(sc, is_new, cum, (size_t)P, &n_new, st));
    HIP_TRY(hipMemcpyAsync(cut, &P, sizeof(long long), hipMemcpyHostToDevice, st));
    if ((unsigned long long)n_additional < n_new) {
        hipLaunchKernelGGL(k_sd_cut, dim3(grid_for(P)), dim3(256), 0, st, is_new, cum, P, (long long)n_additional, cut);
        DMX_TRY(launched("k_sd_cut"));
    }
    hipLaunchKernelGGL(k_sd_mark_overall, dim3(grid_for(P)), dim3(256), 0, st, order, P, cut, member);
    DMX_TRY(launched("k_sd_mark_overall"));
    // union, ascending
    hipLaunchKernelGGL(k_sd_flags, dim3(grid_for(P)), dim3(256), 0, st, member, P, flag);
    DMX_TRY(launched("k_sd_flags"));
    unsigned long long n_sel = 0;
    DMX_TRY(sum_scan(sc, flag, at, (size_t)P, &n_sel, st));
    hipLaunchKernelGGL(k_sd_gather, dim3(grid_for(P)), dim3(256), 0, st, member, at, P, d_selected);
    DMX_TRY(launched("k_sd_gather"));
    if (selected && n_sel) HIP_TRY(hipMemcpyAsync(selected, d_selected, (size_t)n_sel * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_selected = (int64_t)n_sel;
    return 0;
}

}  // extern "C"
