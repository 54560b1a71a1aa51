// resident_reads.hip -- resident read sets: the arrays of one dmx_decoded_reads uploaded once into buffers of the context and
// named by a handle (include/demux_hip_debug.h "Resident reads"; the contract: DESIGN.md "Resident reads").
//
//   ingest   one lane per read walks its CIGAR to reference_end (start + the operations 0, 2, 3, 7, 8: the rule both walkers
//            share), behind a bounds check of the read's CIGAR range; a reduction gives the largest end (dmx_reads_info)
//
// The passes that read a set live with their kernels: dmx_count_reads_resident and dmx_count_reads_push_resident in
// count_reads.hip, dmx_coverage_count_resident in coverage.hip.  They take a ReadsView of these buffers (read_columns.h): no copy.
// Whether a read is valid stays their decision; the upload refuses only what the host-array calls refuse before they upload.
#include <atomic>
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

// handles are unique in the process: one context's handle is never valid on another
std::atomic<int64_t> g_next_handle{1};

// A read whose CIGAR range does not lie inside the array ends where it starts (the passes flag it: nothing is read out of bounds).
__global__ __launch_bounds__(256) void k_rr_ends(const int *__restrict__ start, const long long *__restrict__ cigar_begin,
                                                 const int *__restrict__ n_cigar, const unsigned *__restrict__ cigar, long long n,
                                                 long long n_ops, long long *__restrict__ end)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long c0 = cigar_begin[i];
    long long nc = n_cigar[i];
    if (outside(c0, nc, n_ops)) nc = 0;
    long long ref = start[i];
    for (long long k = 0; k < nc; k++) {
        const unsigned c = cigar[c0 + k];
        const unsigned op = c & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref += (long long)(c >> 4);
    }
    end[i] = ref;
}

int reads_upload(dmx_ctx *c, const dmx_decoded_reads *h, ResidentReads &set)
{
    hipStream_t st = c->stream;
    const size_t n = (size_t)h->n_reads;
    const HostReads host = host_reads(h);
    set.countable = n == 0 || (h->compressed_cb && h->compressed_ub && h->p_misaligned && h->alignment_score);
    const int rc = alloc_read_columns(c, set.columns, host, set.countable);
    set.bytes = (int64_t)read_columns_bytes(set.columns);
    DMX_TRY(rc);
    DMX_TRY(copy_in(out_of(set.columns), host, set.countable, st));
    // ---- ingest: the largest reference_end
    long long top = 0;
    if (n) {
        Scratch sc(c);
        long long *end, *d_top;
        DMX_TRY(sc.get(&end, n));
        DMX_TRY(sc.get(&d_top, 1));
        hipLaunchKernelGGL(k_rr_ends, dim3(grid_for((long long)n)), dim3(256), 0, st, set.columns.start.p, set.columns.cigar_begin.p, set.columns.n_cigar.p,
                           set.columns.cigar.p, (long long)n, set.columns.n_ops, end);
        DMX_TRY(launched("k_rr_ends"));
        DMX_TRY(reduce(sc, end, d_top, (long long)LLONG_MIN, n, rocprim::maximum<long long>(), st));
        HIP_TRY(hipMemcpyAsync(&top, d_top, sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's arrays are free to change from here on)
    set.reference_length = top;
    c->reads_upload_bytes += dmx::host::decoded_reads_bytes(h->n_reads, h->n_cigar_ops, h->n_bases, set.countable && n);
    return 0;
}

}  // namespace

extern "C" {

int dmx_reads_upload(dmx_ctx *c, const dmx_decoded_reads *reads, int64_t *handle)
{
    DMX_TRY(bind(c));
    if (!reads || !handle) return fail(DMX_ERR_INVALID, "reads_upload: null argument");
    *handle = 0;
    DMX_TRY(check_reads(reads, "reads_upload", true));
    ResidentReads set;
    const int rc = reads_upload(c, reads, set);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_resident_reads(c, set);
        return rc;
    }
    const int64_t h = g_next_handle.fetch_add(1);
    c->resident_reads[h] = set;
    *handle = h;
    return 0;
}

int dmx_reads_release(dmx_ctx *c, int64_t handle)
{
    DMX_TRY(bind(c));
    ResidentReads *set = nullptr;
    DMX_TRY(dmx::host::find_resident_reads(c, handle, "reads_release", &set));
    HIP_TRY(hipStreamSynchronize(c->stream));
    dmx::host::release_resident_reads(c, *set);
    c->resident_reads.erase(handle);
    return 0;
}

int dmx_reads_info(dmx_ctx *c, int64_t handle, int64_t *info)
{
    DMX_TRY(bind(c));
    if (!info) return fail(DMX_ERR_INVALID, "reads_info: null info");
    ResidentReads *set = nullptr;
    DMX_TRY(dmx::host::find_resident_reads(c, handle, "reads_info", &set));
    info[0] = set->columns.n;
    info[1] = set->columns.n_ops;
    info[2] = set->columns.n_bases;
    info[3] = set->bytes;
    info[4] = set->reference_length;
    return 0;
}

int dmx_get_reads_upload_bytes(dmx_ctx *c, int64_t *bytes)
{
    DMX_TRY(bind(c));
    if (!bytes) return fail(DMX_ERR_INVALID, "null bytes");
    *bytes = c->reads_upload_bytes;
    return 0;
}

}  // extern "C"
