// resident_calls.hip -- resident call sets: the two record arrays of one CompressedSNPCalls (one chromosome) in blocks of the
// context, named by a handle (include/demux_hip_debug.h "Resident calls"; the contract: DESIGN.md "Resident calls").  The records
// are bytewise the host records (12-byte molecules, 13-byte snp_calls, unaligned), so the consumers are the kernels that take
// uploaded containers apart: k_flatten_container (repack_device.hip) through dmx_stage_device_containers, k_sd_calls
// (snp_detect.hip) through dmx_snp_count_device.
//
//   upload       the two arrays copied, one lane per call checks its molecule_index
//   append       the records of the last count or push (dmx_ctx::d_cr_*), device to device, into blocks that grow by doubling
//   concatenate  the parts' molecules behind one another, one lane per call adds the molecules before its part
//   counts       molecules and calls per compressed_cb, integer atomics
//
// A set is open while it is filled and read-only once sealed: every kernel here and every consumer takes it through const pointers.
#include <atomic>
#include <climits>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "device_scratch.h"
#include "dmx_host.h"

namespace {

using dmx::host::bind;
using dmx::host::call_record_bytes;
using dmx::host::find_resident_calls;
using namespace dmx::scratch;

constexpr int SNP_CALL_BYTES = 13, MOLECULE_BYTES = 12;
enum { BAD_MOLECULE = 1, BAD_BARCODE = 2 };

// handles are unique in the process: one context's handle is never valid on another
std::atomic<int64_t> g_next_handle{1};

__global__ __launch_bounds__(256) void k_rc_check(const unsigned char *__restrict__ snp_calls, long long n, long long n_molecules, int *bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int mol;
    __builtin_memcpy(&mol, snp_calls + i * SNP_CALL_BYTES, 4);
    if (mol < 0 || mol >= n_molecules) atomicOr(bad, BAD_MOLECULE);
}

// out[i] = in[i] with molecule_index + shift (the record's other nine bytes as they are)
__global__ __launch_bounds__(256) void k_rc_shift(const unsigned char *__restrict__ in, long long n, int shift, unsigned char *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char *r = in + i * SNP_CALL_BYTES;
    unsigned char *w = out + i * SNP_CALL_BYTES;
    int mol;
    __builtin_memcpy(&mol, r, 4);
    mol += shift;
    __builtin_memcpy(w, &mol, 4);
    for (int b = 4; b < SNP_CALL_BYTES; b++) w[b] = r[b];
}

__global__ __launch_bounds__(256) void k_rc_molecules_per_barcode(const unsigned char *__restrict__ molecules, long long n_molecules, long long B,
                                                                  ull *__restrict__ count, int *bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_molecules) return;
    int cb;
    __builtin_memcpy(&cb, molecules + i * MOLECULE_BYTES, 4);
    if (cb < 0 || cb >= B)
        atomicOr(bad, BAD_BARCODE);
    else
        atomicAdd(count + cb, 1ull);
}

__global__ __launch_bounds__(256) void k_rc_calls_per_barcode(const unsigned char *__restrict__ snp_calls, long long n,
                                                              const unsigned char *__restrict__ molecules, long long n_molecules, long long B,
                                                              ull *__restrict__ count, int *bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int mol, cb;
    __builtin_memcpy(&mol, snp_calls + i * SNP_CALL_BYTES, 4);
    if (mol < 0 || mol >= n_molecules) {
        atomicOr(bad, BAD_MOLECULE);
        return;
    }
    __builtin_memcpy(&cb, molecules + (long long)mol * MOLECULE_BYTES, 4);
    if (cb < 0 || cb >= B)
        atomicOr(bad, BAD_BARCODE);
    else
        atomicAdd(count + cb, 1ull);
}

// room for n_molecules / n_calls records at least; what the set holds is kept (copied device to device on the ctx stream: the
// old blocks go back to the context's cache, whose re-use is ordered on the same stream).  Growth doubles: appends are amortised.
int reserve_block(dmx_ctx *c, unsigned char *&block, long long &cap, long long held, long long wanted, int record_bytes, bool exact)
{
    if (wanted <= cap) return 0;
    const long long room = exact ? wanted : std::max(wanted, 2 * cap);
    unsigned char *grown = nullptr;
    DMX_TRY(ctx_malloc(c, (void **)&grown, (size_t)room * record_bytes));
    if (held) {
        const hipError_t e = hipMemcpyAsync(grown, block, (size_t)held * record_bytes, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) {
            ctx_free(c, grown);
            return fail(DMX_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
        }
    }
    ctx_free(c, block);
    block = grown;
    cap = room;
    return 0;
}

int reserve(dmx_ctx *c, ResidentCalls &set, long long n_molecules, long long n_calls, bool exact)
{
    DMX_TRY(reserve_block(c, set.molecules, set.cap_molecules, set.n_molecules, n_molecules, MOLECULE_BYTES, exact));
    return reserve_block(c, set.calls, set.cap_calls, set.n_calls, n_calls, SNP_CALL_BYTES, exact);
}

int64_t held_bytes(const ResidentCalls &set) { return call_record_bytes(set.cap_molecules, set.cap_calls); }

int find_sealed(dmx_ctx *c, int64_t handle, const char *who, ResidentCalls **set)
{
    DMX_TRY(find_resident_calls(c, handle, who, set));
    if (!(*set)->sealed) return fail(DMX_ERR_INVALID, "%s: the set %lld is still open (dmx_calls_seal first)", who, (long long)handle);
    return 0;
}

int64_t install(dmx_ctx *c, const ResidentCalls &set)
{
    const int64_t h = g_next_handle.fetch_add(1);
    c->resident_calls[h] = set;
    return h;
}

// what dmx_stage_containers asks of a container (container 0), and what it leaves to the upload of records it never copies
int check_host_container(const dmx_call_container *p)
{
    if (p->n_snp_calls < 0 || p->n_molecules < 0) return fail(DMX_ERR_INVALID, "container 0: negative size");
    if (p->n_snp_calls > 0 && (!p->snp_calls || !p->molecules || p->n_molecules == 0))
        return fail(DMX_ERR_INVALID, "container 0: calls without a molecule table");
    if (p->n_molecules > 0 && !p->molecules) return fail(DMX_ERR_INVALID, "container 0: null molecule records");
    if (p->n_molecules > INT_MAX) return fail(DMX_ERR_UNSUPPORTED, "at most 2^31 - 1 molecules in a call set");
    return 0;
}

int calls_upload(dmx_ctx *c, const dmx_call_container *h, ResidentCalls &set)
{
    hipStream_t st = c->stream;
    DMX_TRY(reserve(c, set, h->n_molecules, h->n_snp_calls, true));
    if (h->n_molecules) HIP_TRY(hipMemcpyAsync(set.molecules, h->molecules, (size_t)h->n_molecules * MOLECULE_BYTES, hipMemcpyHostToDevice, st));
    if (h->n_snp_calls) HIP_TRY(hipMemcpyAsync(set.calls, h->snp_calls, (size_t)h->n_snp_calls * SNP_CALL_BYTES, hipMemcpyHostToDevice, st));
    set.n_molecules = h->n_molecules;
    set.n_calls = h->n_snp_calls;
    c->calls_transfer_bytes[0] += call_record_bytes(h->n_molecules, h->n_snp_calls);
    int h_bad = 0;
    if (h->n_snp_calls) {
        Scratch sc(c);
        int *bad;
        DMX_TRY(sc.get(&bad, 1));
        HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_rc_check, dim3(grid_for(set.n_calls)), dim3(256), 0, st, (const unsigned char *)set.calls, set.n_calls, set.n_molecules, bad);
        DMX_TRY(launched("k_rc_check"));
        HIP_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's arrays are free to change from here on)
    if (h_bad) return fail(DMX_ERR_INVALID, "molecule_index outside the molecule table");
    set.sealed = true;
    return 0;
}

int calls_concatenate(dmx_ctx *c, const std::vector<ResidentCalls *> &parts, ResidentCalls &out)
{
    hipStream_t st = c->stream;
    long long n_molecules = 0, n_calls = 0;
    for (const ResidentCalls *part : parts) {
        n_molecules += part->n_molecules;
        n_calls += part->n_calls;
        if (n_molecules > INT_MAX) return fail(DMX_ERR_UNSUPPORTED, "calls_concatenate: 2^31 molecules or more (molecule_index is an int32)");
    }
    DMX_TRY(reserve(c, out, n_molecules, n_calls, true));
    long long at_molecule = 0, at_call = 0;
    for (const ResidentCalls *part : parts) {
        const unsigned char *molecules = part->molecules, *calls = part->calls;
        if (part->n_molecules)
            HIP_TRY(hipMemcpyAsync(out.molecules + at_molecule * MOLECULE_BYTES, molecules, (size_t)part->n_molecules * MOLECULE_BYTES,
                                   hipMemcpyDeviceToDevice, st));
        if (part->n_calls) {
            hipLaunchKernelGGL(k_rc_shift, dim3(grid_for(part->n_calls)), dim3(256), 0, st, calls, part->n_calls, (int)at_molecule,
                               out.calls + at_call * SNP_CALL_BYTES);
            DMX_TRY(launched("k_rc_shift"));
        }
        at_molecule += part->n_molecules;
        at_call += part->n_calls;
    }
    HIP_TRY(hipStreamSynchronize(st));
    out.n_molecules = n_molecules;
    out.n_calls = n_calls;
    out.sealed = true;
    return 0;
}

int barcode_counts(dmx_ctx *c, const ResidentCalls &set, long long B, int64_t *calls_per_barcode, int64_t *molecules_per_barcode)
{
    hipStream_t st = c->stream;
    Scratch sc(c);
    ull *d_calls, *d_molecules;
    int *bad, h_bad = 0;
    DMX_TRY(sc.get(&d_calls, (size_t)B));
    DMX_TRY(sc.get(&d_molecules, (size_t)B));
    DMX_TRY(sc.get(&bad, 1));
    HIP_TRY(hipMemsetAsync(d_calls, 0, sizeof(ull) * (size_t)std::max(1ll, B), st));
    HIP_TRY(hipMemsetAsync(d_molecules, 0, sizeof(ull) * (size_t)std::max(1ll, B), st));
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
    const unsigned char *molecules = set.molecules, *calls = set.calls;
    if (set.n_molecules) {
        hipLaunchKernelGGL(k_rc_molecules_per_barcode, dim3(grid_for(set.n_molecules)), dim3(256), 0, st, molecules, set.n_molecules, B, d_molecules, bad);
        DMX_TRY(launched("k_rc_molecules_per_barcode"));
    }
    if (set.n_calls) {
        hipLaunchKernelGGL(k_rc_calls_per_barcode, dim3(grid_for(set.n_calls)), dim3(256), 0, st, calls, set.n_calls, molecules, set.n_molecules, B,
                           d_calls, bad);
        DMX_TRY(launched("k_rc_calls_per_barcode"));
    }
    HIP_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    if (B) {
        static_assert(sizeof(ull) == sizeof(int64_t), "");
        HIP_TRY(hipMemcpyAsync(calls_per_barcode, d_calls, sizeof(ull) * (size_t)B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(molecules_per_barcode, d_molecules, sizeof(ull) * (size_t)B, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (h_bad & BAD_MOLECULE) return fail(DMX_ERR_INVALID, "molecule_index outside the molecule table");
    if (h_bad & BAD_BARCODE) return fail(DMX_ERR_INVALID, "compressed_cb outside [0, n_barcodes)");
    return 0;
}

// [p, p + bytes) is device memory of `device`, inside one allocation
int check_device_range(int device, const void *p, size_t bytes, const char *who, int k, const char *what)
{
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device) {
        (void)hipGetLastError();
        return fail(DMX_ERR_INVALID, "%s: %s of container %d is not device memory of device %d", who, what, k, device);
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
    if (e != hipSuccess || (const char *)p + bytes > (const char *)base + size) {
        (void)hipGetLastError();
        return fail(DMX_ERR_INVALID, "%s: %s of container %d reach beyond their device allocation", who, what, k);
    }
    return 0;
}

}  // namespace

namespace dmx {
namespace host {

int check_device_containers(dmx_ctx *c, const dmx_call_container *views, int n_views, const char *who)
{
    if (n_views < 0 || (n_views > 0 && !views)) return fail(DMX_ERR_INVALID, "bad container list");
    for (int k = 0; k < n_views; k++) {
        const dmx_call_container &p = views[k];
        if (p.n_snp_calls < 0 || p.n_molecules < 0) return fail(DMX_ERR_INVALID, "container %d: negative size", k);
        if (p.n_snp_calls > 0 && (!p.snp_calls || !p.molecules || p.n_molecules == 0))
            return fail(DMX_ERR_INVALID, "container %d: calls without a molecule table", k);
        if (p.n_snp_calls == 0) continue;  // (no kernel reads such a part)
        DMX_TRY(check_device_range(c->device, p.snp_calls, (size_t)p.n_snp_calls * SNP_CALL_BYTES, who, k, "the snp_calls"));
        DMX_TRY(check_device_range(c->device, p.molecules, (size_t)p.n_molecules * MOLECULE_BYTES, who, k, "the molecules"));
    }
    return 0;
}

}  // namespace host
}  // namespace dmx

extern "C" {

int dmx_calls_upload(dmx_ctx *c, const dmx_call_container *host, int64_t *handle)
{
    DMX_TRY(bind(c));
    if (!host || !handle) return fail(DMX_ERR_INVALID, "calls_upload: null argument");
    *handle = 0;
    DMX_TRY(check_host_container(host));
    ResidentCalls set;
    const int rc = calls_upload(c, host, set);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_resident_calls(c, set);
        return rc;
    }
    *handle = install(c, set);
    return 0;
}

int dmx_calls_open(dmx_ctx *c, int64_t *handle)
{
    DMX_TRY(bind(c));
    if (!handle) return fail(DMX_ERR_INVALID, "calls_open: null handle");
    *handle = install(c, ResidentCalls());
    return 0;
}

int dmx_calls_append_counted(dmx_ctx *c, int64_t handle)
{
    DMX_TRY(bind(c));
    ResidentCalls *set = nullptr;
    DMX_TRY(find_resident_calls(c, handle, "calls_append_counted", &set));
    if (set->sealed) return fail(DMX_ERR_INVALID, "calls_append_counted: the set %lld is sealed", (long long)handle);
    if (c->cr_molecules < 0)
        return fail(DMX_ERR_INVALID, "call order: calls_append_counted needs the records of a dmx_count_reads or dmx_count_reads_push that succeeded");
    if (c->cr_molecules == 0 && c->cr_calls == 0) return 0;  // a push that emitted nothing
    // molecule_index of a stream's push counts on from the molecules the stream emitted before it; a one-shot count starts at 0
    const long long first = c->crs_state == 0 ? 0 : c->crs_molecules - c->cr_molecules;
    if (first != set->n_molecules)
        return fail(DMX_ERR_INVALID, "calls_append_counted: the records count their molecules from %lld on, the set holds %lld", first, set->n_molecules);
    if (set->n_molecules + c->cr_molecules > INT_MAX) return fail(DMX_ERR_UNSUPPORTED, "at most 2^31 - 1 molecules in a call set");
    DMX_TRY(reserve(c, *set, set->n_molecules + c->cr_molecules, set->n_calls + c->cr_calls, false));
    if (c->cr_molecules)
        HIP_TRY(hipMemcpyAsync(set->molecules + set->n_molecules * MOLECULE_BYTES, c->d_cr_molecules.p, (size_t)c->cr_molecules * MOLECULE_BYTES,
                               hipMemcpyDeviceToDevice, c->stream));
    if (c->cr_calls)
        HIP_TRY(hipMemcpyAsync(set->calls + set->n_calls * SNP_CALL_BYTES, c->d_cr_calls.p, (size_t)c->cr_calls * SNP_CALL_BYTES,
                               hipMemcpyDeviceToDevice, c->stream));
    set->n_molecules += c->cr_molecules;
    set->n_calls += c->cr_calls;
    return 0;
}

int dmx_calls_seal(dmx_ctx *c, int64_t handle)
{
    DMX_TRY(bind(c));
    ResidentCalls *set = nullptr;
    DMX_TRY(find_resident_calls(c, handle, "calls_seal", &set));
    HIP_TRY(hipStreamSynchronize(c->stream));
    set->sealed = true;
    return 0;
}

int dmx_calls_concatenate(dmx_ctx *c, const int64_t *handles, int32_t n, int64_t *out)
{
    DMX_TRY(bind(c));
    if (n < 0 || (n && !handles) || !out) return fail(DMX_ERR_INVALID, "calls_concatenate: bad arguments");
    *out = 0;
    std::vector<ResidentCalls *> parts((size_t)n, nullptr);
    for (int k = 0; k < n; k++) DMX_TRY(find_sealed(c, handles[k], "calls_concatenate", &parts[(size_t)k]));
    ResidentCalls set;
    const int rc = calls_concatenate(c, parts, set);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        dmx::host::release_resident_calls(c, set);
        return rc;
    }
    *out = install(c, set);
    return 0;
}

int dmx_calls_view(dmx_ctx *c, int64_t handle, dmx_call_container *view)
{
    DMX_TRY(bind(c));
    if (!view) return fail(DMX_ERR_INVALID, "calls_view: null view");
    ResidentCalls *set = nullptr;
    DMX_TRY(find_sealed(c, handle, "calls_view", &set));
    view->snp_calls = set->n_calls ? set->calls : nullptr;
    view->n_snp_calls = set->n_calls;
    view->molecules = set->n_molecules ? set->molecules : nullptr;
    view->n_molecules = set->n_molecules;
    view->chrom = 0;
    return 0;
}

int dmx_calls_info(dmx_ctx *c, int64_t handle, int64_t *info)
{
    DMX_TRY(bind(c));
    if (!info) return fail(DMX_ERR_INVALID, "calls_info: null info");
    ResidentCalls *set = nullptr;
    DMX_TRY(find_resident_calls(c, handle, "calls_info", &set));
    info[0] = set->n_molecules;
    info[1] = set->n_calls;
    info[2] = held_bytes(*set);
    info[3] = set->sealed ? 1 : 0;
    return 0;
}

int dmx_calls_fetch(dmx_ctx *c, int64_t handle, void *molecules_out, void *snp_calls_out)
{
    DMX_TRY(bind(c));
    ResidentCalls *set = nullptr;
    DMX_TRY(find_sealed(c, handle, "calls_fetch", &set));
    if ((set->n_molecules && !molecules_out) || (set->n_calls && !snp_calls_out)) return fail(DMX_ERR_INVALID, "calls_fetch: null output");
    if (set->n_molecules)
        HIP_TRY(hipMemcpyAsync(molecules_out, set->molecules, (size_t)set->n_molecules * MOLECULE_BYTES, hipMemcpyDeviceToHost, c->stream));
    if (set->n_calls) HIP_TRY(hipMemcpyAsync(snp_calls_out, set->calls, (size_t)set->n_calls * SNP_CALL_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->calls_transfer_bytes[1] += call_record_bytes(set->n_molecules, set->n_calls);
    return 0;
}

int dmx_calls_release(dmx_ctx *c, int64_t handle)
{
    DMX_TRY(bind(c));
    ResidentCalls *set = nullptr;
    DMX_TRY(find_resident_calls(c, handle, "calls_release", &set));
    HIP_TRY(hipStreamSynchronize(c->stream));
    dmx::host::release_resident_calls(c, *set);
    c->resident_calls.erase(handle);
    return 0;
}

int dmx_calls_barcode_counts(dmx_ctx *c, int64_t handle, int64_t n_barcodes, int64_t *calls_per_barcode, int64_t *molecules_per_barcode)
{
    DMX_TRY(bind(c));
    if (n_barcodes < 0 || n_barcodes > INT_MAX) return fail(DMX_ERR_INVALID, "calls_barcode_counts: n_barcodes must be 0 .. 2^31 - 1");
    if (n_barcodes && (!calls_per_barcode || !molecules_per_barcode)) return fail(DMX_ERR_INVALID, "calls_barcode_counts: null output");
    ResidentCalls *set = nullptr;
    DMX_TRY(find_sealed(c, handle, "calls_barcode_counts", &set));
    return barcode_counts(c, *set, n_barcodes, calls_per_barcode, molecules_per_barcode);
}

int dmx_stage_device_containers(dmx_ctx *c, const dmx_call_container *views, int32_t n_views)
{
    DMX_TRY(bind(c));
    DMX_TRY(dmx::host::check_device_containers(c, views, n_views, "stage_device_containers"));
    return dmx::stage_device_containers(c, views, n_views);
}

int dmx_get_calls_transfer_bytes(dmx_ctx *c, int64_t *bytes)
{
    DMX_TRY(bind(c));
    if (!bytes) return fail(DMX_ERR_INVALID, "null bytes");
    bytes[0] = c->calls_transfer_bytes[0];
    bytes[1] = c->calls_transfer_bytes[1];
    return 0;
}

}  // extern "C"
