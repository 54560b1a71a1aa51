// device_scratch.h -- what the multi-stage device passes (count_reads.hip, coverage.hip) share on the host side: temporaries
// from the context's block cache that go back when the call leaves, uploads, rocPRIM scans and sorts on the ctx stream, the
// stage clock.
#pragma once
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "dmx_host.h"

namespace dmx {
namespace scratch {

typedef unsigned long long ull;

struct Scratch {
    dmx_ctx *ctx;
    std::vector<void *> ptrs;
    size_t held = 0;  // bytes asked for so far; nothing goes back before the call leaves, so this is also the peak
    explicit Scratch(dmx_ctx *c) : ctx(c) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        // an error return leaves with kernels and copies of this call still queued: they finish before their blocks go back
        // to the context's cache (after a call that succeeded the stream is idle already)
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : ptrs) ctx_free(ctx, p);
    }
    template <typename T>
    int get(T **out, size_t count)
    {
        void *p = nullptr;
        const int rc = ctx_malloc(ctx, &p, (count ? count : 1) * sizeof(T));
        if (rc) return rc;
        ptrs.push_back(p);
        held += (count ? count : 1) * sizeof(T);
        *out = (T *)p;
        return 0;
    }
};

inline unsigned grid_for(long long n) { return (unsigned)((n + 255) / 256); }

inline int bits_for(ull n)  // bits that hold the values 0 .. n-1
{
    int b = 0;
    while (b < 64 && (n - 1) >> b) b++;
    return n <= 1 ? 0 : b;
}

template <typename T>
int upload(Scratch &sc, T **out, const T *host, size_t count, hipStream_t st)
{
    DMX_TRY(sc.get(out, count));
    if (count) HIP_TRY(hipMemcpyAsync(*out, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
}

// out[i] = op(in[0] .. in[i]); the last entry is returned through *total (synchronises)
template <typename Op>
int inclusive_scan_total(Scratch &sc, const ull *in, ull *out, size_t n, ull *total, Op op, hipStream_t st)
{
    *total = 0;
    if (n == 0) return 0;
    size_t bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, bytes, in, out, n, op, st));
    char *tmp = nullptr;
    DMX_TRY(sc.get(&tmp, bytes));
    HIP_TRY(rocprim::inclusive_scan(tmp, bytes, in, out, n, op, st));
    HIP_TRY(hipMemcpyAsync(total, out + n - 1, sizeof(ull), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

inline int sum_scan(Scratch &sc, const ull *in, ull *out, size_t n, ull *total, hipStream_t st)
{
    return inclusive_scan_total(sc, in, out, n, total, rocprim::plus<ull>(), st);
}

// stable (LSD radix sort): equal keys keep their input order
template <typename K, typename V>
int sort_pairs(Scratch &sc, const K *keys_in, K *keys_out, const V *vals_in, V *vals_out, size_t n, unsigned end_bit, hipStream_t st)
{
    if (n == 0) return 0;
    if (end_bit == 0) end_bit = 1;
    size_t bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, end_bit, st));
    char *tmp = nullptr;
    DMX_TRY(sc.get(&tmp, bytes));
    HIP_TRY(rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, end_bit, st));
    return 0;
}

// hipEvents at the boundaries of a pass's N stages (dmx_get_count_reads_timings, dmx_get_coverage_timings)
template <int N>
struct StageClock {
    hipEvent_t ev[N + 1] = {};
    int n = 0;
    ~StageClock()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int tick(hipStream_t st)
    {
        HIP_TRY(hipEventCreate(&ev[n]));
        HIP_TRY(hipEventRecord(ev[n], st));
        n++;
        return 0;
    }
    // the spans between the ticks so far into ms[first ..]
    int read(double *ms, int first)
    {
        for (int s = 0; s + 1 < n; s++) {
            float span = 0.0f;
            HIP_TRY(hipEventElapsedTime(&span, ev[s], ev[s + 1]));
            ms[first + s] = span;
        }
        return 0;
    }
};

inline int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DMX_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace scratch
}  // namespace dmx
