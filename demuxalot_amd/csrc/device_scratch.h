// device_scratch.h -- what the multi-stage device passes share on the host side: temporaries from the context's block cache
// that go back when the call leaves, uploads, rocPRIM scans, sorts and reductions on the ctx stream, the stage clock.  Every
// .hip file that needs device temporaries for the length of a call or calls rocPRIM takes them from here.
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
    // Hand-over: the block leaves this call's temporaries and stays allocated; the caller owns it from here (ctx_free when done).
    // False when the block is not one of this call's.
    bool hand_over(const void *p)
    {
        for (size_t i = 0; i < ptrs.size(); i++)
            if (ptrs[i] == p) {
                ptrs.erase(ptrs.begin() + (long)i);
                return true;
            }
        return false;
    }
};

inline unsigned grid_for(long long n) { return (unsigned)((n + 255) / 256); }

constexpr int bits_for(ull n)  // bits that hold the values 0 .. n-1 (n is a count)
{
    int b = 0;
    while (b < 64 && (n - 1) >> b) b++;
    return n <= 1 ? 0 : b;
}

constexpr unsigned bits_of(ull max_value)  // bits of max_value itself, at least 1: a radix sort's end bit for keys up to it
{
    return bits_for(max_value + 1) > 1 ? (unsigned)bits_for(max_value + 1) : 1u;
}

// 64 as a count takes 6 bits (0 .. 63), as a value 7
static_assert(bits_for(0) == 0 && bits_for(1) == 0 && bits_for(2) == 1 && bits_for(63) == 6 && bits_for(64) == 6 && bits_for(65) == 7, "");
static_assert(bits_for((1ull << 32) - 1) == 32 && bits_for(1ull << 32) == 32 && bits_for((1ull << 32) + 1) == 33, "");
static_assert(bits_of(0) == 1 && bits_of(1) == 1 && bits_of(2) == 2 && bits_of(63) == 6 && bits_of(64) == 7 && bits_of(65) == 7, "");
static_assert(bits_of((1ull << 32) - 1) == 32 && bits_of(1ull << 32) == 33 && bits_of((1ull << 32) + 1) == 33, "");

template <typename T>
int upload(Scratch &sc, T **out, const T *host, size_t count, hipStream_t st)
{
    DMX_TRY(sc.get(out, count));
    if (count) HIP_TRY(hipMemcpyAsync(*out, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
}

// A rocPRIM device call runs twice: without temporary storage it only reports how many bytes it wants, then it runs in that
// many bytes of sc.  call(void *temp, size_t &bytes) -> hipError_t; the wrappers below leave the iterator types as the caller
// has them (they are part of the names of the kernels rocPRIM instantiates).
template <typename Call>
int with_temp_storage(Scratch &sc, const char *what, Call call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) {
        char *tmp = nullptr;
        DMX_TRY(sc.get(&tmp, bytes));
        e = call(tmp, bytes);
    }
    if (e != hipSuccess) return fail(DMX_ERR_HIP, "rocprim::%s failed: %s", what, hipGetErrorString(e));
    return 0;
}

template <typename In, typename Out, typename Op>
int inclusive_scan(Scratch &sc, In in, Out out, size_t n, Op op, hipStream_t st)
{
    return with_temp_storage(sc, "inclusive_scan", [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in, out, n, op, st); });
}

template <typename In, typename Out, typename T, typename Op>
int exclusive_scan(Scratch &sc, In in, Out out, T first, size_t n, Op op, hipStream_t st)
{
    return with_temp_storage(sc, "exclusive_scan", [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, first, n, op, st); });
}

template <typename In, typename Out, typename T, typename Op>
int reduce(Scratch &sc, In in, Out out, T first, size_t n, Op op, hipStream_t st)
{
    return with_temp_storage(sc, "reduce", [&](void *t, size_t &b) { return rocprim::reduce(t, b, in, out, first, n, op, st); });
}

// out[i] = op(in[0] .. in[i]); the last entry is returned through *total (synchronises)
template <typename T, typename Op>
int inclusive_scan_total(Scratch &sc, const T *in, T *out, size_t n, T *total, Op op, hipStream_t st)
{
    *total = 0;
    if (n == 0) return 0;
    DMX_TRY(inclusive_scan(sc, in, out, n, op, st));
    HIP_TRY(hipMemcpyAsync(total, out + n - 1, sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// (a template, as everything here that reaches rocPRIM: a file that does not call it instantiates none of its kernels)
template <typename T>
int sum_scan(Scratch &sc, const T *in, T *out, size_t n, T *total, hipStream_t st)
{
    return inclusive_scan_total(sc, in, out, n, total, rocprim::plus<T>(), st);
}

template <typename K>
int sort_keys(Scratch &sc, const K *in, K *out, size_t n, unsigned end_bit, hipStream_t st)
{
    if (n == 0) return 0;
    return with_temp_storage(sc, "radix_sort_keys", [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, in, out, n, 0u, end_bit, st); });
}

// stable (LSD radix sort): equal keys keep their input order
template <typename K, typename V>
int sort_pairs(Scratch &sc, const K *keys_in, K *keys_out, const V *vals_in, V *vals_out, size_t n, unsigned end_bit, hipStream_t st)
{
    if (n == 0) return 0;
    if (end_bit == 0) end_bit = 1;
    return with_temp_storage(sc, "radix_sort_pairs", [&](void *t, size_t &b) {
        return rocprim::radix_sort_pairs(t, b, keys_in, keys_out, vals_in, vals_out, n, 0u, end_bit, st);
    });
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
