// plan_check.h -- the frame the check programs of the pure host headers share (tests/*_check.cpp; built and run by
// tests/check_program.py): the counters and EXPECT, the comparison of two verdicts, the small pooled call most plans are walked on,
// and the summary line with the exit status.  It lives in tests/ and is included by the programs next to it: nothing under
// demuxalot_amd/csrc can reach it.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

static int failures = 0, checks = 0;
// (a macro, so that the line printed is the line of the program that expects; a walk over thousands of states names its first failures)
#define EXPECT(cond)                                                 \
    do {                                                             \
        checks++;                                                    \
        if (!(cond)) {                                               \
            failures++;                                              \
            if (failures < 40) std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
        }                                                            \
    } while (0)

// two verdicts of any plan (status, what, at, value) say the same: the same code, the very same words, index and value
template <class Verdict>
static bool same(const Verdict &a, const Verdict &b)
{
    return a.status == b.status && a.what == b.what && a.at == b.at && a.value == b.value;
}

// one call's arrays, owned: pools {0, 2, 4} and {1, 3} of G = 5, four barcodes, the second in no pool; rows of 6, 0, 3 and 6 options.
// A program extends it with the arrays of its own entry (a grid, weights, rows, fractions, ...); Pools is its plan's view of the pools.
template <class Pools>
struct PooledCall {
    int with_doublets = 1;
    std::vector<int64_t> pool_start{0, 3, 5};
    std::vector<int32_t> donors{0, 2, 4, 1, 3};
    std::vector<float> penalty{-1.5f, 0.25f};
    std::vector<int32_t> pool_of{0, -1, 1, 0};
    std::vector<int64_t> row_ptr{0, 6, 6, 9, 15};
    Pools pools() const { return {with_doublets, (long long)pool_start.size() - 1, pool_start.data(), donors.data(), penalty.data(), pool_of.data(), row_ptr.data()}; }
    void singlets_only()
    {
        with_doublets = 0;
        row_ptr = {0, 3, 3, 5, 8};
    }
};

// Everything the pooled entries refuse of the context and the pools, once each: add(call, facts, code) is handed every such call
// with the facts it is made under and the code it must be refused with (the plan's INVALID or UNSUPPORTED).  The order is the one
// the programs index into: no problem, no table, a communicator, two ranks, a padded table, then the pools.  What is then checked
// of every one of them - against which verdict, behind which bad arguments of its own - is the program's.
template <class Call, class Facts, class Add>
static void borrowed_refusals(const Facts &good, int G, int invalid, int unsupported, Add add)
{
    const Call ok;
    Facts f = good;
    f.have_problem = false;
    add(ok, f, invalid);
    f = good;
    f.have_table = false;
    add(ok, f, invalid);
    f = good;
    f.attached = true;
    add(ok, f, unsupported);
    f = good;
    f.nranks = 2;
    add(ok, f, unsupported);
    f = good;
    f.dense_table = false;
    add(ok, f, unsupported);
    Call c;
    c.with_doublets = 2;
    add(c, good, invalid);
    c = Call();
    c.pool_start[0] = 1;
    add(c, good, invalid);
    c = Call();
    c.pool_start = {0, 3, 3};  // the second pool is empty
    add(c, good, invalid);
    c = Call();
    c.donors = {0, 2, 2, 1, 3};  // not strictly ascending
    add(c, good, invalid);
    c = Call();
    c.donors[4] = G;
    add(c, good, invalid);
    c = Call();
    c.pool_of[3] = 2;
    add(c, good, invalid);
    c = Call();
    c.row_ptr[4] += 1;
    add(c, good, invalid);
}

// "<what>: N checks, M failures", and the program's exit status
static inline int finish(const char *what)
{
    std::printf("%s: %d checks, %d failures\n", what, checks, failures);
    return failures ? 1 : 0;
}
