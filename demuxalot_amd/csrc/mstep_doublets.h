// mstep_doublets.h -- the M-step that also learns from doublet posteriors (mstep_doublets.hip; dmx_steps.cpp: dmx_mstep_doublets,
// dmx_em_doublets): every call of a barcode credits each donor of a live pair option of the barcode's row with the
// donor's responsibility for the call in the even mixture, r = own / (own + other), weighted by the pair's posterior.
#pragma once
#include <memory>

#include <hip/hip_runtime.h>

#include "estep_pools.h"
#include "mstep_weighted.h"

struct dmx_ctx;

namespace dmx {

// the compact rows of a dense pooled E-step and the layout they are read by: device pointers (estep_pools.h: PoolEstepArgs)
struct DoubletRows {
    const float *post;          // compact rows, pool-local option order: singlets, then the pairs i < j, i-major
    const long long *row_ptr;   // [B + 1]
    const int *pool_of;         // [B] (-1: none)
    const long long *opt_ptr;   // [P + 1]
    const unsigned *opts;       // g | h << 16 (table columns)
    const int *pool_size;       // [P] donors of the pool = its singlet options
};

// the live-pair list: per barcode the pair options of its row at or above the threshold, in row order (CSR)
struct DoubletList {
    unsigned long long *count;     // [B + 1] live pairs of every barcode, and 0
    unsigned long long *live_ptr;  // [B + 1] the exclusive scan of `count`
    uint2 *entries;                // (g | h << 16, the posterior's bits); allocated for every pair option of every pooled barcode
};

// argument block of k_mstep_doublets and k_mredo_doublets: the shared block (mstep_weighted.h) and the list the weight reads
struct DoubletMstepArgs {
    WeightedMstepArgs w;
    const unsigned long long *live_ptr;   // [B + 1]
    const uint2 *entries;
};
// k_live_pairs<false> (count) and k_live_pairs<true> (fill) over the barcodes (the scan between them is the host's: device_scratch.h)
hipError_t launch_live_count(hipStream_t st, const DoubletRows &rows, long long B, float min_pair_posterior, unsigned long long *count);
hipError_t launch_live_fill(hipStream_t st, const DoubletRows &rows, long long B, float min_pair_posterior, const DoubletList &list);

// What a call keeps on the device for its M-steps: the rows' pointers, the list's buffers and the temporaries they came from.
struct DoubletRun;
struct DoubletRunDeleter {
    void operator()(DoubletRun *run) const;
};
typedef std::unique_ptr<DoubletRun, DoubletRunDeleter> DoubletRunPtr;
// the list's buffers for the rows of a prepared dense pooled run (dmx_em_doublets); pair_options: dlplan::pair_options of the pools
int prepare_doublet_run(dmx_ctx *c, const PoolsRun &pooled, long long pair_options, DoubletRunPtr &run);

// The M-step of the context's dense singlet posteriors, the run's rows and the table into d_add, on the stream:
// begin_weighted_mstep (mstep_weighted.h), the list rebuilt from the rows (its own span of the DMX_T_ESTEP slot: a pass over the
// E-step's result), run_weighted_mstep around k_mstep_doublets over every (work item, 64-column word) and k_mredo_doublets over the
// queue k_mcombine_weighted left.
int run_mstep_doublets(dmx_ctx *c, float power, float min_pair_posterior, DoubletRun &run);
// dmx_mstep_doublets' device half: the uploads of the layout and the caller's rows, run_mstep_doublets; temporaries go back on return
int run_mstep_doublets_from_host(dmx_ctx *c, float power, float min_pair_posterior, const PoolsPlan &plan, const float *rows, long long pair_options);

}  // namespace dmx
