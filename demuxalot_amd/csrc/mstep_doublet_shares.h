// mstep_doublet_shares.h -- the M-step that learns from doublets of unequal shares (mstep_doublet_shares.hip; dmx_steps.cpp:
// dmx_mstep_doublet_shares, dmx_em_doublet_shares): mstep_doublets.h's crediting with the pair's posterior mean share
// w of its first donor in the responsibility, r = own w_own / (own w_own + other w_other), w_own = w for the first donor and 1 - w
// for the second.  The third form in the frame of mstep_weighted.h.
#pragma once
#include <memory>

#include <hip/hip_runtime.h>

#include "estep_pair_shares.h"
#include "mstep_doublets.h"
#include "mstep_weighted.h"

struct dmx_ctx;

namespace dmx {

// the live-pair list with the share beside the posterior: one 16-byte entry per live pair, in row order (CSR).  count / live_ptr are
// DoubletList's (launch_live_count fills `count`)
struct DoubletShareList {
    unsigned long long *count;     // [B + 1] live pairs of every barcode, and 0
    unsigned long long *live_ptr;  // [B + 1] the exclusive scan of `count`
    uint4 *entries;                // (g | h << 16, the posterior's bits, the share's bits, 0); allocated for every pair option of every pooled barcode
};

// argument block of k_mstep_doublet_shares and k_mredo_doublet_shares: the shared block (mstep_weighted.h) and the list the weight reads
struct DoubletSharesMstepArgs {
    WeightedMstepArgs w;
    const unsigned long long *live_ptr;   // [B + 1]
    const uint4 *entries;
};
// k_live_pair_shares over the barcodes, behind launch_live_count and the host's scan; share_mean: compact like rows.post
hipError_t launch_live_share_fill(hipStream_t st, const DoubletRows &rows, const float *share_mean, long long B, float min_pair_posterior,
                                  const DoubletShareList &list);

// What a call keeps on the device for its M-steps: the rows' pointers, the shares', the list's buffers and their temporaries.
struct DoubletSharesRun;
struct DoubletSharesRunDeleter {
    void operator()(DoubletSharesRun *run) const;
};
typedef std::unique_ptr<DoubletSharesRun, DoubletSharesRunDeleter> DoubletSharesRunPtr;
// the list's buffers for the rows and the share_mean of a prepared dense pass (dmx_em_doublet_shares); pair_options: dlplan::pair_options
int prepare_doublet_shares_run(dmx_ctx *c, const PairSharesRun &estep, long long pair_options, DoubletSharesRunPtr &run);

// The M-step of the context's dense singlet posteriors, the run's rows and shares and the table into d_add, on the stream:
// begin_weighted_mstep, the list rebuilt (its own span of the DMX_T_ESTEP slot), run_weighted_mstep around k_mstep_doublet_shares and
// k_mredo_doublet_shares.
int run_mstep_doublet_shares(dmx_ctx *c, float power, float min_pair_posterior, DoubletSharesRun &run);
// dmx_mstep_doublet_shares' device half: the uploads of the layout, the caller's rows and shares, run_mstep_doublet_shares
int run_mstep_doublet_shares_from_host(dmx_ctx *c, float power, float min_pair_posterior, const PoolsPlan &plan, const float *rows,
                                       const float *shares, long long pair_options);

}  // namespace dmx
