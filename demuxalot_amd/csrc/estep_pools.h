// estep_pools.h -- the pooled E-step (estep_pools.hip; dmx_steps.cpp: dmx_estep_pools): every barcode is scored against the
// donors of its own pool only, all pools in one pass over the resident call records and the one resident genotype table.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pools_plan.h"

struct dmx_ctx;

namespace dmx {

constexpr int POOL_MAX_OPTIONS = (int)pplan::MAX_OPTIONS;  // what pools_plan.h lets through: the widest bucket, 16 slots of 64 lanes
constexpr int POOL_BUCKETS = 5;         // option slots per lane of a launch: 1, 2, 4, 8, 16
inline int pool_bucket_slots(int bucket) { return 1 << bucket; }
static_assert(POOL_MAX_OPTIONS == 64 << (POOL_BUCKETS - 1), "the widest bucket holds the largest pool");
inline int pool_bucket_of(int n_options)  // the narrowest instantiation that holds ceil(n_options / 64) slots
{
    const int slots = (n_options + 63) / 64;
    int bucket = 0;
    while (pool_bucket_slots(bucket) < slots) bucket++;
    return bucket;
}

// argument block of k_estep_pools: one launch walks the barcodes of `list`
struct PoolEstepArgs {
    const long long *pair_ptr;  // [B + 1] the resident problem's records, as EstepArgs has them
    const CallPair *pairs;
    const float *prob;          // [rows, G]
    unsigned prob_bytes;
    const int *list;            // [n_list] barcodes of this launch, by decreasing row length
    long long n_list;
    const int *pool_of;          // [B] pool of every barcode (-1: none; such a barcode is in no list)
    const long long *row_ptr;    // [B + 1] first entry of every barcode's compact row
    const long long *opt_ptr;    // [P + 1] first option of every pool in `opts`
    const unsigned *opts;        // d1 | d2 << 16 (table columns; a singlet: d1 == d2), the layout of EstepArgs::opt_pairs
    const int *pool_size;        // [P] donors of the pool = its singlet options
    const float *pair_penalty;   // [P] logit offset of the pool's pair options
    float *logits, *post;        // compact rows
    int *best;                   // [B] first arg-max option inside the pool's list
    float *best_prob;            // [B]
    double *pair_mass;           // [B] float64 sum of the pair posteriors in ascending option order
    float *dense;                // [B, G] the DENSE form only: a barcode's singlet posteriors at the table columns of its pool's donors.
    int G;                       //        The kernel writes nothing else of the row: the host zeroes the matrix once per call.
};

// dense: the form that also leaves the singlet posteriors in a.dense (learning within pools: the M-step's input)
hipError_t launch_estep_pools(hipStream_t st, const PoolEstepArgs &a, int slots, bool pairs, bool dense = false);

// what dmx_estep_pools has validated and laid out on the host (pools_plan.h: check, layout)
struct PoolsPlan {
    bool with_doublets;
    long long n_pools;
    std::vector<long long> opt_ptr;    // [P + 1]
    std::vector<unsigned> opts;
    std::vector<int> pool_size;        // [P]
    const float *pair_penalty;         // [P]
    const int32_t *pool_of_barcode;    // [B]
    const int64_t *row_ptr;            // [B + 1]
    float *logits_out, *probs_out;     // nullable
    int32_t *best_option;              // nullable
    float *best_prob;
    double *doublet_mass;
};
// The device half in three parts, so that a call of several E-steps (dmx_em_pools) pays the host round trip once.
//   prepare    the download of the context's `order`, the bucket lists, every upload, the compact result buffers; `plan` outlives the run
//   launch     one launch per non-empty bucket.  A dense run writes the singlet posteriors into the context's own d_post as [B, G]
//              (the caller has set K = G and zeroed it: dmx_steps.cpp, begin_dense_pools), rebuilds d_nz / d_first with the floor of
//              `power`; the context's flags: ctx_state.h dense_pass_done
//   read back  the compact rows and read-outs; -1 / NaN for the barcodes of no pool
// The run holds its temporaries (device_scratch.h) until it is destroyed.
struct PoolsRun;
struct PoolsRunDeleter {
    void operator()(PoolsRun *run) const;
};
typedef std::unique_ptr<PoolsRun, PoolsRunDeleter> PoolsRunPtr;
int prepare_estep_pools(dmx_ctx *c, const PoolsPlan &plan, bool dense, PoolsRunPtr &run);
int launch_estep_pools_pass(dmx_ctx *c, PoolsRun &run, float power);
int read_back_estep_pools(dmx_ctx *c, PoolsRun &run);
// the tail of a dense launch, inside its span of the timer: the rebuild and the context's flags.  The dense pass of another kernel
// on a prepared run (estep_ambient.hip) ends with it too.
int close_dense_pools_pass(dmx_ctx *c, float power);
// the three in a row without the dense form: dmx_estep_pools
int run_estep_pools(dmx_ctx *c, const PoolsPlan &plan);
// What another kernel needs to walk a prepared run in place of launch_estep_pools_pass (estep_ambient.hip): the argument block
// without `list` / `n_list` / `dense`, and the barcodes of every bucket.
struct PoolsLaunchView {
    PoolEstepArgs args;
    const int *lists[POOL_BUCKETS];
    long long n_lists[POOL_BUCKETS];
    bool with_doublets;
};
PoolsLaunchView pools_launch_view(const PoolsRun &run);

// dmx_set_keep_pooled: after a successful read-back the pass's compact result becomes the context's pooled slot.
// keep_pooled_result (pooled_readout.hip) hands the layout arrays and the rows over from the temporaries they were allocated in;
// keep_pools_run does so for a prepared run when the switch is on (and nothing when it is off), with the compact alpha_index /
// alpha_mean of a grid pass out of that pass's own temporaries.  dmx_estep_pools_resident, dmx_estep_ambient_resident, dmx_em_pools
// and dmx_em_ambient never call it: the slot is none of theirs.
namespace scratch {
struct Scratch;
}
int keep_pooled_result(dmx_ctx *c, const PoolsPlan &plan, const PoolEstepArgs &a, scratch::Scratch &rows, scratch::Scratch *grid,
                       const int *alpha_index, const float *alpha_mean);
int keep_pools_run(dmx_ctx *c, PoolsRun &run, scratch::Scratch *grid = nullptr, const int *alpha_index = nullptr, const float *alpha_mean = nullptr);

}  // namespace dmx
