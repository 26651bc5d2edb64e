// replicates.h -- weighted-marker likelihood replicates: many integer weight vectors over ONE resident
// sample, evaluated together (marker_sum_kernels.hip) and searched in lock-step (refit.h).  vb2_replicates_* of the C-ABI.
#ifndef VB2_REPLICATES_H_
#define VB2_REPLICATES_H_

#include <cstdint>
#include <vector>

#include "../../include/vb2_abi.h"
#include "row_set.h"

namespace vb2 {

class Context;

// A row set (row_set.h: eval, time_launch, num_row, device_bytes) whose rows are weight vectors.  Its eval refuses a null llk
// before anything reaches the stream.
class Replicates : public RowSet {
public:
    // weight: [num_rep][ctx->num_marker] counts in panel order.  Device memory from the slab cache: the sorted weight rows
    // [num_rep][m_pad] and one stage (rows, weight-row indices, results, a launch's partial sums); the context must outlive it.
    static int create(Context* ctx, int num_rep, const uint8_t* weight, Replicates** out);
    // one OptimizeLLK per replicate under `model`, all advancing in lock-step, each step one eval()
    int optimize(const vb2_model& model, vb2_estimate* est, int32_t* status);

    std::vector<int64_t> counted;          // [num_rep] counted markers of the sample with a weight > 0

private:
    Replicates();
};

// The lock-step driver over any evaluator of a step (vb2_replicates_lockstep; no device): replicate r's search is the
// reference-exact OptimizeLLK from the reference start.  A replicate whose first evaluation returns exactly 0.0 for every
// point selects no counted marker (a counted marker's log-likelihood is negative): its status is VB2_ERR_INVALID and the
// others go on.  The return value: a failure of fn (it ends every search).
int replicates_lockstep(vb2_replicates_eval_fn fn, void* user, int num_rep, int num_pc, bool data_has_known_af,
                        const vb2_model& model, vb2_estimate* est, int32_t* status, int64_t* num_step);

}  // namespace vb2

struct vb2_replicates {
    vb2::Replicates* impl;
};

#endif
