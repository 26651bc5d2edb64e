// conditioned.h -- the likelihood given a hypothesised contaminant: per-marker genotype priors
// ("hypotheses") over ONE resident sample, evaluated together (marker_sum_kernels.hip) and refitted in lock-step
// (refit.h).  vb2_conditioned_* of the C-ABI.
#ifndef VB2_CONDITIONED_H_
#define VB2_CONDITIONED_H_

#include <cstdint>

#include "../../include/vb2_abi.h"
#include "row_set.h"

namespace vb2 {

class SourceSet;

// A row set (row_set.h: eval, eval_begin / eval_end, time_launch, num_row, device_bytes) whose rows are hypotheses.
class Conditioned : public RowSet {
public:
    // prior: [num_hyp][ctx->num_marker][3] float32 in panel order (host).  Device memory from the slab cache: the sorted
    // planes [num_hyp][3][m_pad] and one stage (rows, hypothesis indices, results, a launch's partial sums); one pinned
    // stage; the context must outlive the set.
    static int create(Context* ctx, int num_hyp, const float* prior, Conditioned** out);
    // hypothesis h = the q plane of the set's sample candidate[h], device to device
    static int create_from_set(Context* ctx, SourceSet* set, int num_hyp, const int32_t* candidate, Conditioned** out);

private:
    Conditioned();
    float* planes() const { return static_cast<float*>(d_payload_); }
};

// The refits of every hypothesis of every set in ONE gang (vb2_conditioned_optimize_llk): pc1_fixed [num_set][num_pc].
int conditioned_optimize(Conditioned* const* sets, int num_set, const vb2_model& model, const double* pc1_fixed,
                         vb2_estimate* est, int32_t* status);

// The lock-step driver over any evaluator of a step (vb2_conditioned_lockstep; no device): hypothesis h's search is the
// reference-exact OptimizeLLK under `model` with is_heter = 0, its pc1 rows overwritten with pc1_fixed + h * k on their way
// to the evaluator.  A hypothesis whose first evaluation returns exactly 0.0 for every point has no counted marker: its
// status is VB2_ERR_INVALID and the others go on.  The return value: a failure of the step (it ends every search).
int conditioned_lockstep(vb2_conditioned_eval_fn fn, void* user, int num_hyp, int num_pc, const vb2_model& model,
                         const double* pc1_fixed, vb2_estimate* est, int32_t* status);

}  // namespace vb2

struct vb2_conditioned {
    vb2::Conditioned* impl;
};

#endif
