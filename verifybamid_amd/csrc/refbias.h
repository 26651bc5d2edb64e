// refbias.h -- the reference bias beta estimated jointly with FREEMIX (vb2_abi.h section 3g): rows of
// ONE double, a beta each, over ONE resident sample, evaluated together (refbias_kernels.hip) and refitted in lock-step
// (refit.h); the fixed procedure that maximises the profile likelihood over beta, over any evaluator.  vb2_refbias_* of the
// C-ABI.
#ifndef VB2_REFBIAS_H_
#define VB2_REFBIAS_H_

#include <cstdint>

#include "../../include/vb2_abi.h"
#include "row_set.h"

namespace vb2 {

// A row set (row_set.h: eval, eval_begin / eval_end, time_launch, num_row, device_bytes) whose rows are values of beta.
class RefBias : public RowSet {
public:
    // beta: [num_row] within [0.25, 0.75] (host).  Refused on a probability-domain context whose bound (Context::pd_max_bound)
    // exceeds kPdMaxBound / 2.  Device memory from the slab cache; the context must outlive the set.
    static int create(Context* ctx, int num_row, const double* beta, RefBias** out);
    // one OptimizeLLK per row under `model` as it is, all advancing in lock-step, each step one eval()
    int optimize(const vb2_model& model, vb2_estimate* est, int32_t* status);

private:
    RefBias();
};

// The procedure of section 3g over any evaluator (vb2_refbias_lockstep; no device).  The device and the restatement go
// through this one statement of it.
int refbias_fit(vb2_refbias_eval_fn fn, void* user, int num_pc, const vb2_model& model, bool data_has_known_af,
                vb2_refbias_fit* out);
// ... over sets on the context, one per lock-step call (vb2_refbias_fit_ctx)
int refbias_fit_ctx(Context* ctx, const vb2_model& model, vb2_refbias_fit* out);

}  // namespace vb2

struct vb2_refbias {
    vb2::RefBias* impl;
};

#endif
