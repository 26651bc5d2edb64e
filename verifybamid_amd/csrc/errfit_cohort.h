// errfit_cohort.h -- the error-rate fit of a cohort (vb2_abi.h section 3h): errfit.h's procedure for
// up to 64 samples in lock-step, every sample on its own error table or all of them on one pooled table.  Written once over
// two callbacks -- the E-steps of the live samples and their searches under tables -- so that the device and the numpy
// restatement go through one statement of it.  vb2_errfit_cohort_* of the C-ABI.
#ifndef VB2_ERRFIT_COHORT_H_
#define VB2_ERRFIT_COHORT_H_

#include <functional>

#include "../../include/vb2_abi.h"

namespace vb2 {

struct ErrFitCohortSteps {
    // (n, s) [S][94] of the live samples, sample i at (pc1 [i][num_pc], pc2 [i][num_pc], alpha [i]) under err [i][94]
    std::function<int(const int32_t* live, const double* err, const double* pc1, const double* pc2, const double* alpha,
                      int64_t* n, double* s)> stats;
    // the reference-exact OptimizeLLK of every live sample from the reference's start under err [i][94]: est [i] and
    // status [i] of the live ones (a sample whose search fails leaves with its code; the others go on).  Non-zero: the step
    // failed as a whole and ends the fit
    std::function<int(const int32_t* live, const double* err, vb2_estimate* est, int32_t* status)> search;
};

// nominal [S]: every sample's own estimate; enter [S] or null: a sample whose own run failed (non-zero) never enters and
// keeps that code as its status.  fits [S]; pool: the pooled summary (filled in both modes: without pooling its table is
// empty and its sums are over the samples' own fits)
int errfit_cohort(const ErrFitCohortSteps& steps, int num_sample, int num_pc, const vb2_model& model, bool data_has_known_af,
                  const vb2_estimate* nominal, const int32_t* enter, const vb2_errfit_opts* opts, bool pooled, const char* who,
                  vb2_errfit* fits, vb2_errfit_pool* pool);

// ... on the device: one ErrStatBatch, per iteration fresh contexts under the new tables and one vb2_batch_optimize_llk
int errfit_cohort_inputs(const vb2_input* const* in, int num_sample, const vb2_options* opt, const vb2_model& model,
                         const vb2_estimate* nominal, const int32_t* enter, const vb2_errfit_opts* opts, bool pooled,
                         vb2_errfit* fits, vb2_errfit_pool* pool);

}  // namespace vb2
#endif
