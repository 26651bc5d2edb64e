// errfit.h -- empirical base-error rates fitted jointly with FREEMIX (vb2_abi.h section 3h): the
// alternating maximisation over the error table and the model's parameters, written once over two callbacks -- the E-step
// and a search under a table -- so that the device and the numpy restatement go through the same statement of it.
// vb2_errfit_* and vb2_run_errfit of the C-ABI.
#ifndef VB2_ERRFIT_H_
#define VB2_ERRFIT_H_

#include <functional>

#include "../../include/vb2_abi.h"

namespace vb2 {

struct ErrFitSteps {
    // (n, s) [94] at a point under a table
    std::function<int(const double* err, const double* pc1, const double* pc2, double alpha, int64_t* n, double* s)> stats;
    // the reference-exact OptimizeLLK from the reference's start, every evaluation under the table
    std::function<int(const double* err, vb2_estimate* est)> search;
};

// the procedure of section 3h; `who` names the entry in the messages
int errfit(const ErrFitSteps& steps, int num_pc, const vb2_model& model, bool data_has_known_af, const vb2_estimate& nominal,
           const vb2_errfit_opts* opts, const char* who, vb2_errfit* out);

// ... on the device: one ErrStat, one fresh context per iteration
int errfit_input(const vb2_input* in, const vb2_options* opt, const vb2_model& model, const vb2_estimate& nominal,
                 const vb2_errfit_opts* opts, vb2_errfit* out);

}  // namespace vb2
#endif
