// errfit.h -- empirical base-error rates fitted jointly with FREEMIX (vb2_abi.h section 3h): the
// alternating maximisation over the error table and the model's parameters, written once over two callbacks -- the E-step
// and a search under a table -- so that the device and the numpy restatement go through the same statement of it.
// vb2_errfit_* and vb2_run_errfit of the C-ABI.
#ifndef VB2_ERRFIT_H_
#define VB2_ERRFIT_H_

#include <functional>
#include <string>

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

// the procedure's pieces, shared with the cohort form (errfit_cohort.h):
// the search's own point of an estimate: the reported PCs with the reference's swap of indices 0, 1 undone (source.cpp)
void errfit_search_point(const vb2_estimate& est, int k, bool heter, double* p1, double* p2);
// kappa, tol and max_iter of opts with the defaults filled in; VB2_ERR_INVALID (a fixed alpha too) with `who` in front
int errfit_options(const vb2_model& model, const vb2_errfit_opts* opts, const char* who, double* kappa, double* tol, int* max_iter);
void errfit_nominal_table(double* eps0);           // [94]: pow(10.0, q / -10.0)
// the M-step: next [94] from (n, s) under the prior; returns the stop rule's maximum against eps
double errfit_mstep(const int64_t* n, const double* s, const double* eps0, const double* eps, double kappa, double* next);

// <prefix>.ErrorFit and <prefix>.ErrorRates of vb2_run_errfit (vb2_abi.h section 3h); freemix: the run's own, folded
int write_errfit_files(const std::string& prefix, const std::string& seq_id, double freemix, const vb2_errfit& f);
// <prefix>.ErrorRates alone: a row per quality with reads
int write_error_rates(const std::string& prefix, const double* err, const int64_t* n, const double* s);

// ... on the device: one ErrStat, one fresh context per iteration
int errfit_input(const vb2_input* in, const vb2_options* opt, const vb2_model& model, const vb2_estimate& nominal,
                 const vb2_errfit_opts* opts, vb2_errfit* out);

}  // namespace vb2
#endif
