// refit.h -- the lock-step searches of the rows of a set (replicates, hypotheses, pair hypotheses) over any evaluator of a
// step: row r's search is the reference-exact OptimizeLLK under the model, one side of its points held where the options
// say so.  No device: vb2_replicates_lockstep, vb2_conditioned_lockstep and vb2_paired_lockstep hand it a caller's
// evaluator, the sets on a context their own (row_set.cpp).
#ifndef VB2_REFIT_H_
#define VB2_REFIT_H_

#include <cstdint>

#include "../../include/vb2_abi.h"

namespace vb2 {

// One step of every row still searching: row r's num_point[r] points, rows and results concatenated in row order (the shape
// of vb2_replicates_eval_fn, vb2_conditioned_eval_fn and vb2_paired_eval_fn).
typedef int (*RowsEvalFn)(void* user, int32_t num_row, const int32_t* num_point, const double* pc1, const double* pc2,
                          const double* alpha, double* llk);

struct Refit {
    enum Held { kNone, kPc1, kPc2 };
    const char* who = "";                  // the entry the messages name
    const char* empty_message = "";        // the last error where a row turns out empty (below)
    Held held = kNone;                     // the side overwritten with the row's fixed PCs on the way to the evaluator ...
    const double* fixed = nullptr;         // ... fixed + (fixed_row ? fixed_row[r] : r) * num_pc, the llk0 call included
    const int32_t* fixed_row = nullptr;
    bool homogeneous = false;              // the searches run under is_heter = 0: pc1 = pc2 = v, the reference's start
    bool refuse_fixed_alpha = false;       // a fixed alpha leaves the search nothing to estimate: VB2_ERR_INVALID
    const uint8_t* known_af = nullptr;     // [num_row] the row's data has known allele frequencies; null: none has
    int64_t* num_step = nullptr;           // the steps taken, where asked for
};

// A row whose first evaluation returns exactly 0.0 for every point counts no marker (a counted marker's log-likelihood is
// negative): its status is VB2_ERR_INVALID and the others go on.  The return value: a failure of fn (it ends every search).
int refit_lockstep(const Refit& opt, RowsEvalFn fn, void* user, int num_row, int num_pc, const vb2_model& model,
                   vb2_estimate* est, int32_t* status);

}  // namespace vb2
#endif
