// cohort_stages.h -- the seam between the cohort pipeline (cohort.cpp) and what a run does after its last sample
// (cohort_stages.cpp: --FindSource, --FindRelated, --RefitSource, --MatchedNormal with --PairInterval).  The pipeline
// knows a feature only as a CohortStage: four questions while the samples retire, one call when they all have.
#ifndef VB2_COHORT_STAGES_H_
#define VB2_COHORT_STAGES_H_

#include <initializer_list>
#include <memory>
#include <vector>

#include "context.h"
#include "host_clock.h"
#include "hostio.h"
#include "source.h"

namespace vb2 {

// What finish() works on.  The pipeline's threads are joined; `set` (null when no stage asked for planes) and the parked
// contexts ([sample], null = not kept; empty when none was) are the pipeline's and outlive every stage's finish().
struct CohortEnd {
    const vb2_cohort_args* a;
    vb2_run_result* out;
    int32_t* status;
    const vb2_model& model;
    SourceSet* set;
    const std::vector<vb2_ctx*>& parked;
    int64_t parked_bytes;
};

struct CohortStage {
    const char* const flag;                            // names the stage where a sample's row cannot be made
    const int planes;                                  // 1. the source-set planes it reads (the run's set has the OR; 0: none)
    CohortStage(const char* name, int reads) : flag(name), planes(reads) {}
    virtual ~CohortStage() = default;
    virtual bool wants_row(int) const { return true; }             // 2. a searched sample s gets a row in the set
    virtual bool keeps(int, bool /*row_made*/) const { return false; }      // 3. ... and its context stays for finish()
    // 4. the stage takes the retiring samples' flattened inputs: the readers then leave the raw arrays in them, and the
    // releaser hands every searched sample's over (with its estimate) instead of freeing it
    virtual bool takes_flat() const { return false; }
    virtual void take_flat(int, std::unique_ptr<vb2_flat>, const vb2_estimate&) {}
    // once, on the calling thread, in the order the stages were given; a failure (its text in g_last_error) fails the run
    // and skips the stages behind.  A set a stage builds on a parked context goes before finish() returns.
    virtual int finish(const CohortEnd& e) = 0;
};

struct CohortStages {
    std::initializer_list<CohortStage*> after;     // (a null is skipped) questions 2 and 3 are asked on the releaser thread
    bool intervals = false;                // --CohortInterval: a stage of the pipeline itself; ci [S] may be null
    vb2_interval* ci = nullptr;
    const double* err_table = nullptr;     // --ErrorTable: every sample's context is made under it (vb2_ctx_create_ex)
};

// A cohort run with these stages; no exception leaves it, the run's error is the last error.
int cohort_run_with(const vb2_cohort_args* a, vb2_run_result* out, int32_t* status, const CohortStages& stages);

}  // namespace vb2
#endif
