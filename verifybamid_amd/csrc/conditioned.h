// conditioned.h -- the likelihood given a hypothesised contaminant: per-marker genotype priors
// ("hypotheses") over ONE resident sample, evaluated together (marker_sum_kernels.hip) and refitted in lock-step
// (lockstep.h).  vb2_conditioned_* of the C-ABI.
#ifndef VB2_CONDITIONED_H_
#define VB2_CONDITIONED_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "../../include/vb2_abi.h"
#include "point_stage.h"

namespace vb2 {

class Context;
class SourceSet;

class Conditioned {
public:
    // prior: [num_hyp][ctx->num_marker][3] float32 in panel order (host).  Device memory from the slab cache: the sorted
    // planes [num_hyp][3][m_pad] and one stage (rows, hypothesis indices, results, a launch's partial sums); one pinned
    // stage; the context must outlive the set.
    static int create(Context* ctx, int num_hyp, const float* prior, Conditioned** out);
    // hypothesis h = the q plane of the set's sample candidate[h], device to device
    static int create_from_set(Context* ctx, SourceSet* set, int num_hyp, const int32_t* candidate, Conditioned** out);
    ~Conditioned();
    // hypothesis h evaluates num_point[h] (0..VB2_BATCH_SLOTS) points; rows and results concatenated in hypothesis order
    int eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk);
    // the two halves of eval: upload and launch, asynchronous on the context's stream; synchronise and download.  A begin
    // without points needs no end (its end does nothing).
    int eval_begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha);
    int eval_end(double* llk);
    // Measurement aid (tools/conditioned_time.py; event-timed, milliseconds per repetition into ms[reps]): ONE launch pair
    // of num_point <= kMaxPointsPerLaunch points (pc = 0.01, alpha = 0.03), point p under hypothesis p % num_hyp.
    int time_launch(int num_point, int warmup, int reps, double* ms);

    Context* ctx = nullptr;
    int num_hyp = 0;
    int64_t device_bytes = 0;              // what the set holds in device memory
    // evaluations that reached the device, and their marker launches
    int64_t num_step() const { return stage_.num_step; }
    int64_t num_launch() const { return stage_.num_launch; }

private:
    Conditioned() {}
    static int make(Context* ctx, int num_hyp, const char* who, Conditioned** out);   // everything but the planes' content
    PointStage::Launch launcher() const;
    float* d_planes_ = nullptr;
    size_t d_planes_bytes_ = 0;
    PointStage stage_;                     // num_hyp * VB2_BATCH_SLOTS points; the indices: hypotheses
};

// The refits of every hypothesis of every set in ONE gang (vb2_conditioned_optimize_llk).
int conditioned_optimize(Conditioned* const* sets, int num_set, const vb2_model& model, const double* pc1_fixed,
                         vb2_estimate* est, int32_t* status);

// The lock-step driver over any evaluator of a step (vb2_conditioned_lockstep; no device): hypothesis h's search is the
// reference-exact OptimizeLLK under `model` with is_heter = 0, its pc1 rows overwritten with pc1_fixed + fixed_row[h] * k on
// their way to the evaluator.  known_af: [num_hyp] or null.  A hypothesis whose first evaluation returns exactly 0.0 for
// every point has no counted marker: its status is VB2_ERR_INVALID and the others go on.  The return value: a failure of
// the step (it ends every search).
typedef int (*ConditionedStep)(void* user, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                               double* llk);
int conditioned_lockstep(ConditionedStep fn, void* user, int num_hyp, int num_pc, const uint8_t* known_af, const vb2_model& model,
                         const double* pc1_fixed, const int32_t* fixed_row, vb2_estimate* est, int32_t* status);

}  // namespace vb2

struct vb2_conditioned {
    vb2::Conditioned* impl;
};

#endif
