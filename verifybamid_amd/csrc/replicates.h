// replicates.h -- weighted-marker likelihood replicates: many integer weight vectors over ONE resident
// sample, evaluated together (marker_sum_kernels.hip) and searched in lock-step (lockstep.h).  vb2_replicates_* of the C-ABI.
#ifndef VB2_REPLICATES_H_
#define VB2_REPLICATES_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/vb2_abi.h"
#include "point_stage.h"

struct vb2_flat;

namespace vb2 {

class Context;

class Replicates {
public:
    // weight: [num_rep][ctx->num_marker] counts in panel order.  Device memory from the slab cache: the sorted weight rows
    // [num_rep][m_pad] and one stage (rows, weight-row indices, results, a launch's partial sums); the context must outlive it.
    static int create(Context* ctx, int num_rep, const uint8_t* weight, Replicates** out);
    ~Replicates();
    // replicate r evaluates num_point[r] (0..VB2_BATCH_SLOTS) points; rows and results concatenated in replicate order
    int eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk);
    // one OptimizeLLK per replicate under `model`, all advancing in lock-step, each step one eval()
    int optimize(const vb2_model& model, vb2_estimate* est, int32_t* status);
    // Measurement aid (tools/conditioned_time.py; event-timed, milliseconds per repetition into ms[reps]): ONE launch pair
    // of num_point <= kMaxPointsPerLaunch points (pc = 0.01, alpha = 0.03), point p under weight row p % num_rep.
    int time_launch(int num_point, int warmup, int reps, double* ms);

    Context* ctx = nullptr;
    int num_rep = 0;
    std::vector<int64_t> counted;          // [num_rep] counted markers of the sample with a weight > 0
    int64_t device_bytes = 0;              // what the set holds in device memory
    // eval() calls that reached the device, and their marker launches
    int64_t num_step() const { return stage_.num_step; }
    int64_t num_launch() const { return stage_.num_launch; }

private:
    Replicates() {}
    PointStage::Launch launcher() const;
    uint8_t* d_weights_ = nullptr;
    size_t d_weights_bytes_ = 0;
    PointStage stage_;                     // num_rep * VB2_BATCH_SLOTS points; the indices: weight rows
};

// The lock-step driver over any evaluator of a step (vb2_replicates_lockstep; no device): replicate r's search is the
// reference-exact OptimizeLLK from the reference start.  A replicate whose first evaluation returns exactly 0.0 for every
// point selects no counted marker (a counted marker's log-likelihood is negative): its status is VB2_ERR_INVALID and the
// others go on.  The return value: a failure of fn (it ends every search).
int replicates_lockstep(vb2_replicates_eval_fn fn, void* user, int num_rep, int num_pc, bool data_has_known_af,
                        const vb2_model& model, vb2_estimate* est, int32_t* status, int64_t* num_step);

// vb2_run with a stage between the search and the writers: hook(ctx, flat, model, estimate) runs on the run's context (one
// device) after a successful search; a non-zero return fails the run.  Defined in abi.cpp.
typedef std::function<int(vb2_ctx* ctx, const vb2_flat& flat, const vb2_model& model, const vb2_estimate& est)> RunHook;
int run_with_hook(const vb2_run_args* args, vb2_run_result* out, const RunHook& hook);

}  // namespace vb2

struct vb2_replicates {
    vb2::Replicates* impl;
};

#endif
