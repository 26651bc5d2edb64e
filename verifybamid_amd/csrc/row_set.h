// row_set.h -- what Replicates, Conditioned and Paired are made of: rows of a per-marker payload (weight rows, prior
// planes) over ONE resident sample in the context's sorted order, one slab from the slab cache, and the stage that
// evaluates points of several rows together (point_stage.h).  A class says what it is with a Kind and fills the payload;
// the checks, the two halves of an evaluation and the lock-step refits of several sets (refit.h) are here once.
#ifndef VB2_ROW_SET_H_
#define VB2_ROW_SET_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/vb2_abi.h"
#include "point_stage.h"
#include "refit.h"

namespace vb2 {

class Context;
struct DeviceLayout;

class RowSet {
public:
    struct Kind {
        const char* eval_who;              // "vb2_conditioned_eval": the entry eval's messages name
        const char* count_noun;            // "a hypothesis's" point count outside ...
        const char* rows_noun;             // (1..65535 "hypotheses")
        const char* nomem_who;             // take_device's (device_util.h); null: none
        bool llk_checked_first;            // eval refuses a null llk before anything reaches the stream (else: after, drained)
        size_t (*row_bytes)(const DeviceLayout& L);
        // one launch pair (PointStage::Launch) over the payload
        hipError_t (*launch)(const DeviceLayout& L, int num_point, const double* d_rows, const int32_t* d_idx, const void* d_payload,
                             double* d_partial, double* d_out, hipStream_t stream);
    };

    RowSet(const RowSet&) = delete;
    RowSet& operator=(const RowSet&) = delete;
    // row r evaluates num_point[r] (0..VB2_BATCH_SLOTS) points; rows and results concatenated in row order
    int eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk);
    // the two halves of eval: upload and launch, asynchronous on the context's stream; synchronise and download.  A begin
    // without points needs no end (its end does nothing).
    int eval_begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha)
    {
        return begin(num_point, pc1, pc2, alpha, true);
    }
    int eval_end(double* llk) { return stage_.end(llk); }
    bool eval_pending() const { return stage_.pending() != 0; }     // between an eval_begin with points and its eval_end
    // Measurement aid (tools/conditioned_time.py, paired_time.py, replicate_time.py; event-timed, milliseconds per repetition
    // into ms[reps]): ONE launch pair of num_point <= kMaxPointsPerLaunch points (pc = 0.01, alpha = 0.03), point p under
    // row p % num_row.
    int time_launch(int num_point, int warmup, int reps, double* ms) { return stage_.time_launch(num_point, num_row, warmup, reps, ms, launch_); }

    Context* ctx = nullptr;
    int num_row = 0;
    int64_t device_bytes = 0;              // what the set holds in device memory
    // evaluations that reached the device, and their marker launches
    int64_t num_step() const { return stage_.num_step; }
    int64_t num_launch() const { return stage_.num_launch; }

protected:
    explicit RowSet(const Kind& kind) : kind_(kind) {}
    // (not virtual: a set is deleted as what it is.)  The device first, then the stage drained -- a begun evaluation reads
    // the payload --, then the slab back to the cache.
    ~RowSet();
    // The checks of a creating entry `who`, then everything but the payload's content: the slab and the stage.
    int init(Context* ctx, int num_row, const char* who);
    // Panel-order rows from the host into a slab that goes back to the cache when permute(d_panel) has put them into the
    // payload; failed: VB2_ERR_HIP, "<what><HIP's text>".
    int upload(const void* rows, size_t bytes, const char* what, const std::function<hipError_t(const void* d_panel)>& permute);
    void* d_payload_ = nullptr;            // [num_row] rows of kind.row_bytes
    size_t d_payload_bytes_ = 0;

private:
    int begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, bool have_llk);
    const Kind& kind_;
    PointStage stage_;                     // num_row * VB2_BATCH_SLOTS points; the indices: rows
    PointStage::Launch launch_;
};

// The refits of every row of every set in ONE gang (vb2_conditioned_optimize_llk, vb2_paired_optimize_llk): opt.fixed
// [num_set][num_pc], a set's rows all holding its own; opt.fixed_row and opt.known_af are filled in here.
int optimize_row_sets(RowSet* const* sets, int num_set, Refit opt, const vb2_model& model, vb2_estimate* est, int32_t* status);
template <class Set>
int optimize_sets(Set* const* sets, int num_set, const Refit& opt, const vb2_model& model, vb2_estimate* est, int32_t* status)
{
    const std::vector<RowSet*> base(sets, sets + (sets && num_set > 0 ? num_set : 0));
    return optimize_row_sets(sets ? base.data() : nullptr, num_set, opt, model, est, status);
}

}  // namespace vb2
#endif
