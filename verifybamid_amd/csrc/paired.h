// paired.h -- the likelihood given genotype priors on BOTH components, with markers left out: pair
// hypotheses over ONE resident sample, evaluated together (marker_sum_kernels.hip: PairTerm) and refitted in lock-step
// (lockstep.h) with the intended sample's PCs held.  vb2_paired_* of the C-ABI; --MatchedNormal.
#ifndef VB2_PAIRED_H_
#define VB2_PAIRED_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "../../include/vb2_abi.h"
#include "point_stage.h"

namespace vb2 {

class Context;
class SourceSet;

class Paired {
public:
    // prior: [num_hyp][ctx->num_marker][6] float32 in panel order (host): pi1[3] | pi2[3] per marker.  Device memory from
    // the slab cache: the sorted planes [num_hyp][6][m_pad] and one stage; one pinned stage; the context must outlive the set.
    static int create(Context* ctx, int num_hyp, const float* prior, Paired** out);
    // hypothesis h = the paired rule on the q plane of the set's sample normal[h], device to device: pi1 all zero, pi2 = q
    // where the normal counts the marker and max(q[0], q[2]) >= hom_min, every other marker left out
    static int create_from_set(Context* ctx, SourceSet* set, int num_hyp, const int32_t* normal, double hom_min, Paired** out);
    ~Paired();
    // hypothesis h evaluates num_point[h] (0..VB2_BATCH_SLOTS) points; rows and results concatenated in hypothesis order
    int eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk);
    // the two halves of eval, as Conditioned's
    int eval_begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha);
    int eval_end(double* llk);
    // Measurement aid (tools/paired_time.py), as Conditioned::time_launch
    int time_launch(int num_point, int warmup, int reps, double* ms);

    Context* ctx = nullptr;
    int num_hyp = 0;
    int64_t device_bytes = 0;              // what the set holds in device memory
    std::vector<int64_t> given;            // [num_hyp] counted markers of the context the hypothesis does not leave out
    int64_t num_step() const { return stage_.num_step; }
    int64_t num_launch() const { return stage_.num_launch; }

private:
    Paired() {}
    static int make(Context* ctx, int num_hyp, const char* who, Paired** out);   // everything but the planes' content
    int count_given(const char* who);      // given[] from the planes (one plane per hypothesis comes down)
    PointStage::Launch launcher() const;
    float* d_planes_ = nullptr;
    size_t d_planes_bytes_ = 0;
    PointStage stage_;                     // num_hyp * VB2_BATCH_SLOTS points; the indices: hypotheses
};

// The refits of every hypothesis of every set in ONE gang (vb2_paired_optimize_llk): pc2_fixed [num_set][num_pc].
int paired_optimize(Paired* const* sets, int num_set, const vb2_model& model, const double* pc2_fixed, vb2_estimate* est,
                    int32_t* status);

// The lock-step driver over any evaluator of a step (vb2_paired_lockstep; no device): hypothesis h's search is the
// reference-exact OptimizeLLK under `model` with is_heter = 0, its pc2 rows overwritten with pc2_fixed + fixed_row[h] * k on
// their way to the evaluator, the llk0 call included.  known_af: [num_hyp] or null.  A hypothesis whose first evaluation
// returns exactly 0.0 for every point walks no marker: its status is VB2_ERR_INVALID and the others go on.  The return
// value: a failure of the step (it ends every search).
typedef int (*PairedStep)(void* user, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                          double* llk);
int paired_lockstep(PairedStep fn, void* user, int num_hyp, int num_pc, const uint8_t* known_af, const vb2_model& model,
                    const double* pc2_fixed, const int32_t* fixed_row, vb2_estimate* est, int32_t* status);

}  // namespace vb2

struct vb2_paired {
    vb2::Paired* impl;
};

#endif
