// paired.h -- the likelihood given genotype priors on BOTH components, with markers left out: pair
// hypotheses over ONE resident sample, evaluated together (marker_sum_kernels.hip: PairTerm) and refitted in lock-step
// (refit.h) with the intended sample's PCs held.  vb2_paired_* of the C-ABI; --MatchedNormal.
#ifndef VB2_PAIRED_H_
#define VB2_PAIRED_H_

#include <cstdint>
#include <vector>

#include "../../include/vb2_abi.h"
#include "row_set.h"

namespace vb2 {

class SourceSet;
class PairDerivStage;

// A row set (row_set.h: eval, eval_begin / eval_end, time_launch, num_row, device_bytes) whose rows are pair hypotheses.
class Paired : public RowSet {
public:
    // prior: [num_hyp][ctx->num_marker][6] float32 in panel order (host): pi1[3] | pi2[3] per marker.  Device memory from
    // the slab cache: the sorted planes [num_hyp][6][m_pad] and one stage; one pinned stage; the context must outlive the set.
    static int create(Context* ctx, int num_hyp, const float* prior, Paired** out);
    // hypothesis h = the paired rule on the q plane of the set's sample normal[h], device to device: pi1 all zero, pi2 = q
    // where the normal counts the marker and max(q[0], q[2]) >= hom_min, every other marker left out
    static int create_from_set(Context* ctx, SourceSet* set, int num_hyp, const int32_t* normal, double hom_min, Paired** out);

    std::vector<int64_t> given;            // [num_hyp] counted markers of the context the hypothesis does not leave out

    ~Paired();
    // LLK(. | h), its gradient and Hessian (vb2_paired_derivs): paired_derivs on this set alone
    int derivs(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk, double* grad,
               double* hess);
    // The marker scratch of the derivative kernels, kDerivChunk x kDerivVals x m_pad doubles per hypothesis: from the slab
    // cache on the first call, kept for the set's lifetime and counted in device_bytes.
    int ensure_deriv_scratch();
    double* deriv_marker(int h) const;     // hypothesis h's share of it
    const float* hyp_planes(int h) const;  // its six planes [6][m_pad]

private:
    Paired();
    double* d_deriv_ = nullptr;
    size_t d_deriv_bytes_ = 0;
    PairDerivStage* deriv_stage_ = nullptr;   // derivs' own staging, on the first call
    int count_given(const char* who);      // given[] from the planes (one plane per hypothesis comes down)
    float* planes() const { return static_cast<float*>(d_payload_); }
};

// The refits of every hypothesis of every set in ONE gang (vb2_paired_optimize_llk): pc2_fixed [num_set][num_pc].
int paired_optimize(Paired* const* sets, int num_set, const vb2_model& model, const double* pc2_fixed, vb2_estimate* est,
                    int32_t* status);

// Where the job table, the planes table, the parameter rows and the outputs of a derivative step lie, in one pinned slab
// and one device slab from the caches: room for `num_job` (context, hypothesis) jobs of kDerivChunk points each.
class PairDerivStage {
public:
    static int create(int device, int num_job, int num_pc, PairDerivStage** out);
    ~PairDerivStage();
    size_t device_bytes() const { return d_bytes_; }
    int64_t num_step = 0;                  // launch pairs taken

private:
    friend int paired_derivs(Paired* const*, int, PairDerivStage*, const int32_t*, const double*, const double*, const double*,
                             double*, double*, double*);
    PairDerivStage() = default;
    int device_ = -1, num_job_ = 0, k_ = 0;
    size_t o_planes_ = 0, o_rows_ = 0, o_res_ = 0, total_ = 0;
    void *d_ = nullptr, *h_ = nullptr;
    size_t d_bytes_ = 0, h_bytes_ = 0;
};

// The derivatives of every hypothesis of every set at its own points: num_point [sum of num_hyp] >= 0 in set order, rows and
// results concatenated in that order.  Each chunk of kDerivChunk points per hypothesis is ONE launch pair over every
// (set, hypothesis) that still has points -- the sets may be on different contexts of one device; it runs on the first
// set's stream, every other being idle (the entries are synchronous).  stage: room for the sum of num_hyp jobs.
int paired_derivs(Paired* const* sets, int num_set, PairDerivStage* stage, const int32_t* num_point, const double* pc1,
                  const double* pc2, const double* alpha, double* llk, double* grad, double* hess);

// The intervals of every hypothesis of every set in ONE IntervalGang (vb2_paired_interval): pc2_fixed [num_set][num_pc].
int paired_interval(Paired* const* sets, int num_set, const vb2_model& model, const double* pc2_fixed, const vb2_estimate* est,
                    vb2_interval* out, int32_t* status, int64_t* num_step, const char* const* labels = nullptr);

// The lock-step driver over any evaluator of a step (vb2_paired_lockstep; no device): hypothesis h's search is the
// reference-exact OptimizeLLK under `model` with is_heter = 0, its pc2 rows overwritten with pc2_fixed + h * k on their way
// to the evaluator, the llk0 call included.  A hypothesis whose first evaluation returns exactly 0.0 for every point walks
// no marker: its status is VB2_ERR_INVALID and the others go on.  The return value: a failure of the step (it ends every
// search).
int paired_lockstep(vb2_paired_eval_fn fn, void* user, int num_hyp, int num_pc, const vb2_model& model, const double* pc2_fixed,
                    vb2_estimate* est, int32_t* status);

}  // namespace vb2

struct vb2_paired {
    vb2::Paired* impl;
};

#endif
