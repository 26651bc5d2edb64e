// source.h -- vb2_source_set internals (source.cpp): the float32 marginals of a cohort's samples on one device, their
// pairwise source scores (source_kernels.hip) and their pairwise relatedness statistics (related_kernels.hip).
#ifndef VB2_SOURCE_H_
#define VB2_SOURCE_H_

#include <hip/hip_runtime_api.h>

#include <mutex>
#include <string>
#include <vector>

#include "context.h"
#include "source_kernels.h"

namespace vb2 {

// The search point of `ctx`'s sample as a source set takes it (SourceSet::put), from the estimate a search under `model`
// reported: the reference's swap of indices 0 and 1 undone (as interval.cpp), then mirrored when the fit put the larger
// share first -- p1 [num_pc] is always the minor component's, *alpha (may be null) its share.
void search_point(const Context& ctx, const vb2_model& model, const vb2_estimate& est, std::vector<double>* p1,
                  std::vector<double>* p2, double* alpha);

class SourceSet {
public:
    // planes: VB2_SET_SOURCE (c q), VB2_SET_RELATED (q h t) or both (c q h t)
    static int create(int num_marker, int capacity, int device, SourceSet** out, int planes = VB2_SET_SOURCE);
    ~SourceSet();
    // the next free slot (add) or a given one (put: a cohort's samples retire in any order); thread-safe
    int add(Context* ctx, const vb2_model& model, const vb2_estimate& est, int* index);
    int put(int slot, Context* ctx, const vb2_model& model, const vb2_estimate& est);
    // slots [0, n) count as added, with or without a row (a cohort's failed samples: NaN)
    void set_count(int n);
    int count();
    int scores(double* score, int32_t* shared);
    // K [n][n][4] and shared [n][n] of a set with the related planes (related_kernels.hip)
    int relations(double* llr, int32_t* shared);
    int planes() const { return planes_; }
    // what a set of hypotheses reads of a sample (conditioned.cpp): the q plane [num_marker][3] of the slot's device row,
    // nullptr = the slot holds none
    int device() const { return device_; }
    int num_marker() const { return num_marker_; }
    const float* q_row(int slot)
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (slot < 0 || slot >= capacity_ || !rows_[(size_t)slot]) return nullptr;
        return rows_[(size_t)slot] + q_offset_;
    }
    // Measurement aids (tools/source_time.py; event-timed, milliseconds per repetition into ms[reps]): the pair kernels
    // over n synthetic rows (seeded non-negative triples; what was in the set is overwritten), and the marginal kernel of
    // a context into slot 0 (the row's memset included, as an add pays it).
    int time_pairs(int n, uint32_t seed, int warmup, int reps, double* ms, bool related = false);
    int time_marginals(Context* ctx, double alpha, int warmup, int reps, double* ms);

private:
    MarginalRelated planes_of(float* row) const;      // where the planes of a slot's row lie
    int device_ = -1, num_marker_ = 0, capacity_ = 0, n_ = 0, planes_ = VB2_SET_SOURCE;
    size_t row_floats_ = 0, q_offset_ = 0;            // floats of a row; where its q plane begins
    float* d_slab_ = nullptr;
    hipStream_t stream_ = nullptr;
    std::vector<const float*> rows_;         // [capacity] device rows, nullptr = none
    std::mutex mu_;
};

// <prefix>.Sources (vb2_cohort_run_sources): per sample its `top` best candidates by descending score
int write_sources(const std::string& prefix, int n, int top, const char* const* names, const vb2_run_result* res,
                  const int32_t* status, const double* score, const int32_t* shared);

// <prefix>.Related (vb2_cohort_run_related): per searched sample its `top` partners by descending max_r K_r
int write_related(const std::string& prefix, int n, int top, const char* const* names, const int32_t* status, const double* llr,
                  const int32_t* shared);

// <prefix>.SourceFit (vb2_cohort_run_source_fits): per searched sample with a first candidate the refit given it
int write_source_fit(const std::string& prefix, int n, const char* const* names, const vb2_source_fit* fit);

}  // namespace vb2

struct vb2_source_set {
    vb2::SourceSet* impl;
};

#endif
