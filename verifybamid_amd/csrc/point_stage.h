// point_stage.h -- the stage of a set that evaluates points of several rows (weight rows, hypotheses) over one context
// in launches of at most kMaxPointsPerLaunch points: one pinned slab and one device slab laid out
//     rows [cap][2k+1] | row indices [cap] | results [cap]        (on the device also: a launch's partial sums)
// with the fill, the upload, the chunked launches, the download and the event-timed loop.  The stage of every RowSet
// (row_set.h): Replicates, Conditioned and Paired.
#ifndef VB2_POINT_STAGE_H_
#define VB2_POINT_STAGE_H_

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <functional>

namespace vb2 {

class Context;

class PointStage {
public:
    // One launch pair of num_point <= kMaxPointsPerLaunch points on the stream: rows, the rows' indices, a launch's partial
    // sums, results.
    typedef std::function<hipError_t(int num_point, const double* d_rows, const int32_t* d_idx, double* d_partial, double* d_out,
                                     hipStream_t stream)>
        Launch;

    PointStage() {}
    PointStage(const PointStage&) = delete;
    PointStage& operator=(const PointStage&) = delete;
    ~PointStage();
    // cap points at most per evaluation, partial_doubles of scratch for a launch; the current device is ctx's.  nomem_who:
    // take_device's (device_util.h).
    int create(Context* ctx, size_t cap, size_t partial_doubles, const char* nomem_who);

    // The total of num_point[0..num_row), each within 0..VB2_BATCH_SLOTS; false: one is not.
    static bool count(int num_row, const int32_t* num_point, size_t* total);
    // Row r takes num_point[r] points, `total` in all; pc1, pc2, alpha concatenated in row order.  One upload, a launch per
    // kMaxPointsPerLaunch points on the context's stream (the partial sums are stream-ordered), one download: asynchronous.
    // Whatever it returns, end() leaves the stages free again.
    int begin(int num_row, const int32_t* num_point, size_t total, const double* pc1, const double* pc2, const double* alpha,
              const Launch& launch);
    // synchronises, and copies the results of the begun evaluation to llk (may be null); nothing begun: nothing done
    int end(double* llk);
    size_t pending() const { return pending_; }

    // Event-timed, milliseconds per repetition into ms[reps]: ONE launch of num_point points (pc = 0.01, alpha = 0.03),
    // point p under row p % num_row.
    int time_launch(int num_point, int num_row, int warmup, int reps, double* ms, const Launch& launch);

    size_t cap() const { return cap_; }
    size_t device_bytes() const { return d_bytes_; }
    int64_t num_step = 0, num_launch = 0;  // evaluations that reached the device, and their launches

private:
    Context* ctx_ = nullptr;
    void* d_ = nullptr;
    size_t d_bytes_ = 0;
    void* h_ = nullptr;                    // pinned: rows | row indices | results
    size_t h_bytes_ = 0;
    size_t cap_ = 0;
    size_t o_idx_ = 0, o_res_ = 0, o_part_ = 0;   // offsets into the stages (o_part_: device only)
    size_t pending_ = 0;                   // points of a begun evaluation
};

}  // namespace vb2
#endif
