// source_kernels.h -- per-marker genotype marginals of a sample at one point, and the pairwise source scores of a
// cohort (source_kernels.hip).
#ifndef VB2_SOURCE_KERNELS_H_
#define VB2_SOURCE_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include "../../include/vb2_abi.h"
#include "llk_kernels.h"

namespace vb2 {

// The floor of a marker's dot c_i . q_j in the score: bounds what one marker can veto (a genotyping error, a copy-number
// site) at log(1e-30) = -69 nats.  Part of the statistic's definition: ONE constant, the header's VB2_SOURCE_DOT_FLOOR; the
// kernel compares float32 dots against its float32 rounding (1.0000000031710769e-30: 3e-9 relative above 1e-30, four
// orders of magnitude inside the float32 evaluation's error bound of a floored marker).
constexpr float kSourceDotFloor = (float)VB2_SOURCE_DOT_FLOOR;
static_assert(kSourceDotFloor == 1e-30f && kSourceDotFloor >= 1.17549435e-38f,
              "the kernel's floor is the float32 rounding of VB2_SOURCE_DOT_FLOOR, a normal float");

// A sample's row in a set: two planes of float32, c[M][3] then q[M][3] (24 bytes per marker), zeros where the sample does
// not count the marker.
constexpr int kSourceRowFloats = 6;

// Pair kernel tiling: a workgroup takes kPairTile targets x kPairTile candidates x one stripe of the markers; the stripe's
// markers go through LDS kPairChunk at a time.  The stripe length is a constant: the partial sums of a pair -- one per
// stripe, added in stripe order by the second kernel -- are then the same whatever the set holds.
constexpr int kPairTile = 16;
constexpr int kPairChunk = 64;
constexpr int kPairStripe = 4096;
// Dots that share one logarithm: 1 -- every marker's dot takes its own (the error bound of the score then has no batching term)
constexpr int kPairLogBatch = 1;

// Enqueue the marginals of one point (row = pc1 | pc2 | alpha in device memory): contam_lik / geno_post [M][3] and log_l [M]
// in panel order (doubles; any may be nullptr), and/or the float32 set row.  pidx: sorted position -> panel marker
// ([num_active]).  The outputs must be zero-filled beforehand: only counted markers are written.
hipError_t launch_source_marginals(const DeviceLayout& L, int num_marker, const double* d_point, const int32_t* pidx,
                                   double* contam_lik, double* geno_post, double* log_l, float* row, hipStream_t stream);

// What the marginal kernel's related instantiation writes besides contam_lik / geno_post / log_l: the
// doubles own_lik = h and kin_post = t [M][3] in panel order, and the float32 planes [M][3] of a set row, each wherever the
// set keeps it.  Any may be nullptr; zero-filled beforehand like the other outputs.
struct MarginalRelated {
    double* own_lik = nullptr;
    double* kin_post = nullptr;
    float* c = nullptr;
    float* q = nullptr;
    float* h = nullptr;
    float* t = nullptr;
};
hipError_t launch_related_marginals(const DeviceLayout& L, int num_marker, const double* d_point, const int32_t* pidx,
                                    double* contam_lik, double* geno_post, double* log_l, const MarginalRelated& rel,
                                    hipStream_t stream);

inline int source_num_stripe(int64_t num_marker) { return (int)((num_marker + kPairStripe - 1) / kPairStripe); }
// entries of scratch (doubles in part_s, ints in part_n) for n samples
inline size_t source_partial_count(int n, int64_t num_marker) { return (size_t)n * (size_t)n * (size_t)source_num_stripe(num_marker); }

// Scores of every ordered pair (target i, candidate j) of the n rows (d_rows[i]: device pointer to sample i's row, nullptr =
// the sample has none: NaN): score[n][n], shared[n][n] in device memory.
hipError_t launch_source_pairs(const float* const* d_rows, int n, int64_t num_marker, double* part_s, int32_t* part_n,
                               double* score, int32_t* shared, hipStream_t stream);

}  // namespace vb2

#endif
