// related_kernels.h -- the pairwise relatedness statistics of a cohort (related_kernels.hip).
#ifndef VB2_RELATED_KERNELS_H_
#define VB2_RELATED_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include "../../include/vb2_abi.h"
#include "source_kernels.h"

namespace vb2 {

// The floor of a marker's mixture k0 + k1 d1 + k2 d2: section 11's constant, the header's VB2_SOURCE_DOT_FLOOR in float32.
constexpr float kRelatedFloor = kSourceDotFloor;
constexpr int kNumRelation = VB2_NUM_RELATION;
static_assert(kNumRelation == 4 && VB2_REL_DUP == 0 && VB2_REL_PO == 1 && VB2_REL_FS == 2 && VB2_REL_D2 == 3,
              "the kernel forms the four mixtures in the header's order");

// The tiling is the source pair kernel's: kPairTile targets x kPairTile partners x one stripe of kPairStripe markers per
// workgroup, kPairChunk markers through LDS at a time.  Per pair and stripe the kernel leaves four FP64 sums of log2 and a
// count; the reduce kernel adds the stripes in stripe order and multiplies by ln 2.
inline size_t related_partial_count(int n, int64_t num_marker)
{
    return (size_t)n * (size_t)n * (size_t)source_num_stripe(num_marker);
}

// K of every ordered pair (target i, partner j) of the n rows.  d_rows[i]: device pointer to sample i's row, nullptr = none
// (NaN); a row holds its planes q | h | t, [num_marker][3] floats each, from float `q_offset` on.  part_k
// [related_partial_count][4] and part_n [related_partial_count] are scratch; llr [n][n][4], shared [n][n] in device memory.
hipError_t launch_related_pairs(const float* const* d_rows, size_t q_offset, int n, int64_t num_marker, double* part_k,
                                int32_t* part_n, double* llr, int32_t* shared, hipStream_t stream);

}  // namespace vb2

#endif
