// refbias_kernels.h -- launcher of the per-marker sum whose TABLE depends on a second scalar, the reference bias beta of
// the row a point belongs to (refbias_kernels.hip; vb2_abi.h section 3g).
#ifndef VB2_REFBIAS_KERNELS_H_
#define VB2_REFBIAS_KERNELS_H_

#include "llk_kernels.h"

namespace vb2 {

constexpr double kBiasMin = 0.25, kBiasMax = 0.75;       // the domain of beta
// table row strides in doubles: probability domain -- the six off-diagonal pairs and (het, het) at beta, then the same
// seven at 1 - beta (112 bytes, seven 16-byte slots: odd); run words -- seven logarithms per code
constexpr int kBiasRowDoublesPd = 14, kBiasRowDoublesRun = 7;

// LLK(pc1, pc2, alpha; beta) at num_point <= kMaxPointsPerLaunch points: rows d_points [num_point][2k+1] (pc1 | pc2 |
// alpha), d_row[p] the row of point p in d_beta [..] (one double per row, within [kBiasMin, kBiasMax]: the caller's
// check).  d_partial: num_point * marker_sum_tile_groups(L) doubles of scratch; d_out [num_point].  A point's value is the
// same bits whatever else the launch holds (one partial sum per tile group, then one fixed-order sum).
hipError_t launch_llk_bias(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_row,
                           const double* d_beta, double* d_partial, double* d_out, hipStream_t stream);

}  // namespace vb2
#endif
