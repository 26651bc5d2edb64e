// weighted_kernels.h -- launchers of the weighted-marker evaluation (weighted_kernels.hip).
#ifndef VB2_WEIGHTED_KERNELS_H_
#define VB2_WEIGHTED_KERNELS_H_

#include "llk_kernels.h"

namespace vb2 {

// tile groups (256 markers of the sorted order) of a layout: a point's partial sums, one per group
inline int weighted_tile_groups(const DeviceLayout& L) { return (L.num_mt + 15) / 16; }

// panel-order weight rows [num_rep][num_marker] -> the context's sorted order [num_rep][m_pad]; positions past the counted
// markers (the tiles' padding) get 0.  pidx: sorted position -> panel marker (Context::ensure_pidx), [num_active].
hipError_t launch_weights_permute(const DeviceLayout& L, int num_marker, int num_rep, const uint8_t* d_panel,
                                  const int32_t* d_pidx, uint8_t* d_sorted, hipStream_t stream);

// LLK_w at num_point <= kMaxPointsPerLaunch points: rows d_points [num_point][2k+1] (pc1 | pc2 | alpha), d_row[p] the weight
// row of point p in d_weights [..][m_pad].  d_partial: num_point * weighted_tile_groups(L) doubles of scratch; d_out [num_point].
// A point's value is the same bits whatever else the launch holds (one partial sum per tile group, then one fixed-order sum).
hipError_t launch_llk_weighted(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_row,
                               const uint8_t* d_weights, double* d_partial, double* d_out, hipStream_t stream);

}  // namespace vb2
#endif
