// conditioned_kernels.h -- launchers of the likelihood conditioned on a hypothesised contaminant (conditioned_kernels.hip;
// DESIGN.md section 13).
#ifndef VB2_CONDITIONED_KERNELS_H_
#define VB2_CONDITIONED_KERNELS_H_

#include "llk_kernels.h"

namespace vb2 {

// tile groups (256 markers of the sorted order) of a layout: a point's partial sums, one per group
inline int conditioned_tile_groups(const DeviceLayout& L) { return (L.num_mt + 15) / 16; }
// floats of one hypothesis in the sorted order: three planes of m_pad
inline size_t conditioned_hyp_floats(const DeviceLayout& L) { return 3 * (size_t)L.m_pad; }

// panel-order prior rows d_panel [num_hyp][num_marker][3] -> the context's sorted order as planes d_planes
// [num_hyp][3][m_pad]; positions past the counted markers (the tiles' padding) and positions whose panel marker is out of
// range get 0.  pidx: sorted position -> panel marker (Context::ensure_pidx), [num_active].  d_panel is an upload or the q
// plane of a source set's row (one hypothesis per call then).
hipError_t launch_prior_permute(const DeviceLayout& L, int num_marker, int num_hyp, const float* d_panel, const int32_t* d_pidx,
                                float* d_planes, hipStream_t stream);

// LLK(. | h) at num_point <= kMaxPointsPerLaunch points: rows d_points [num_point][2k+1] (pc1 | pc2 | alpha), d_hyp[p] the
// hypothesis of point p in d_planes [..][3][m_pad].  d_partial: num_point * conditioned_tile_groups(L) doubles of scratch;
// d_out [num_point].  A point's value is the same bits whatever else the launch holds (one partial sum per tile group, then
// one fixed-order sum).
hipError_t launch_llk_conditioned(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_hyp,
                                  const float* d_planes, double* d_partial, double* d_out, hipStream_t stream);

}  // namespace vb2
#endif
