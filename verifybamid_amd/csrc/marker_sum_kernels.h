// marker_sum_kernels.h -- launchers of the three per-marker sums over one resident sample (marker_sum_kernels.hip): the
// weighted-marker evaluation, the likelihood conditioned on a hypothesised contaminant (section 13)
// and the likelihood given priors on both components (section 16).
#ifndef VB2_MARKER_SUM_KERNELS_H_
#define VB2_MARKER_SUM_KERNELS_H_

#include "llk_kernels.h"

namespace vb2 {

// tile groups (256 markers of the sorted order) of a layout: a point's partial sums, one per group
int marker_sum_tile_groups(const DeviceLayout& L);
// floats of one hypothesis in the sorted order: three planes of m_pad
inline size_t conditioned_hyp_floats(const DeviceLayout& L) { return 3 * (size_t)L.m_pad; }

// panel-order weight rows [num_rep][num_marker] -> the context's sorted order [num_rep][m_pad]; positions past the counted
// markers (the tiles' padding) get 0.  pidx: sorted position -> panel marker (Context::ensure_pidx), [num_active].
hipError_t launch_weights_permute(const DeviceLayout& L, int num_marker, int num_rep, const uint8_t* d_panel,
                                  const int32_t* d_pidx, uint8_t* d_sorted, hipStream_t stream);

// panel-order prior rows d_panel [num_hyp][num_marker][3] -> the context's sorted order as planes d_planes
// [num_hyp][3][m_pad]; positions past the counted markers (the tiles' padding) and positions whose panel marker is out of
// range get 0.  d_panel is an upload or the q plane of a source set's row (one hypothesis per call then).
hipError_t launch_prior_permute(const DeviceLayout& L, int num_marker, int num_hyp, const float* d_panel, const int32_t* d_pidx,
                                float* d_planes, hipStream_t stream);

// LLK_w at num_point <= kMaxPointsPerLaunch points: rows d_points [num_point][2k+1] (pc1 | pc2 | alpha), d_row[p] the weight
// row of point p in d_weights [..][m_pad].  d_partial: num_point * marker_sum_tile_groups(L) doubles of scratch; d_out
// [num_point].  A point's value is the same bits whatever else the launch holds (one partial sum per tile group, then one
// fixed-order sum).
hipError_t launch_llk_weighted(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_row,
                               const uint8_t* d_weights, double* d_partial, double* d_out, hipStream_t stream);

// LLK(. | h) the same way: d_hyp[p] the hypothesis of point p in d_planes [..][3][m_pad].
hipError_t launch_llk_conditioned(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_hyp,
                                  const float* d_planes, double* d_partial, double* d_out, hipStream_t stream);

// The pair hypotheses of DESIGN.md section 16: floats of one hypothesis in the sorted order, six planes of m_pad (pi1[0..2],
// pi2[0..2]).
inline size_t paired_hyp_floats(const DeviceLayout& L) { return 6 * (size_t)L.m_pad; }
// panel-order rows d_panel [num_hyp][num_marker][6] (pi1 | pi2) -> planes d_planes [num_hyp][6][m_pad]; the tiles' padding
// and positions whose panel marker is out of range get 0 (no counted marker: never read).
hipError_t launch_pair_permute(const DeviceLayout& L, int num_marker, int num_hyp, const float* d_panel, const int32_t* d_pidx,
                               float* d_planes, hipStream_t stream);
// ONE hypothesis's planes from the q plane d_q [num_marker][3] of a source set's row: pi1 all zero; pi2 = q where the triple
// is not all zero and max(q[0], q[2]) >= hom_min; every other counted position left out (pi2 = -1, 0, 0).
hipError_t launch_pair_build(const DeviceLayout& L, int num_marker, const float* d_q, const int32_t* d_pidx, double hom_min,
                             float* d_planes, hipStream_t stream);
// LLK(. | h) with a prior on either component: d_hyp[p] the hypothesis of point p in d_planes [..][6][m_pad]; a position
// whose pi2[0] is negative is not walked.
hipError_t launch_llk_paired(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_hyp,
                             const float* d_planes, double* d_partial, double* d_out, hipStream_t stream);

}  // namespace vb2
#endif
