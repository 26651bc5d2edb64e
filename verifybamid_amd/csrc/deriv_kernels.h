// deriv_kernels.h -- derivatives of the genotype-mixture log-likelihood on the device (deriv_kernels.hip).
#ifndef VB2_DERIV_KERNELS_H_
#define VB2_DERIV_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include "llk_kernels.h"

namespace vb2 {

// Per marker and point, the read-loop kernel writes these ten scalars (0 for a marker whose likelihood L is not > 0, h:310):
// log L, then with x, y in {1 = AF of pc1 (contaminant), 2 = AF of pc2 (intended), a = alpha}:
//   l_1, l_2, l_a, l_11, l_22, l_12, l_1a, l_2a, l_aa    (l_x = L_x / L, l_xy = L_xy / L - l_x l_y)
constexpr int kDerivVals = 10;
// Points per pass of the two kernels: the scratch of a context holds kDerivChunk x kDerivVals x m_pad doubles
constexpr int kDerivChunk = 4;

// Outputs per point of the reduction: the LLK, the gradient (n = 2k + 1 entries, order pc1[0..k) pc2[0..k) alpha) and the upper
// triangle of the Hessian, row by row
__host__ __device__ inline int deriv_out_count(int k) { const int n = 2 * k + 1; return 1 + n + n * (n + 1) / 2; }
// doubles of device scratch a context needs (per-marker scalars, parameter rows, outputs of one chunk)
inline size_t deriv_scratch_doubles(const DeviceLayout& L)
{
    return (size_t)kDerivChunk * ((size_t)kDerivVals * (size_t)L.m_pad + (size_t)(2 * L.num_pc + 1) + (size_t)deriv_out_count(L.num_pc));
}

// Enqueue the derivatives of num_point <= kDerivChunk rows (pc1 | pc2 | alpha, device memory) on stream: d_out receives
// deriv_out_count(k) doubles per point.  d_marker: kDerivChunk x kDerivVals x m_pad doubles of scratch.
hipError_t launch_llk_derivs(const DeviceLayout& L, int num_point, const double* d_points, double* d_marker, double* d_out,
                             hipStream_t stream);

// One sample's share of a launch pair that serves several samples: its layout, num_point <= kDerivChunk parameter rows, its own
// scratch (kDerivChunk x kDerivVals x m_pad doubles) and where its deriv_out_count(k) doubles per point go.  All device memory.
struct DerivJob {
    DeviceLayout L;
    const double* points;
    double* marker;
    double* out;
    int32_t num_point;
    int32_t reserved;
};
// Enqueue the derivatives of num_job jobs on stream as one launch of the marker kernel per layout class present and one of
// the reduction.  h_jobs: the table as the host wrote it (probability-domain jobs first), d_jobs: where it is -- or will be,
// stream-ordered before this call -- on the device.  Every point's results are launch_llk_derivs' bits.
hipError_t launch_llk_derivs_multi(const DerivJob* h_jobs, const DerivJob* d_jobs, int num_job, hipStream_t stream);

// The derivatives of LLK(. | h) for a pair hypothesis (DESIGN.md sections 16 and 17): d_planes its six planes [6][m_pad] in
// the layout's sorted order (pi1[0..2] | pi2[0..2], marker_sum_kernels.h).  A marker whose pi2[0] is negative is not walked
// and adds ten zeros; a side whose triple is not all zero takes it for its prior and has no derivative in its PCs there.
// The same scratch, outputs and reduction as launch_llk_derivs; all-zero planes give its bits.
hipError_t launch_llk_pair_derivs(const DeviceLayout& L, int num_point, const double* d_points, const float* d_planes,
                                  double* d_marker, double* d_out, hipStream_t stream);
// ... and of several (context, hypothesis) jobs in one launch pair: job j's hypothesis is d_planes[j] (a table in device
// memory beside d_jobs, in the jobs' order).  Two hypotheses of one context are two jobs with that context's layout and
// marker scratch of their own.  Every point's results are launch_llk_pair_derivs' bits.
hipError_t launch_llk_pair_derivs_multi(const DerivJob* h_jobs, const DerivJob* d_jobs, const float* const* d_planes, int num_job,
                                        hipStream_t stream);

}  // namespace vb2

#endif
