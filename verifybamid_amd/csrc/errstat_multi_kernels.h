// errstat_multi_kernels.h -- launcher of the batched E-step of the error-rate fit (errstat_multi_kernels.hip; DESIGN.md
// section 24): what errstat_kernels.h computes for one sample, for up to 64 samples in one launch pair, every sample at its
// own point under its own error table.  Every word it returns for a sample is the word launch_errstat returns for that
// sample alone at the same point and table, whatever the grid and whatever else the launch holds.
#ifndef VB2_ERRSTAT_MULTI_KERNELS_H_
#define VB2_ERRSTAT_MULTI_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "errstat_kernels.h"

namespace vb2 {

constexpr int kErrMultiMaxSample = 64;             // samples of one launch
constexpr int kErrMultiMaxGrid = 64;               // workgroups one sample takes at most
// reads of a marker group that are staged in LDS at a time (two bytes each); a group of 256 markers at depth 30 is one
// chunk, a deeper one takes several and is staged twice, once per pass.  A multiple of 16.
constexpr int kErrMultiChunk = 8192;

// one sample with work in the launch: workgroups wg_first .. wg_first + wg_count walk its marker groups in stripes, group g
// leaves its log-likelihood in partial[grp_first + g]; the result goes to out[sample * kErrOutWords ..]
struct ErrMultiJob {
    ErrStatInput in;
    const ErrStatPoint* point;
    int sample;
    int wg_first, wg_count;
    int grp_first;
};

// d_jobs [num_job], d_wg_job [grid]: the job of every workgroup (grid = the sum of the jobs' wg_count); d_slab: grid *
// kErrBinWords words; d_partial: the sum of the jobs' groups; d_out: num_sample * kErrOutWords words, zeroed here first, so
// that a sample without a job reads zeros and a log-likelihood of 0.  The reduce runs one workgroup per job.
hipError_t launch_errstat_multi(const ErrMultiJob* d_jobs, int num_job, const int* d_wg_job, int grid, int num_sample,
                                unsigned long long* d_slab, double* d_partial, unsigned long long* d_out, hipStream_t stream);

}  // namespace vb2
#endif
