// errstat_kernels.h -- launcher of the E-step of the error-rate fit (errstat_kernels.hip; vb2_abi.h
// section 3h): per reported quality the reads of the counted markers and the expected number of error reads among them, at
// one point (pc1, pc2, alpha) under one error table.  It walks the RAW input -- the context's layouts have folded class
// "other" into a constant and merged neighbouring qualities into window rows, and both are needed apart here.
#ifndef VB2_ERRSTAT_KERNELS_H_
#define VB2_ERRSTAT_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace vb2 {

constexpr int kErrNumQual = 94;                    // clamped qualities 0..93 (ContaminationEstimator.h:65-74, 296-298)
constexpr int kErrMaxPc = 64;                      // VB2_MAX_PC
constexpr int kErrThreads = 256;                   // one thread per marker, 256 markers of the panel order per group
// per quality three 64-bit integers: reads, and the expected errors in fixed point, sum floor(r 2^32) and sum of the next 32
// bits of every r
constexpr int kErrBinWords = 3 * kErrNumQual;
constexpr int kErrOutWords = kErrBinWords + 1;     // ... and the log-likelihood's bits

// the raw sample on the device, in panel order
struct ErrStatInput {
    int num_marker, num_pc;
    const uint8_t* bases;          // [R]
    const uint8_t* quals;          // [R]
    const int64_t* read_off;       // [M + 1], relative to the first read
    const uint8_t* alt_base;       // [M]
    const double* ud;              // [M][k] row-major, or null with known_af
    const double* mu;              // [M]
    const double* known_af;        // [M] or null
    double avg_depth, sd_depth;
    int sanity_disabled;
};

// what one evaluation reads beside the sample: err [94], pc1 [64], pc2 [64], alpha
struct ErrStatPoint {
    double err[kErrNumQual];
    double pc1[kErrMaxPc], pc2[kErrMaxPc];
    double alpha;
};

inline int errstat_groups(int num_marker) { return (num_marker + kErrThreads - 1) / kErrThreads; }

// grid workgroups (1..errstat_groups) walk the marker groups in stripes.  d_slab: grid * kErrBinWords words, d_partial:
// errstat_groups doubles; d_out [kErrOutWords]: the bins summed over the workgroups, then the log-likelihood.  Every word of
// d_out is the same bits whatever the grid: the bins are integer sums, the log-likelihood one fixed tree per marker group
// and one fixed-order sum over the groups.
hipError_t launch_errstat(const ErrStatInput& in, const ErrStatPoint* d_point, int grid, unsigned long long* d_slab,
                          double* d_partial, unsigned long long* d_out, hipStream_t stream);

}  // namespace vb2
#endif
