// errstat.h -- host side of the E-step of the error-rate fit (errstat_kernels.hip; vb2_abi.h section
// 3h): a device copy of a sample's RAW input and the evaluation of (n, s, llk) on it.  vb2_errstat_* of the C-ABI.
#ifndef VB2_ERRSTAT_H_
#define VB2_ERRSTAT_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/vb2_abi.h"
#include "errstat_kernels.h"

namespace vb2 {

// true: the table is there and every entry lies within [0, 1]; else the error text is set, `who` in front
bool err_table_ok(const double* err_table, const char* who);

class ErrStat {
public:
    ~ErrStat();
    static int create(const vb2_input* in, const vb2_options* opt, ErrStat** out);
    // n, s [94] and llk (any may be null) at the point under the table; synchronous
    int eval(const double* err_table, const double* pc1, const double* pc2, double alpha, int64_t* n, double* s, double* llk);

    int device = -1, num_cu = 0;
    int num_marker = 0, num_pc = 0;
    int64_t num_read = 0, device_bytes = 0, num_launch = 0;

private:
    ErrStat() = default;
    ErrStatInput in_{};
    hipStream_t stream_ = nullptr;
    bool own_stream_ = false;
    void* d_mem_ = nullptr;            // one slab: the sample, the point, the workgroups' bins, the groups' sums, the result
    size_t d_mem_bytes_ = 0;
    ErrStatPoint* d_point_ = nullptr;
    unsigned long long* d_slab_ = nullptr;
    double* d_partial_ = nullptr;
    unsigned long long* d_out_ = nullptr;
    int max_grid_ = 1;
};

}  // namespace vb2

struct vb2_errstat {
    vb2::ErrStat* impl;
};

#endif
