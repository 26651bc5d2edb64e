// errstat.h -- host side of the E-step of the error-rate fit (errstat_kernels.hip; vb2_abi.h section
// 3h): a device copy of a sample's RAW input and the evaluation of (n, s, llk) on it; and the same for up to 64 samples in
// one launch pair (errstat_multi_kernels.hip).  vb2_errstat_* of the C-ABI.
#ifndef VB2_ERRSTAT_H_
#define VB2_ERRSTAT_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/vb2_abi.h"
#include "errstat_kernels.h"
#include "errstat_multi_kernels.h"

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

// Up to 64 samples' raw inputs on one device and their E-steps in one launch pair, every sample at its own point under its
// own table.  Inputs whose ud / means / known_af pointers (and shapes) are equal share one device copy: the samples of a
// cohort share the panel.  What it returns for a sample is ErrStat::eval's bits for that sample alone.
class ErrStatBatch {
public:
    ~ErrStatBatch();
    // in[s] null: a sample that holds nothing (it takes no workgroup and reads zeros)
    static int create(const vb2_input* const* in, int num_sample, const vb2_options* opt, ErrStatBatch** out);
    // live [S] or null (all); err_tables [S][94]; pc1, pc2 [S][num_pc] (null when every sample has known AF); alpha [S];
    // n [S][94], s [S][94], llk [S] (any may be null).  A sample that is not live, or holds no marker, reads zeros.
    int eval(const int32_t* live, const double* err_tables, const double* pc1, const double* pc2, const double* alpha, int64_t* n,
             double* s, double* llk);

    int device = -1, num_cu = 0;
    int num_sample = 0, num_pc = 0;            // num_pc: the largest of the samples' (the stride of pc1 / pc2)
    int num_panel = 0;                         // distinct device copies of (ud, means) or known_af
    int64_t num_marker = 0, num_read = 0, device_bytes = 0, num_launch = 0, num_eval = 0;
    int last_grid = 0;                         // workgroups of the last marker launch

private:
    ErrStatBatch() = default;
    struct Sample {
        ErrStatInput in{};
        int ngrp = 0, grp_first = 0;
        bool known_af = false;
    };
    Sample sample_[kErrMultiMaxSample];
    hipStream_t stream_ = nullptr;
    bool own_stream_ = false;
    void* d_mem_ = nullptr;
    size_t d_mem_bytes_ = 0;
    // what an evaluation uploads, in one piece: the points, the jobs, the workgroups' jobs
    char* d_up_ = nullptr;
    size_t up_bytes_ = 0, o_jobs_ = 0, o_wg_ = 0;
    char* h_up_ = nullptr;                     // its host image
    unsigned long long* h_out_ = nullptr;
    unsigned long long* d_slab_ = nullptr;
    double* d_partial_ = nullptr;
    unsigned long long* d_out_ = nullptr;
    int max_grid_ = 1;
};

}  // namespace vb2

struct vb2_errstat {
    vb2::ErrStat* impl;
};

struct vb2_errstat_batch {
    vb2::ErrStatBatch* impl;
};

#endif
