// derivs.cpp -- host side of the LLK's derivatives (deriv_kernels.hip): Context::derivs_host and vb2_llk_derivs_batch.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"
#include "deriv_kernels.h"

namespace vb2 {

#define VB2_HIP_D(call)                                                                \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_error(std::string(#call) + " failed: " + hipGetErrorString(e_));       \
            return VB2_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

int Context::derivs_host(int num_point, const double* pc1, const double* pc2, const double* alpha, double* llk, double* grad,
                         double* hess)
{
    if (num_point < 0 || (num_point > 0 && (!pc1 || !pc2 || !alpha || !llk || !grad || !hess))) {
        set_error("vb2_llk_derivs_batch: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (num_point == 0) return VB2_OK;
    if (resident_active) {
        set_error("vb2_llk_derivs_batch: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    VB2_HIP_D(hipSetDevice(device));
    const int k = num_pc, n = 2 * k + 1, nout = deriv_out_count(k);
    // scratch: once per context, through the slab cache ([chunk][kDerivVals][m_pad] | [chunk][2k+1] | [chunk][nout])
    if (!d_deriv) {
        const size_t bytes = deriv_scratch_doubles(L) * sizeof(double);
        size_t got = 0;
        void* p = cached_device_slab(bytes, device, &got);
        if (!p) {
            VB2_HIP_D(hipMalloc(&p, bytes));
            got = bytes;
        }
        d_deriv = static_cast<double*>(p);
        d_deriv_bytes = got;
    }
    double* const d_marker = d_deriv;
    double* const d_rows = d_marker + (size_t)kDerivChunk * kDerivVals * (size_t)L.m_pad;
    double* const d_res = d_rows + (size_t)kDerivChunk * n;
    // every chunk is enqueued before the one synchronisation: the scratch is stream-ordered, the host rows and results
    // have a slot per point
    std::vector<double> rows((size_t)num_point * n), res((size_t)num_point * nout);
    for (int b = 0; b < num_point; ++b) {
        double* row = rows.data() + (size_t)b * n;
        std::memcpy(row, pc1 + (size_t)b * k, sizeof(double) * k);
        std::memcpy(row + k, pc2 + (size_t)b * k, sizeof(double) * k);
        row[2 * k] = alpha[b];
    }
    for (int done = 0; done < num_point; done += kDerivChunk) {
        const int c = std::min(kDerivChunk, num_point - done);
        VB2_HIP_D(hipMemcpyAsync(d_rows, rows.data() + (size_t)done * n, sizeof(double) * (size_t)c * n, hipMemcpyHostToDevice,
                                 stream));
        VB2_HIP_D(launch_llk_derivs(L, c, d_rows, d_marker, d_res, stream));
        VB2_HIP_D(hipMemcpyAsync(res.data() + (size_t)done * nout, d_res, sizeof(double) * (size_t)c * nout,
                                 hipMemcpyDeviceToHost, stream));
    }
    VB2_HIP_D(hipStreamSynchronize(stream));
    for (int pb = 0; pb < num_point; ++pb) {
        const double* r = res.data() + (size_t)pb * nout;
        llk[pb] = r[0];
        std::memcpy(grad + (size_t)pb * n, r + 1, sizeof(double) * n);
        double* h = hess + (size_t)pb * n * n;
        int e = 1 + n;
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j, ++e) h[(size_t)i * n + j] = h[(size_t)j * n + i] = r[e];
    }
    return VB2_OK;
}

}  // namespace vb2
