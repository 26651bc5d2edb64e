// derivs.cpp -- host side of the LLK's derivatives (deriv_kernels.hip): Context::derivs_host (vb2_llk_derivs_batch) and, for
// several samples in one launch pair, Batch::derivs (vb2_batch_derivs).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch.h"
#include "context.h"
#include "deriv_kernels.h"
#include "device_util.h"

namespace vb2 {

// scratch: once per context, through the slab cache ([chunk][kDerivVals][m_pad] | [chunk][2k+1] | [chunk][nout])
int Context::ensure_deriv_scratch()
{
    VB2_HIP(hipSetDevice(device));
    if (d_deriv) return VB2_OK;
    const size_t bytes = deriv_scratch_doubles(L) * sizeof(double);
    size_t got = 0;
    void* p = cached_device_slab(bytes, device, &got);
    if (!p) {
        VB2_HIP(hipMalloc(&p, bytes));
        got = bytes;
    }
    d_deriv = static_cast<double*>(p);
    d_deriv_bytes = got;
    return VB2_OK;
}

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
    if (const int rc = ensure_deriv_scratch()) return rc;
    const int k = num_pc, n = 2 * k + 1, nout = deriv_out_count(k);
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
        VB2_HIP(hipMemcpyAsync(d_rows, rows.data() + (size_t)done * n, sizeof(double) * (size_t)c * n, hipMemcpyHostToDevice,
                                 stream));
        VB2_HIP(launch_llk_derivs(L, c, d_rows, d_marker, d_res, stream));
        VB2_HIP(hipMemcpyAsync(res.data() + (size_t)done * nout, d_res, sizeof(double) * (size_t)c * nout,
                                 hipMemcpyDeviceToHost, stream));
    }
    VB2_HIP(hipStreamSynchronize(stream));
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

namespace {
// where the pieces of a step lie, in the pinned slab and (the first two) in the device slab alike
struct DerivStage {
    size_t o_jobs, o_rows, o_res, up_bytes, total;
    DerivStage(int S, int k)
    {
        const size_t n = 2 * (size_t)k + 1;
        o_jobs = 0;
        o_rows = (sizeof(DerivJob) * (size_t)S + 255) & ~(size_t)255;
        up_bytes = o_rows + sizeof(double) * (size_t)S * kDerivChunk * n;
        o_res = (up_bytes + 255) & ~(size_t)255;
        total = o_res + sizeof(double) * (size_t)S * kDerivChunk * (size_t)deriv_out_count(k);
    }
};
}

int Batch::ensure_deriv_resources()
{
    VB2_HIP(hipSetDevice(device));
    for (Context* c : ctx_)
        if (c)
            if (const int rc = c->ensure_deriv_scratch()) return rc;
    if (dv_pin_) return VB2_OK;
    const DerivStage st(num_sample, num_pc);
    if (!stream_) {
        stream_ = cached_stream(device);
        if (!stream_) VB2_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    }
    dv_dev_ = cached_device_slab(st.total, device, &dv_dev_bytes_);
    if (!dv_dev_) {
        VB2_HIP(hipMalloc(&dv_dev_, st.total));
        dv_dev_bytes_ = st.total;
    }
    void* pin = cached_pinned_slab(st.total, device, &dv_pin_bytes_);
    if (!pin) {
        VB2_HIP(hipHostMalloc(&pin, st.total, hipHostMallocMapped));
        dv_pin_bytes_ = st.total;
    }
    dv_pin_ = pin;
    return VB2_OK;
}

int Batch::derivs(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk, double* grad,
                  double* hess)
{
    if (!num_point) {
        set_error("vb2_batch_derivs: invalid argument");
        return VB2_ERR_INVALID;
    }
    const int S = num_sample, k = num_pc, n = 2 * k + 1, nout = deriv_out_count(k);
    std::vector<size_t> first((size_t)S + 1, 0);
    int most = 0;
    for (int s = 0; s < S; ++s) {
        if (num_point[s] < 0 || (num_point[s] > 0 && !ctx_[s])) {
            set_error("vb2_batch_derivs: a negative point count, or points for an empty slot");
            return VB2_ERR_INVALID;
        }
        if (num_point[s] > 0 && ctx_[s]->resident_active) {
            set_error("vb2_batch_derivs: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
            return VB2_ERR_INVALID;
        }
        first[s + 1] = first[s] + (size_t)num_point[s];
        most = std::max(most, (int)num_point[s]);
    }
    if (most == 0) return VB2_OK;
    if (!pc1 || !pc2 || !alpha || !llk || !grad || !hess) {
        set_error("vb2_batch_derivs: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (in_flight_) {
        set_error("vb2_batch_derivs: an evaluation step of the batch is in flight");
        return VB2_ERR_INVALID;
    }
    if (const int rc = ensure_deriv_resources()) return rc;
    const DerivStage st(S, k);
    char* const hp = static_cast<char*>(dv_pin_);
    char* const dp = static_cast<char*>(dv_dev_);
    DerivJob* const h_jobs = reinterpret_cast<DerivJob*>(hp + st.o_jobs);
    double* const h_rows = reinterpret_cast<double*>(hp + st.o_rows);
    const double* const h_res = reinterpret_cast<const double*>(hp + st.o_res);
    std::vector<int> who(S);
    for (int done = 0; done < most; done += kDerivChunk) {
        // this step's jobs: the probability-domain samples first (one marker launch per layout class)
        int nj = 0;
        for (int cls = 1; cls >= 0; --cls)
            for (int s = 0; s < S; ++s)
                if (num_point[s] > done && (ctx_[s]->L.pd != 0) == (cls != 0)) who[nj++] = s;
        for (int j = 0; j < nj; ++j) {
            const int s = who[j];
            Context* c = ctx_[s];
            const int cnt = std::min(kDerivChunk, num_point[s] - done);
            DerivJob& job = h_jobs[j];
            job.L = c->L;
            job.L.stamps = nullptr;
            job.points = reinterpret_cast<const double*>(dp + st.o_rows) + (size_t)j * kDerivChunk * n;
            job.marker = c->d_deriv;
            job.out = reinterpret_cast<double*>(dp + st.o_res) + (size_t)j * kDerivChunk * nout;
            job.num_point = cnt;
            job.reserved = 0;
            for (int b = 0; b < cnt; ++b) {
                const size_t src = first[s] + (size_t)done + (size_t)b;
                double* row = h_rows + ((size_t)j * kDerivChunk + b) * n;
                std::memcpy(row, pc1 + src * k, sizeof(double) * k);
                std::memcpy(row + k, pc2 + src * k, sizeof(double) * k);
                row[2 * k] = alpha[src];
            }
        }
        const size_t up = st.o_rows + sizeof(double) * (size_t)nj * kDerivChunk * n;
        VB2_HIP(hipMemcpyAsync(dp, hp, up, hipMemcpyHostToDevice, stream_));
        VB2_HIP(launch_llk_derivs_multi(h_jobs, reinterpret_cast<const DerivJob*>(dp + st.o_jobs), nj, stream_));
        VB2_HIP(hipMemcpyAsync(hp + st.o_res, dp + st.o_res, sizeof(double) * (size_t)nj * kDerivChunk * nout,
                                 hipMemcpyDeviceToHost, stream_));
        VB2_HIP(hipStreamSynchronize(stream_));
        ++num_deriv_step;
        for (int j = 0; j < nj; ++j) {
            const int s = who[j];
            const int cnt = std::min(kDerivChunk, num_point[s] - done);
            for (int b = 0; b < cnt; ++b) {
                const size_t dst = first[s] + (size_t)done + (size_t)b;
                const double* r = h_res + ((size_t)j * kDerivChunk + b) * nout;
                llk[dst] = r[0];
                std::memcpy(grad + dst * n, r + 1, sizeof(double) * n);
                double* h = hess + dst * n * n;
                int e = 1 + n;
                for (int i = 0; i < n; ++i)
                    for (int jj = i; jj < n; ++jj, ++e) h[(size_t)i * n + jj] = h[(size_t)jj * n + i] = r[e];
            }
        }
    }
    return VB2_OK;
}

}  // namespace vb2
