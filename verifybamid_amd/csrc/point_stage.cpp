// point_stage.cpp -- see point_stage.h
#include "point_stage.h"

#include <algorithm>
#include <cstring>

#include "context.h"
#include "device_util.h"

namespace vb2 {

int PointStage::create(Context* ctx, size_t cap, size_t partial_doubles, const char* nomem_who)
{
    ctx_ = ctx;
    cap_ = cap;
    const int k = ctx->num_pc;
    o_idx_ = up256(sizeof(double) * cap * (size_t)(2 * k + 1));
    o_res_ = up256(o_idx_ + sizeof(int32_t) * cap);
    o_part_ = up256(o_res_ + sizeof(double) * cap);
    if (const int rc = take_device(o_part_ + sizeof(double) * partial_doubles, ctx->device, &d_, &d_bytes_, nomem_who)) return rc;
    h_ = cached_pinned_slab(o_part_, ctx->device, &h_bytes_);
    if (!h_) {
        VB2_HIP(hipHostMalloc(&h_, o_part_, hipHostMallocMapped));
        h_bytes_ = o_part_;
    }
    return VB2_OK;
}

PointStage::~PointStage()
{
    if (!ctx_) return;
    (void)hipSetDevice(ctx_->device);
    if (pending_) (void)hipStreamSynchronize(ctx_->stream);
    give_device(d_, d_bytes_, ctx_->device);
    if (h_ && !recycle_pinned_slab(h_, h_bytes_, ctx_->device)) (void)hipHostFree(h_);
}

bool PointStage::count(int num_row, const int32_t* num_point, size_t* total)
{
    *total = 0;
    for (int r = 0; r < num_row; ++r) {
        if (num_point[r] < 0 || num_point[r] > VB2_BATCH_SLOTS) return false;
        *total += (size_t)num_point[r];
    }
    return true;
}

int PointStage::begin(int num_row, const int32_t* num_point, size_t total, const double* pc1, const double* pc2,
                      const double* alpha, const Launch& launch)
{
    VB2_HIP(hipSetDevice(ctx_->device));
    const int k = ctx_->num_pc, n = 2 * k + 1;
    char* const hp = static_cast<char*>(h_);
    char* const dp = static_cast<char*>(d_);
    double* const h_rows = reinterpret_cast<double*>(hp);
    int32_t* const h_idx = reinterpret_cast<int32_t*>(hp + o_idx_);
    size_t p = 0;
    for (int r = 0; r < num_row; ++r)
        for (int b = 0; b < num_point[r]; ++b, ++p) {
            double* row = h_rows + p * n;
            std::memcpy(row, pc1 + p * k, sizeof(double) * k);
            std::memcpy(row + k, pc2 + p * k, sizeof(double) * k);
            row[2 * k] = alpha[p];
            h_idx[p] = r;
        }
    hipStream_t s = ctx_->stream;
    pending_ = total;                      // (from here on the stream may hold work on the stages)
    VB2_HIP(hipMemcpyAsync(dp, hp, sizeof(double) * total * n, hipMemcpyHostToDevice, s));
    VB2_HIP(hipMemcpyAsync(dp + o_idx_, hp + o_idx_, sizeof(int32_t) * total, hipMemcpyHostToDevice, s));
    for (size_t done = 0; done < total; done += kMaxPointsPerLaunch) {
        const int c = (int)std::min<size_t>(kMaxPointsPerLaunch, total - done);
        VB2_HIP(launch(c, reinterpret_cast<const double*>(dp) + done * n, reinterpret_cast<const int32_t*>(dp + o_idx_) + done,
                       reinterpret_cast<double*>(dp + o_part_), reinterpret_cast<double*>(dp + o_res_) + done, s));
        ++num_launch;
    }
    VB2_HIP(hipMemcpyAsync(hp + o_res_, dp + o_res_, sizeof(double) * total, hipMemcpyDeviceToHost, s));
    return VB2_OK;
}

int PointStage::end(double* llk)
{
    if (!pending_) return VB2_OK;
    const size_t total = pending_;
    pending_ = 0;
    VB2_HIP(hipSetDevice(ctx_->device));
    VB2_HIP(hipStreamSynchronize(ctx_->stream));
    ++num_step;
    if (llk) std::memcpy(llk, static_cast<const char*>(h_) + o_res_, sizeof(double) * total);
    return VB2_OK;
}

int PointStage::time_launch(int num_point, int num_row, int warmup, int reps, double* ms, const Launch& launch)
{
    if (num_point < 1 || num_point > kMaxPointsPerLaunch || (size_t)num_point > cap_ || warmup < 0 || reps < 1 || !ms ||
        ctx_->resident_active || pending_) {
        set_error("time_launch: invalid argument");
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipSetDevice(ctx_->device));
    const int k = ctx_->num_pc, n = 2 * k + 1;
    char* const hp = static_cast<char*>(h_);
    char* const dp = static_cast<char*>(d_);
    double* const h_rows = reinterpret_cast<double*>(hp);
    int32_t* const h_idx = reinterpret_cast<int32_t*>(hp + o_idx_);
    for (int p = 0; p < num_point; ++p) {
        for (int j = 0; j < 2 * k; ++j) h_rows[(size_t)p * n + j] = 0.01;
        h_rows[(size_t)p * n + 2 * k] = 0.03;
        h_idx[p] = p % num_row;
    }
    hipStream_t s = ctx_->stream;
    VB2_HIP(hipMemcpyAsync(dp, hp, sizeof(double) * (size_t)num_point * n, hipMemcpyHostToDevice, s));
    VB2_HIP(hipMemcpyAsync(dp + o_idx_, hp + o_idx_, sizeof(int32_t) * (size_t)num_point, hipMemcpyHostToDevice, s));
    TimerEvents ev;
    VB2_HIP(hipEventCreate(&ev.a));
    VB2_HIP(hipEventCreate(&ev.b));
    for (int r = -warmup; r < reps; ++r) {
        VB2_HIP(hipEventRecord(ev.a, s));
        VB2_HIP(launch(num_point, reinterpret_cast<const double*>(dp), reinterpret_cast<const int32_t*>(dp + o_idx_),
                       reinterpret_cast<double*>(dp + o_part_), reinterpret_cast<double*>(dp + o_res_), s));
        VB2_HIP(hipEventRecord(ev.b, s));
        VB2_HIP(hipEventSynchronize(ev.b));
        float t = 0.0f;
        VB2_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
        if (r >= 0) ms[r] = (double)t;
    }
    return VB2_OK;
}

}  // namespace vb2
