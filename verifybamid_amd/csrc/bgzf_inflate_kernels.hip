// bgzf_inflate_kernels.hip -- BGZF blocks inflated on the device (bgzf_inflate_kernels.h).
//
// bgzf_inflate_kernel: one wave -- a workgroup of 64 threads -- per BGZF block.  The decoder is bgzf_inflate_core.h, the one
// the CPU check runs under the host sanitizers.  All 64 lanes run it in step on the same bits: its state is the same in
// every lane (the payload's bytes and the tables are read at wave-uniform addresses, which the memory pipes broadcast), so
// there is no divergence, no lane to wait for and nothing to hand from lane to lane.  The work that has width is shared:
//   * a literal is stored by lane 0;
//   * a match, a stored block's run and the final flush are copied by the wave, lane l taking bytes l, l + 64, ...
//     A match at a distance below its length repeats the last `dist` bytes: byte i comes from byte i mod dist of the
//     window BEFORE the match, which the copy does not write, so the lanes need no order among themselves.
// The block's output is staged in LDS (64 KiB: a BGZF block's ISIZE is at most 65 536 and its window is its own output),
// beside the code-length and symbol tables (1 080 bytes): 66 616 bytes per workgroup, two workgroups per CU.  LDS
// operations of one wave complete in order, so a lane reads what another lane of its wave stored before without a
// barrier; the wavefront-scope fences keep the compiler to that order.  The flush to global memory is coalesced, 16 bytes
// per lane where the output is aligned.  Nothing is written to global memory for a block whose status is not kDone.
// No array in a local variable: no scratch (tests/test_bgzf_inflate_cpu.py reads the code object's notes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bgzf_inflate_core.h"
#include "bgzf_inflate_kernels.h"

namespace vb2 {
namespace {

constexpr uint32_t kWave = 64;

struct GlobalSource {
    const uint8_t* p;
    __device__ uint8_t operator[](uint32_t i) const { return p[i]; }
};

__device__ inline void wave_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

struct WaveSink {
    uint8_t* w;          // the window in LDS
    uint32_t lane;
    __device__ void put(uint32_t at, uint8_t b)
    {
        if (lane == 0) w[at] = b;
    }
    __device__ void copy_back(uint32_t at, uint32_t dist, uint32_t len)
    {
        wave_order();
        const uint8_t* from = w + (at - dist);
        for (uint32_t i = lane; i < len; i += kWave) w[at + i] = from[i < dist ? i : i % dist];
        wave_order();
    }
    __device__ void copy_in(uint32_t at, const GlobalSource& s, uint32_t from, uint32_t len)
    {
        wave_order();
        for (uint32_t i = lane; i < len; i += kWave) w[at + i] = s.p[from + i];
        wave_order();
    }
};

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ raw, uint64_t raw_bytes,
                                                          const InflateJob* __restrict__ jobs, int32_t num_job,
                                                          uint8_t* __restrict__ out, uint64_t out_bytes, int32_t* __restrict__ status)
{
    __shared__ uint4 window[bgzf::kMaxIsize / 16];
    __shared__ bgzf::Tables tables;
    const uint32_t j = blockIdx.x;
    if (j >= (uint32_t)num_job) return;
    const uint32_t lane = threadIdx.x;
    const InflateJob job = jobs[j];
    if (job.isize > bgzf::kMaxIsize || job.raw_off > raw_bytes || job.raw_len > raw_bytes - job.raw_off || job.out_off > out_bytes ||
        job.isize > out_bytes - job.out_off) {
        if (lane == 0) status[j] = bgzf::kBadJob;
        return;
    }
    const GlobalSource src{raw + job.raw_off};
    WaveSink sink{reinterpret_cast<uint8_t*>(window), lane};
    const int32_t st = bgzf::inflate(src, job.raw_len, sink, job.isize, tables);
    wave_order();
    if (st == bgzf::kDone) {
        uint8_t* o = out + job.out_off;
        const uint8_t* w = reinterpret_cast<const uint8_t*>(window);
        uint32_t done = 0;
        if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
            const uint32_t n16 = job.isize >> 4;
            for (uint32_t i = lane; i < n16; i += kWave) reinterpret_cast<uint4*>(o)[i] = window[i];
            done = n16 << 4;
        }
        for (uint32_t i = done + lane; i < job.isize; i += kWave) o[i] = w[i];
    }
    if (lane == 0) status[j] = st;
}

std::mutex g_totals_mu;
InflateTotals g_totals;

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

hipError_t launch_bgzf_inflate(const uint8_t* raw, uint64_t raw_bytes, const InflateJob* jobs, int32_t num_job, uint8_t* out,
                               uint64_t out_bytes, int32_t* status, hipStream_t s)
{
    if (num_job <= 0) return hipSuccess;
    bgzf_inflate_kernel<<<(uint32_t)num_job, kWave, 0, s>>>(raw, raw_bytes, jobs, num_job, out, out_bytes, status);
    return hipGetLastError();
}

void inflate_totals(InflateTotals* out, bool reset)
{
    std::lock_guard<std::mutex> g(g_totals_mu);
    if (out) *out = g_totals;
    if (reset) g_totals = InflateTotals();
}

DeviceInflater::DeviceInflater(int device, hipStream_t stream, size_t batch_bytes)
    : device_(device), stream_(stream), batch_bytes_(std::max<size_t>(align16(batch_bytes), (size_t)1 << 17))
{
    // (a batch holds at least one block: 64 KiB of payload, 64 KiB inflated)
    max_jobs_ = std::max<size_t>(1024, batch_bytes_ >> 10);
}

DeviceInflater::~DeviceInflater()
{
    if (device_ >= 0) (void)hipSetDevice(device_);
    for (hipEvent_t& e : ev_)
        if (e) (void)hipEventDestroy(e);
    if (h_stage_) (void)hipHostFree(h_stage_);
    if (h_jobs_) (void)hipHostFree(h_jobs_);
    if (h_status_) (void)hipHostFree(h_status_);
    if (d_raw_) (void)hipFree(d_raw_);
    if (d_out_) (void)hipFree(d_out_);
    if (d_jobs_) (void)hipFree(d_jobs_);
    if (d_status_) (void)hipFree(d_status_);
    if (own_stream_) (void)hipStreamDestroy(own_stream_);
}

#define VB2_INFL_HIP(call)                                                                                    \
    do {                                                                                                      \
        const hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                               \
            if (err) *err = std::string("device inflate: ") + #call + ": " + hipGetErrorString(e_);         \
            return e_ == hipErrorOutOfMemory ? bamio::kErrNoMem : bamio::kErrIo;                              \
        }                                                                                                     \
    } while (0)

int DeviceInflater::init(std::string* err)
{
    if (ready_) return bamio::kOk;
    if (device_ >= 0) VB2_INFL_HIP(hipSetDevice(device_));
    if (!stream_) {
        VB2_INFL_HIP(hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking));
        stream_ = own_stream_;
    }
    VB2_INFL_HIP(hipHostMalloc(&h_stage_, batch_bytes_, hipHostMallocDefault));
    VB2_INFL_HIP(hipHostMalloc(&h_jobs_, max_jobs_ * sizeof(InflateJob), hipHostMallocDefault));
    VB2_INFL_HIP(hipHostMalloc(&h_status_, max_jobs_ * sizeof(int32_t), hipHostMallocDefault));
    VB2_INFL_HIP(hipMalloc(&d_raw_, batch_bytes_));
    VB2_INFL_HIP(hipMalloc(&d_out_, batch_bytes_));
    VB2_INFL_HIP(hipMalloc(&d_jobs_, max_jobs_ * sizeof(InflateJob)));
    VB2_INFL_HIP(hipMalloc(&d_status_, max_jobs_ * sizeof(int32_t)));
    for (hipEvent_t& e : ev_) VB2_INFL_HIP(hipEventCreate(&e));
    ready_ = true;
    return bamio::kOk;
}

int DeviceInflater::run(const bamio::InflateItem* items, size_t n, int32_t* status, std::string* err)
{
    if (n == 0) return bamio::kOk;
    if (const int rc = init(err)) return rc;
    if (device_ >= 0) VB2_INFL_HIP(hipSetDevice(device_));
    uint8_t* const stage = static_cast<uint8_t*>(h_stage_);
    InflateJob* const jobs = static_cast<InflateJob*>(h_jobs_);
    const int32_t* const h_status = static_cast<const int32_t*>(h_status_);
    InflateTotals add;
    size_t k = 0;
    while (k < n) {
        // a batch: payloads back to back, outputs back to back at multiples of 16 bytes
        size_t nj = 0, raw_at = 0, out_at = 0;
        while (k + nj < n && nj < max_jobs_) {
            const bamio::InflateItem& it = items[k + nj];
            if (it.isize > bgzf::kMaxIsize || it.raw_len > batch_bytes_) {          // (a BGZF block's payload is below 64 KiB)
                if (err) *err = "device inflate: a block of more than 65 536 bytes";
                return bamio::kErrInvalid;
            }
            if (raw_at + it.raw_len > batch_bytes_ || out_at + it.isize > batch_bytes_) break;
            jobs[nj] = InflateJob{(uint64_t)raw_at, (uint64_t)out_at, it.raw_len, it.isize};
            if (it.raw_len) std::memcpy(stage + raw_at, it.raw, it.raw_len);
            raw_at += it.raw_len;
            out_at = align16(out_at + it.isize);
            ++nj;
        }
        const size_t out_used = std::min(out_at, batch_bytes_);
        VB2_INFL_HIP(hipEventRecord(ev_[0], stream_));
        if (raw_at) VB2_INFL_HIP(hipMemcpyAsync(d_raw_, stage, raw_at, hipMemcpyHostToDevice, stream_));
        VB2_INFL_HIP(hipMemcpyAsync(d_jobs_, jobs, nj * sizeof(InflateJob), hipMemcpyHostToDevice, stream_));
        VB2_INFL_HIP(hipEventRecord(ev_[1], stream_));
        VB2_INFL_HIP(launch_bgzf_inflate(static_cast<const uint8_t*>(d_raw_), raw_at, static_cast<const InflateJob*>(d_jobs_), (int32_t)nj,
                                         static_cast<uint8_t*>(d_out_), out_used, static_cast<int32_t*>(d_status_), stream_));
        VB2_INFL_HIP(hipEventRecord(ev_[2], stream_));
        // (the payloads have gone up by the time the kernel has run: the staging buffer takes the inflated bytes)
        if (out_used) VB2_INFL_HIP(hipMemcpyAsync(stage, d_out_, out_used, hipMemcpyDeviceToHost, stream_));
        VB2_INFL_HIP(hipMemcpyAsync(h_status_, d_status_, nj * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        VB2_INFL_HIP(hipEventRecord(ev_[3], stream_));
        VB2_INFL_HIP(hipStreamSynchronize(stream_));
        float ms[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) VB2_INFL_HIP(hipEventElapsedTime(&ms[i], ev_[i], ev_[i + 1]));
        const double t_host = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        for (size_t i = 0; i < nj; ++i) {
            const bamio::InflateItem& it = items[k + i];
            status[k + i] = h_status[i];
            if (h_status[i] == bgzf::kDone) {
                if (it.isize) std::memcpy(it.dst, stage + jobs[i].out_off, it.isize);
                add.bytes_inflated += it.isize;
            } else {
                ++add.refused;
            }
            add.bytes_raw += it.raw_len;
        }
        add.seconds_stage += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t_host;
        add.seconds_upload += 1e-3 * ms[0];
        add.seconds_kernel += 1e-3 * ms[1];
        add.seconds_copyback += 1e-3 * ms[2];
        add.blocks += (int64_t)nj;
        ++add.batches;
        k += nj;
    }
    {
        std::lock_guard<std::mutex> g(g_totals_mu);
        g_totals.blocks += add.blocks;
        g_totals.batches += add.batches;
        g_totals.bytes_raw += add.bytes_raw;
        g_totals.bytes_inflated += add.bytes_inflated;
        g_totals.refused += add.refused;
        g_totals.seconds_upload += add.seconds_upload;
        g_totals.seconds_kernel += add.seconds_kernel;
        g_totals.seconds_copyback += add.seconds_copyback;
        g_totals.seconds_stage += add.seconds_stage;
    }
    return bamio::kOk;
}

int bgzf_inflate_buffer(const uint8_t* bytes, uint64_t n, int device, size_t batch_bytes, uint8_t* out, int64_t out_capacity,
                        int64_t* out_bytes, int32_t* block_status, int32_t status_capacity, int32_t* num_block, std::string* err)
{
    std::vector<bamio::BlockSpan> blocks;
    if (const int rc = bamio::list_bgzf_blocks(bytes, n, "vb2_bgzf_inflate: the buffer", &blocks, err)) return rc;
    uint64_t total = 0;
    for (const bamio::BlockSpan& b : blocks) total += b.isize;
    *out_bytes = (int64_t)total;
    *num_block = (int32_t)std::min<size_t>(blocks.size(), 0x7fffffff);
    if (blocks.size() > 0x7fffffffull || (int64_t)total > out_capacity || (int64_t)blocks.size() > (int64_t)status_capacity) {
        if (err) *err = "vb2_bgzf_inflate: " + std::to_string(blocks.size()) + " blocks of " + std::to_string(total) +
                        " bytes do not fit the caller's arrays";
        return bamio::kErrInvalid;
    }
    if (total) std::memset(out, 0, (size_t)total);
    std::vector<bamio::InflateItem> items(blocks.size());
    uint64_t at = 0;
    for (size_t i = 0; i < blocks.size(); ++i) {
        items[i] = bamio::InflateItem{bytes + blocks[i].raw_off, blocks[i].raw_len, out + at, blocks[i].isize};
        block_status[i] = bgzf::kNotRun;
        at += blocks[i].isize;
    }
    DeviceInflater inflater(device, nullptr, batch_bytes);
    return inflater.run(items.data(), items.size(), block_status, err);
}

}  // namespace vb2
