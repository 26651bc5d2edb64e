// bgzf_inflate_kernels.h -- BGZF blocks inflated on the device (bgzf_inflate_kernels.hip): the kernel's
// launcher over a job table, and the bamio::BlockInflater that feeds it in batches through one pinned staging buffer.
#ifndef VB2_BGZF_INFLATE_KERNELS_H_
#define VB2_BGZF_INFLATE_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "bam_io.h"

namespace vb2 {

// One BGZF block: its deflate payload at raw + raw_off, its inflated bytes to out + out_off.
struct InflateJob {
    uint64_t raw_off, out_off;
    uint32_t raw_len, isize;
};
static_assert(sizeof(InflateJob) == 24, "jobs are 24 bytes");

// One wave per job.  status[j] = a code of bgzf_inflate_core.h; out + out_off is written only where it is kDone.  A job
// that points outside [0, raw_bytes) or [0, out_bytes), or whose isize passes 65 536, is not run (kBadJob).
hipError_t launch_bgzf_inflate(const uint8_t* raw, uint64_t raw_bytes, const InflateJob* jobs, int32_t num_job, uint8_t* out,
                               uint64_t out_bytes, int32_t* status, hipStream_t s);

// What the device inflate of this process has done so far (every DeviceInflater adds to it; vb2_bgzf_inflate_stats).
struct InflateTotals {
    int64_t blocks = 0, batches = 0, bytes_raw = 0, bytes_inflated = 0, refused = 0;
    double seconds_upload = 0, seconds_kernel = 0, seconds_copyback = 0, seconds_stage = 0;
};
void inflate_totals(InflateTotals* out, bool reset);

// Batches of at most batch_bytes (raw payloads, and inflated bytes) through one pinned buffer of that size: upload, one
// launch, copy-back, then the inflated bytes into every item's dst.  Its buffers live as long as it does.
class DeviceInflater : public bamio::BlockInflater {
public:
    // device < 0: the current one.  stream: null = a stream of its own
    DeviceInflater(int device, hipStream_t stream, size_t batch_bytes);
    ~DeviceInflater() override;
    int run(const bamio::InflateItem* items, size_t n, int32_t* status, std::string* err) override;

private:
    int device_;
    hipStream_t stream_, own_stream_ = nullptr;
    size_t batch_bytes_, max_jobs_;
    void *h_stage_ = nullptr, *h_jobs_ = nullptr, *h_status_ = nullptr;
    void *d_raw_ = nullptr, *d_out_ = nullptr, *d_jobs_ = nullptr, *d_status_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    int init(std::string* err);
    bool ready_ = false;
};

// vb2_bgzf_inflate: the blocks of a buffer through a DeviceInflater, nothing else (no zlib, no CRC32).  A code of bam_io.h.
int bgzf_inflate_buffer(const uint8_t* bytes, uint64_t n, int device, size_t batch_bytes, uint8_t* out, int64_t out_capacity,
                        int64_t* out_bytes, int32_t* block_status, int32_t status_capacity, int32_t* num_block, std::string* err);

}  // namespace vb2

#endif
