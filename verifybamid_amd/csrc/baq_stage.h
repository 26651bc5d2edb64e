// baq_stage.h -- --ApplyBAQ between a batch's upload and its cover pass: the load's reference spans
// and tables on the device, per batch the tasks up, the two tiers' launches, the cap's four integers back, the cap finished
// on the host with libm, one adjusted mapQ per record up again.
#ifndef VB2_BAQ_STAGE_H_
#define VB2_BAQ_STAGE_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vb2_abi.h"
#include "bam_batches.h"
#include "baq_host.h"
#include "device_util.h"

namespace vb2 {

class BaqStage {
public:
    BaqStage(const baq::Options& opt, hipStream_t s) : opt_(opt), s_(s) {}
    BaqStage(const BaqStage&) = delete;
    BaqStage& operator=(const BaqStage&) = delete;
    // the spans and the tables up; the buffers of a batch of at most max_rec records and max_bytes bytes
    int init(const baq::Spans& spans, size_t max_rec, size_t max_bytes);
    // One batch of the cutter, with its tasks; d_desc / d_data: its descriptors and bytes on the device.  Afterwards
    // adjq() holds the adjusted qualities (at the offsets of d_data's) and adj_mapq() the mapQ per record, -1 = dropped.
    // sink (may be null) gets every record's adjusted qualities, mapQ, outcome and cap4 appended.
    int run(const RecordBatch& batch, const bamio::RecordDesc* d_desc, const uint8_t* d_data, BaqRecords* sink);
    const uint8_t* adjq() const { return d_adjq_.as<uint8_t>(); }
    const int16_t* adj_mapq() const { return d_mapq_.as<int16_t>(); }
    vb2_baq_stats stats{};

private:
    struct Tiers {
        size_t n_lds, n_glob;
        uint64_t stride, slice;        // bytes of workspace a global-tier record gets, and an LDS-tier one
        uint32_t lds_bytes;
        int grid_g;
    };
    int plan_tiers(const RecordBatch& batch, std::vector<uint32_t>* list, Tiers* t);
    baq::Options opt_;
    hipStream_t s_;
    size_t max_rec_ = 0, max_bytes_ = 0, extra_cap_ = 0, slab_cap_ = 0;
    uint64_t span_bytes_ = 0;
    // (members go in reverse order of declaration: the buffers from d_spans_ to d_slab_, then the events from begin to spare)
    struct Events {
        OwnedEvent spare, end, mid, begin;
    } ev_;
    DeviceBuffer d_slab_, d_extra_, d_mapq_, d_undef_, d_cap4_, d_adjq_, d_list_, d_tasks_, d_tables_, d_spans_;
};

}  // namespace vb2

#endif
