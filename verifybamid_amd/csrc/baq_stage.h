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
#include "bam_io.h"
#include "baq_host.h"

namespace vb2 {

class BaqStage {
public:
    BaqStage(const baq::Options& opt, hipStream_t s) : opt_(opt), s_(s) {}
    ~BaqStage();
    BaqStage(const BaqStage&) = delete;
    BaqStage& operator=(const BaqStage&) = delete;
    // the spans and the tables up; the buffers of a batch of at most max_rec records and max_bytes bytes
    int init(const baq::Spans& spans, size_t max_rec, size_t max_bytes);
    // One batch.  tasks / extra: of its records, in order; h_desc: its descriptors (host), d_desc / d_data: on the device.
    // Afterwards adjq() holds the adjusted qualities (at the offsets of d_data's) and adj_mapq() the mapQ per record, -1 =
    // dropped.  cap4 / mapq / outcome / qual (each may be null) get the batch's values appended (qual: per record its
    // l_seq adjusted qualities).
    int run(const std::vector<baq::Task>& tasks, const std::vector<uint8_t>& extra, const bamio::RecordDesc* h_desc, size_t nr,
            const bamio::RecordDesc* d_desc, const uint8_t* d_data, size_t nb, std::vector<int32_t>* cap4, std::vector<int16_t>* mapq,
            std::vector<uint8_t>* outcome, std::vector<uint8_t>* qual);
    const uint8_t* adjq() const { return static_cast<const uint8_t*>(d_adjq_); }
    const int16_t* adj_mapq() const { return static_cast<const int16_t*>(d_mapq_); }
    vb2_baq_stats stats{};

private:
    baq::Options opt_;
    hipStream_t s_;
    size_t max_rec_ = 0, max_bytes_ = 0, extra_cap_ = 0, slab_cap_ = 0;
    uint64_t span_bytes_ = 0;
    void *d_spans_ = nullptr, *d_tables_ = nullptr, *d_tasks_ = nullptr, *d_list_ = nullptr, *d_adjq_ = nullptr, *d_cap4_ = nullptr,
         *d_undef_ = nullptr, *d_mapq_ = nullptr, *d_extra_ = nullptr, *d_slab_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
};

}  // namespace vb2

#endif
