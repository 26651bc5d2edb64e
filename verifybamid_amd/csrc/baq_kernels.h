// baq_kernels.h -- the device stage of --ApplyBAQ (baq_kernels.hip): per record of an uploaded batch
// the adjusted qualities and the four integers of the mapping-quality cap.
#ifndef VB2_BAQ_KERNELS_H_
#define VB2_BAQ_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "bam_io.h"
#include "baq_host.h"

namespace vb2 {

constexpr int kBaqLanes = 16, kBaqGroups = 4;      // lanes per record, records per wave (one wave per workgroup)

struct BaqBatch {
    const bamio::RecordDesc* desc;      // the batch's descriptors ...
    const uint8_t* data;                // ... and bytes
    uint64_t data_bytes;
    const baq::Task* tasks;             // parallel to desc
    const uint8_t* spans;               // the load's reference spans, nt16 codes
    uint64_t span_bytes;
    const uint8_t* extra;               // the batch's BQ strings
    uint64_t extra_bytes;
    const baq::Tables* tables;
    int32_t illumina;
    uint8_t* adjq;                      // data_bytes: a record's adjusted qualities where `data` has its qualities
    int32_t* cap4;                      // 4 per record
    int32_t* undefined;                 // per record
};

// One tier's records: list[0 .. n) are record numbers of the batch.  slab == null: the LDS tier, every record's workspace
// fits lds_bytes / kBaqGroups; else the global tier, workgroup w's lane group g owns slab + (w * kBaqGroups + g) * stride.
hipError_t launch_baq(const BaqBatch& b, const uint32_t* list, int64_t n, uint8_t* slab, uint64_t stride, uint32_t lds_bytes,
                      int grid, hipStream_t s);

}  // namespace vb2

#endif
