// bam_batches.h -- the upload batches of the built-in BAM reader: a scan's kept records cut into
// runs of at most `batch_bytes` bytes of variable parts (tunable bam_batch_kb) and `batch_rec` descriptors, the variable
// parts copied back to back and the descriptors rebased onto the batch.  With the spans of --ApplyBAQ a batch also carries
// its records' tasks.  The load's pileup and vb2_baq_records(where = 1) cut the same batches.
// Plain C++17 like bam_io.h and baq_host.h: no HIP header and nothing of context.h, so the caller sets the error
// (tests/bam_batches_check_main.cpp links the unit under the host sanitizers).
#ifndef VB2_BAM_BATCHES_H_
#define VB2_BAM_BATCHES_H_

#include <cstdint>
#include <string>
#include <vector>

#include "bam_io.h"
#include "baq_host.h"

namespace vb2 {

// a record's variable part: name, CIGAR, packed bases, qualities (the qualities are its last l_seq bytes)
inline size_t var_bytes(const bamio::RecordDesc& d)
{
    return (size_t)d.l_read_name + 4 * (size_t)d.n_cigar + ((size_t)d.l_seq + 1) / 2 + (size_t)d.l_seq;
}

// A batch closes when its bytes are full; its records are bounded by its bytes (a record has at least a name), or when
// its descriptors weigh as much as its bytes would.
struct BatchPlan {
    size_t batch_bytes = 0;      // max(bam_batch_kb << 10, the largest record's variable part)
    size_t batch_rec = 0;        // min(max(records, 1), max(batch_bytes / sizeof(RecordDesc), 1))
};
// bamio::kErrInvalid with "<who>: bam_batch_kb asks for batches of 4 GiB or more" in *err when batch_bytes > 0xfff00000
int plan_batches(const bamio::Scan& scan, int bam_batch_kb, const std::string& who, BatchPlan* plan, std::string* err);

// One cut batch.  bytes / desc / group are the caller's buffers (pinned or plain) of batch_bytes bytes and batch_rec
// entries; group may be null.  desc[r].data is the record's offset in bytes.  tasks / extra: filled under --ApplyBAQ,
// a kind-1 task's bq_off pointing at its BQ string in extra.
struct RecordBatch {
    uint8_t* bytes = nullptr;
    bamio::RecordDesc* desc = nullptr;
    uint16_t* group = nullptr;
    size_t nb = 0, nr = 0;
    std::vector<baq::Task> tasks;
    std::vector<uint8_t> extra;
};

// The records of a scan in order, chunk by chunk; empty chunks are skipped, and a scan without a record cuts no batch.
class BatchCursor {
public:
    // spans and opt: both (--ApplyBAQ) or neither
    BatchCursor(const bamio::Scan& scan, const BatchPlan& plan, const baq::Spans* spans = nullptr, const baq::Options* opt = nullptr);
    bool done() const { return ci_ >= scan_.chunks.size(); }
    // cuts the next batch into b's buffers; bamio::kErrInvalid with "<who>: internal error: a record passes its chunk"
    int next(RecordBatch* b, const std::string& who, std::string* err);

private:
    void skip_empty();
    const bamio::Scan& scan_;
    const BatchPlan plan_;
    const baq::Spans* spans_;
    const baq::Options* opt_;
    size_t ci_ = 0, ri_ = 0;     // next record: scan.chunks[ci].recs[ri]
};

}  // namespace vb2

#endif
