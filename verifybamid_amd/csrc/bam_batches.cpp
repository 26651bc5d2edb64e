// bam_batches.cpp -- see bam_batches.h.
#include "bam_batches.h"

#include <algorithm>
#include <cstring>

namespace vb2 {

int plan_batches(const bamio::Scan& scan, int bam_batch_kb, const std::string& who, BatchPlan* plan, std::string* err)
{
    size_t largest = 0, total_rec = 0;
    for (const bamio::Chunk& ch : scan.chunks) {
        total_rec += ch.recs.size();
        for (const bamio::RecordDesc& d : ch.recs) largest = std::max(largest, var_bytes(d));
    }
    plan->batch_bytes = std::max<size_t>((size_t)std::max(bam_batch_kb, 1) << 10, largest);
    if (plan->batch_bytes > 0xfff00000ull) {
        *err = who + ": bam_batch_kb asks for batches of 4 GiB or more";
        return bamio::kErrInvalid;
    }
    plan->batch_rec = std::min<size_t>(std::max<size_t>(total_rec, 1), std::max<size_t>(plan->batch_bytes / sizeof(bamio::RecordDesc), 1));
    return bamio::kOk;
}

BatchCursor::BatchCursor(const bamio::Scan& scan, const BatchPlan& plan, const baq::Spans* spans, const baq::Options* opt)
    : scan_(scan), plan_(plan), spans_(spans), opt_(opt)
{
    skip_empty();
}

void BatchCursor::skip_empty()
{
    while (ci_ < scan_.chunks.size() && ri_ >= scan_.chunks[ci_].recs.size()) {
        ++ci_;
        ri_ = 0;
    }
}

int BatchCursor::next(RecordBatch* b, const std::string& who, std::string* err)
{
    b->nb = b->nr = 0;
    b->tasks.clear();
    b->extra.clear();
    while (ci_ < scan_.chunks.size() && b->nr < plan_.batch_rec) {
        const bamio::Chunk& ch = scan_.chunks[ci_];
        const bamio::RecordDesc& d = ch.recs[ri_];
        const size_t vb = var_bytes(d);
        if ((size_t)d.data > ch.bytes.size() || vb > ch.bytes.size() - d.data) {      // (bam_io.cpp has checked this)
            *err = who + ": internal error: a record passes its chunk";
            return bamio::kErrInvalid;
        }
        if (b->nb + vb > plan_.batch_bytes) break;
        std::memcpy(b->bytes + b->nb, ch.bytes.data() + d.data, vb);
        b->desc[b->nr] = d;
        b->desc[b->nr].data = (uint32_t)b->nb;
        if (b->group) b->group[b->nr] = ri_ < ch.group.size() ? ch.group[ri_] : bamio::kNoGroup;
        if (spans_) {
            const uint8_t* bq = nullptr;
            baq::Task t = baq::make_task(scan_, ci_, ri_, *spans_, *opt_, &bq);
            if (t.kind == 1 && bq) {
                t.bq_off = (uint32_t)b->extra.size();
                b->extra.insert(b->extra.end(), bq, bq + d.l_seq);
            }
            b->tasks.push_back(t);
        }
        b->nb += vb;
        ++b->nr;
        ++ri_;
        skip_empty();
    }
    return bamio::kOk;
}

}  // namespace vb2
