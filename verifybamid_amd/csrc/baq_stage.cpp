// baq_stage.cpp -- see baq_stage.h.
#include "baq_stage.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "baq_kernels.h"
#include "context.h"   // set_error
#include "device_util.h"
#include "tunables.h"

namespace vb2 {

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr uint64_t kSlabLimit = 2ull << 30;      // the global tier's slabs together
constexpr int kGlobalGrid = 2048, kLdsGrid = 2048;      // workgroups of one wave: 12 fit a CU at the kernel's registers

}  // namespace

BaqStage::~BaqStage()
{
    for (void* p : {d_spans_, d_tables_, d_tasks_, d_list_, d_adjq_, d_cap4_, d_undef_, d_mapq_, d_extra_, d_slab_})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : ev_)
        if (e) (void)hipEventDestroy(e);
}

int BaqStage::init(const baq::Spans& spans, size_t max_rec, size_t max_bytes)
{
    max_rec_ = std::max<size_t>(max_rec, 1);
    max_bytes_ = std::max<size_t>(max_bytes, 1);
    span_bytes_ = spans.codes.size();
    VB2_HIP(hipMalloc(&d_spans_, std::max<size_t>(spans.codes.size(), 1)));
    VB2_HIP(hipMalloc(&d_tables_, sizeof(baq::Tables)));
    VB2_HIP(hipMalloc(&d_tasks_, max_rec_ * sizeof(baq::Task)));
    VB2_HIP(hipMalloc(&d_list_, max_rec_ * 4));
    VB2_HIP(hipMalloc(&d_adjq_, max_bytes_));
    VB2_HIP(hipMalloc(&d_cap4_, max_rec_ * 16));
    VB2_HIP(hipMalloc(&d_undef_, max_rec_ * 4));
    VB2_HIP(hipMalloc(&d_mapq_, max_rec_ * 2));
    for (hipEvent_t& e : ev_) VB2_HIP(hipEventCreate(&e));
    if (!spans.codes.empty()) VB2_HIP(hipMemcpyAsync(d_spans_, spans.codes.data(), spans.codes.size(), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemcpyAsync(d_tables_, &baq::tables(), sizeof(baq::Tables), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipStreamSynchronize(s_));
    stats.seconds_fasta = spans.seconds;
    stats.fasta_bytes = spans.bytes_read;
    return VB2_OK;
}

int BaqStage::run(const std::vector<baq::Task>& tasks, const std::vector<uint8_t>& extra, const bamio::RecordDesc* h_desc, size_t nr,
                  const bamio::RecordDesc* d_desc, const uint8_t* d_data, size_t nb, std::vector<int32_t>* cap4, std::vector<int16_t>* mapq,
                  std::vector<uint8_t>* outcome, std::vector<uint8_t>* qual)
{
    const double t0 = now_s();
    if (nr > max_rec_ || nb > max_bytes_ || tasks.size() != nr) {
        set_error("--ApplyBAQ: internal error: a batch passes the stage's buffers");
        return VB2_ERR_INVALID;
    }
    if (nr == 0) return VB2_OK;
    const int kb = std::max(1, std::min(vb2::tunables().baq_lds_kb, 80));
    const uint32_t lds_bytes = (uint32_t)kb << 10;
    const uint64_t slice = (lds_bytes / kBaqGroups) & ~7ull;
    // the tiers, by the workspace's formula
    std::vector<uint32_t> list(nr);
    size_t n_lds = 0, n_glob = 0;
    uint64_t stride = 0;
    for (size_t r = 0; r < nr; ++r) {
        const uint64_t wb = tasks[r].kind == 2 ? baq::work_bytes(tasks[r].l_ref, h_desc[r].l_seq, tasks[r].bw) : 0;
        if (wb <= slice) {
            list[n_lds++] = (uint32_t)r;
        } else {
            list[nr - 1 - n_glob++] = (uint32_t)r;
            stride = std::max<uint64_t>(stride, (wb + 7) & ~7ull);
        }
        if (tasks[r].kind == 2) (wb <= slice ? stats.records_lds : stats.records_global) += 1;
    }
    std::reverse(list.begin() + (ptrdiff_t)n_lds, list.end());      // (the global tier in batch order too)
    int grid_g = (int)std::min<size_t>((n_glob + kBaqGroups - 1) / kBaqGroups, (size_t)kGlobalGrid);
    if (n_glob > 0) {
        while (grid_g > 1 && (uint64_t)grid_g * kBaqGroups * stride > kSlabLimit) grid_g /= 2;
        const uint64_t want = (uint64_t)grid_g * kBaqGroups * stride;
        if (want > kSlabLimit) {
            set_error("--ApplyBAQ: a read's alignment matrix needs " + std::to_string(stride) + " bytes: more than the stage gives one read");
            return VB2_ERR_NOMEM;
        }
        if (want > slab_cap_) {
            if (d_slab_) (void)hipFree(d_slab_);
            d_slab_ = nullptr;
            slab_cap_ = 0;
            VB2_HIP(hipMalloc(&d_slab_, (size_t)want));
            slab_cap_ = (size_t)want;
        }
    }
    if (extra.size() > extra_cap_) {
        if (d_extra_) (void)hipFree(d_extra_);
        d_extra_ = nullptr;
        extra_cap_ = 0;
        VB2_HIP(hipMalloc(&d_extra_, extra.size()));
        extra_cap_ = extra.size();
    }
    VB2_HIP(hipMemcpyAsync(d_tasks_, tasks.data(), nr * sizeof(baq::Task), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemcpyAsync(d_list_, list.data(), nr * 4, hipMemcpyHostToDevice, s_));
    if (!extra.empty()) VB2_HIP(hipMemcpyAsync(d_extra_, extra.data(), extra.size(), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemsetAsync(d_cap4_, 0, nr * 16, s_));
    VB2_HIP(hipMemsetAsync(d_undef_, 0, nr * 4, s_));
    BaqBatch b;
    b.desc = d_desc;
    b.data = d_data;
    b.data_bytes = nb;
    b.tasks = static_cast<const baq::Task*>(d_tasks_);
    b.spans = static_cast<const uint8_t*>(d_spans_);
    b.span_bytes = span_bytes_;
    b.extra = static_cast<const uint8_t*>(d_extra_);
    b.extra_bytes = extra.size();
    b.tables = static_cast<const baq::Tables*>(d_tables_);
    b.illumina = opt_.illumina ? 1 : 0;
    b.adjq = static_cast<uint8_t*>(d_adjq_);
    b.cap4 = static_cast<int32_t*>(d_cap4_);
    b.undefined = static_cast<int32_t*>(d_undef_);
    const uint32_t* d_list = static_cast<const uint32_t*>(d_list_);
    VB2_HIP(hipEventRecord(ev_[0], s_));
    VB2_HIP(launch_baq(b, d_list, (int64_t)n_lds, nullptr, slice, lds_bytes,
                       (int)std::min<size_t>((n_lds + kBaqGroups - 1) / kBaqGroups, (size_t)kLdsGrid), s_));
    VB2_HIP(hipEventRecord(ev_[1], s_));
    VB2_HIP(launch_baq(b, d_list + n_lds, (int64_t)n_glob, static_cast<uint8_t*>(d_slab_), stride, 0, grid_g, s_));
    VB2_HIP(hipEventRecord(ev_[2], s_));
    std::vector<int32_t> h_cap(nr * 4), h_undef(nr);
    VB2_HIP(hipMemcpyAsync(h_cap.data(), d_cap4_, nr * 16, hipMemcpyDeviceToHost, s_));
    VB2_HIP(hipMemcpyAsync(h_undef.data(), d_undef_, nr * 4, hipMemcpyDeviceToHost, s_));
    VB2_HIP(hipStreamSynchronize(s_));
    float ms = 0;
    VB2_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
    stats.seconds_lds += 1e-3 * ms;
    VB2_HIP(hipEventElapsedTime(&ms, ev_[1], ev_[2]));
    stats.seconds_global += 1e-3 * ms;
    // the cap's end on the host (libm), one mapQ per record back
    const double c0 = now_s();
    std::vector<int16_t> h_mapq(nr);
    for (size_t r = 0; r < nr; ++r) {
        int mq = h_desc[r].mapq;
        uint8_t oc = tasks[r].outcome;
        if (oc == baq::kOutside) {
            mq = -1;
        } else if (tasks[r].cap) {
            mq = baq::capped_mapq(mq, baq::cap_finish(&h_cap[4 * r], opt_.cap));
            if (mq < 0) oc = baq::kCapDropped;
        }
        h_mapq[r] = (int16_t)mq;
        stats.undefined_rows += h_undef[r];
        ++stats.records;
        switch (oc) {
        case baq::kRealigned: ++stats.realigned; break;
        case baq::kAlone: ++stats.left_alone; break;
        case baq::kTagApplied: ++stats.tag_applied; break;
        case baq::kNoReference: ++stats.no_reference; break;
        case baq::kOutside: ++stats.dropped_outside; break;
        case baq::kCapDropped: ++stats.dropped_cap; break;
        default: ++stats.not_asked; break;
        }
        if (outcome) outcome->push_back(oc);
    }
    VB2_HIP(hipMemcpyAsync(d_mapq_, h_mapq.data(), nr * 2, hipMemcpyHostToDevice, s_));
    std::vector<uint8_t> h_adjq;
    if (qual) {
        h_adjq.resize(nb);
        VB2_HIP(hipMemcpyAsync(h_adjq.data(), d_adjq_, nb, hipMemcpyDeviceToHost, s_));
    }
    VB2_HIP(hipStreamSynchronize(s_));
    stats.seconds_cap += now_s() - c0;
    if (cap4) cap4->insert(cap4->end(), h_cap.begin(), h_cap.end());
    if (mapq) mapq->insert(mapq->end(), h_mapq.begin(), h_mapq.end());
    if (qual)
        for (size_t r = 0; r < nr; ++r) {
            const bamio::RecordDesc& d = h_desc[r];
            const size_t at = (size_t)d.data + d.l_read_name + 4 * (size_t)d.n_cigar + ((size_t)d.l_seq + 1) / 2;
            qual->insert(qual->end(), h_adjq.begin() + (ptrdiff_t)at, h_adjq.begin() + (ptrdiff_t)(at + (size_t)d.l_seq));
        }
    stats.seconds_stage += now_s() - t0;
    return VB2_OK;
}

}  // namespace vb2
