// baq_stage.cpp -- see baq_stage.h.
#include "baq_stage.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "baq_kernels.h"
#include "context.h"   // set_error
#include "device_util.h"
#include "host_clock.h"
#include "tunables.h"

namespace vb2 {

namespace {

constexpr uint64_t kSlabLimit = 2ull << 30;      // the global tier's slabs together
constexpr int kGlobalGrid = 2048, kLdsGrid = 2048;      // workgroups of one wave: 12 fit a CU at the kernel's registers

}  // namespace

int BaqStage::init(const baq::Spans& spans, size_t max_rec, size_t max_bytes)
{
    max_rec_ = std::max<size_t>(max_rec, 1);
    max_bytes_ = std::max<size_t>(max_bytes, 1);
    span_bytes_ = spans.codes.size();
    VB2_HIP(hipMalloc(&d_spans_.p, std::max<size_t>(spans.codes.size(), 1)));
    VB2_HIP(hipMalloc(&d_tables_.p, sizeof(baq::Tables)));
    VB2_HIP(hipMalloc(&d_tasks_.p, max_rec_ * sizeof(baq::Task)));
    VB2_HIP(hipMalloc(&d_list_.p, max_rec_ * 4));
    VB2_HIP(hipMalloc(&d_adjq_.p, max_bytes_));
    VB2_HIP(hipMalloc(&d_cap4_.p, max_rec_ * 16));
    VB2_HIP(hipMalloc(&d_undef_.p, max_rec_ * 4));
    VB2_HIP(hipMalloc(&d_mapq_.p, max_rec_ * 2));
    for (OwnedEvent* e : {&ev_.begin, &ev_.mid, &ev_.end, &ev_.spare}) VB2_HIP(hipEventCreate(&e->e));
    if (!spans.codes.empty()) VB2_HIP(hipMemcpyAsync(d_spans_.p, spans.codes.data(), spans.codes.size(), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemcpyAsync(d_tables_.p, &baq::tables(), sizeof(baq::Tables), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipStreamSynchronize(s_));
    stats.seconds_fasta = spans.seconds;
    stats.fasta_bytes = spans.bytes_read;
    return VB2_OK;
}

// The batch's records into the tiers, by the workspace's formula: the LDS tier's records first in *list, the global tier's
// behind them, both in batch order; the global tier's grid and slab, grown when a record needs more.
int BaqStage::plan_tiers(const RecordBatch& batch, std::vector<uint32_t>* list_out, Tiers* t)
{
    const std::vector<baq::Task>& tasks = batch.tasks;
    const bamio::RecordDesc* const h_desc = batch.desc;
    const size_t nr = batch.nr;
    std::vector<uint32_t>& list = *list_out;
    const int kb = std::max(1, std::min(vb2::tunables().baq_lds_kb, 80));
    const uint32_t lds_bytes = (uint32_t)kb << 10;
    const uint64_t slice = (lds_bytes / kBaqGroups) & ~7ull;
    list.assign(nr, 0u);
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
            if (d_slab_.p) (void)hipFree(d_slab_.p);
            d_slab_.p = nullptr;
            slab_cap_ = 0;
            VB2_HIP(hipMalloc(&d_slab_.p, (size_t)want));
            slab_cap_ = (size_t)want;
        }
    }
    *t = Tiers{n_lds, n_glob, stride, slice, lds_bytes, grid_g};
    return VB2_OK;
}

int BaqStage::run(const RecordBatch& batch, const bamio::RecordDesc* d_desc, const uint8_t* d_data, BaqRecords* sink)
{
    const double t0 = now_s();
    const std::vector<baq::Task>& tasks = batch.tasks;
    const std::vector<uint8_t>& extra = batch.extra;
    const bamio::RecordDesc* const h_desc = batch.desc;
    const size_t nr = batch.nr, nb = batch.nb;
    if (nr > max_rec_ || nb > max_bytes_ || tasks.size() != nr) {
        set_error("--ApplyBAQ: internal error: a batch passes the stage's buffers");
        return VB2_ERR_INVALID;
    }
    if (nr == 0) return VB2_OK;
    std::vector<uint32_t> list;
    Tiers t;
    if (int rc = plan_tiers(batch, &list, &t)) return rc;
    const size_t n_lds = t.n_lds, n_glob = t.n_glob;
    if (extra.size() > extra_cap_) {
        if (d_extra_.p) (void)hipFree(d_extra_.p);
        d_extra_.p = nullptr;
        extra_cap_ = 0;
        VB2_HIP(hipMalloc(&d_extra_.p, extra.size()));
        extra_cap_ = extra.size();
    }
    VB2_HIP(hipMemcpyAsync(d_tasks_.p, tasks.data(), nr * sizeof(baq::Task), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemcpyAsync(d_list_.p, list.data(), nr * 4, hipMemcpyHostToDevice, s_));
    if (!extra.empty()) VB2_HIP(hipMemcpyAsync(d_extra_.p, extra.data(), extra.size(), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemsetAsync(d_cap4_.p, 0, nr * 16, s_));
    VB2_HIP(hipMemsetAsync(d_undef_.p, 0, nr * 4, s_));
    BaqBatch b;
    b.desc = d_desc;
    b.data = d_data;
    b.data_bytes = nb;
    b.tasks = d_tasks_.as<const baq::Task>();
    b.spans = d_spans_.as<const uint8_t>();
    b.span_bytes = span_bytes_;
    b.extra = d_extra_.as<const uint8_t>();
    b.extra_bytes = extra.size();
    b.tables = d_tables_.as<const baq::Tables>();
    b.illumina = opt_.illumina ? 1 : 0;
    b.adjq = d_adjq_.as<uint8_t>();
    b.cap4 = d_cap4_.as<int32_t>();
    b.undefined = d_undef_.as<int32_t>();
    const uint32_t* d_list = d_list_.as<const uint32_t>();
    VB2_HIP(hipEventRecord(ev_.begin.e, s_));
    VB2_HIP(launch_baq(b, d_list, (int64_t)n_lds, nullptr, t.slice, t.lds_bytes,
                       (int)std::min<size_t>((n_lds + kBaqGroups - 1) / kBaqGroups, (size_t)kLdsGrid), s_));
    VB2_HIP(hipEventRecord(ev_.mid.e, s_));
    VB2_HIP(launch_baq(b, d_list + n_lds, (int64_t)n_glob, d_slab_.as<uint8_t>(), t.stride, 0, t.grid_g, s_));
    VB2_HIP(hipEventRecord(ev_.end.e, s_));
    std::vector<int32_t> h_cap(nr * 4), h_undef(nr);
    VB2_HIP(hipMemcpyAsync(h_cap.data(), d_cap4_.p, nr * 16, hipMemcpyDeviceToHost, s_));
    VB2_HIP(hipMemcpyAsync(h_undef.data(), d_undef_.p, nr * 4, hipMemcpyDeviceToHost, s_));
    VB2_HIP(hipStreamSynchronize(s_));
    float ms = 0;
    VB2_HIP(hipEventElapsedTime(&ms, ev_.begin.e, ev_.mid.e));
    stats.seconds_lds += 1e-3 * ms;
    VB2_HIP(hipEventElapsedTime(&ms, ev_.mid.e, ev_.end.e));
    stats.seconds_global += 1e-3 * ms;
    // the cap's end on the host (libm), one mapQ per record back
    const double c0 = now_s();
    std::vector<int16_t> h_mapq(nr);
    std::vector<baq::Finished> ends(nr);
    for (size_t r = 0; r < nr; ++r) {
        ends[r] = baq::finish_record(h_desc[r].mapq, tasks[r], &h_cap[4 * r], opt_, &stats);
        h_mapq[r] = (int16_t)ends[r].mapq;
        stats.undefined_rows += h_undef[r];
    }
    VB2_HIP(hipMemcpyAsync(d_mapq_.p, h_mapq.data(), nr * 2, hipMemcpyHostToDevice, s_));
    std::vector<uint8_t> h_adjq;
    if (sink) {
        h_adjq.resize(nb);
        VB2_HIP(hipMemcpyAsync(h_adjq.data(), d_adjq_.p, nb, hipMemcpyDeviceToHost, s_));
    }
    VB2_HIP(hipStreamSynchronize(s_));
    stats.seconds_cap += now_s() - c0;
    if (sink)
        for (size_t r = 0; r < nr; ++r) {
            const bamio::RecordDesc& d = h_desc[r];      // (its qualities end its variable part)
            sink->append(h_adjq.data() + d.data + var_bytes(d) - (size_t)d.l_seq, d.l_seq, ends[r], &h_cap[4 * r]);
        }
    stats.seconds_stage += now_s() - t0;
    return VB2_OK;
}

}  // namespace vb2
