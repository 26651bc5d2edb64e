// bam_flatten.cpp -- BAM/CRAM -> per-marker pileup on the host, the
// "SimplePileupViewer runs once on host" stage of BASELINE.json's north_star for --BamFile input.
//
// Behaviour restated from the reference (file:line relative to the reference root):
//   read filter + BAQ + mapQ cap       SimplePileupViewer.cpp:172-237 (mplp_func)
//   per-region pileup over the panel   SimplePileupViewer.cpp:245-557 (SimplePileup)
//   base characters                    SimplePileupViewer.cpp:25-62   (pileup_seq)
//   defaults                           main.cpp:81-96: min-MQ 2, min-BQ 13, adjust-MQ (capQ) 40,
//                                      max depth 8000, REALN (BAQ) + SMART_OVERLAPS, read filter
//                                      UNMAP | SECONDARY | QCFAIL | DUP
// It fills the same PileupViewer (sites in two pools, hostio.h) the text-pileup reader fills, so the
// sanity check, BuildResolvedMarkers and the flattening into pinned SoA arrays are shared.
//
// This is the built-in reader, the one every build of this repository ships: the host stage of
// bam_io.cpp (BGZF, header, .bai, records; plain C++ and zlib), the upload batches of bam_batches.cpp, the per-marker pileup
// of the decoded records on the device (bam_pileup_kernels.hip), the pools back into the PileupViewer.  It applies BAQ and
// the mapQ cap only under bam_adjust = 1 (--ApplyBAQ: fasta_io.cpp, baq_host.cpp, baq_stage.cpp, baq_kernels.hip;
// DESIGN.md section 22) and takes the panel's REF allele as the reference base; it is pinned to tests/bam_ref.py's
// restatement and to the reference's golden files (tests/test_bam_gpu.py).  A reader through htslib, unvalidated, is in
// bam_htslib.cpp and replaces this file only under `cmake -DVB2_WITH_HTSLIB=ON`.
//
// Two behaviours of the reference that look like slips are kept on purpose, because the golden
// outputs were produced with them (SimplePileupViewer.cpp:448-476, 502-511):
//   * a read that has a DELETION at the site contributes no base (pileup_seq, :32) but its quality
//     still goes to qualInfo (:462-470), so from that read on the site's bases and qualities are
//     paired off by one -- ComputeMixLLKs walks baseInfo's length (ContaminationEstimator.h:285-298).
//     Here: the qualities of deleted reads are kept in the list and the first bases.size() of them
//     are what add_site pairs with the bases;
//   * every position the pileup engine reports inside a region is indexed (posIndex, :427-438), even
//     if every read failed min-BQ and the site ends up empty; a marker no read covers is never
//     reported, hence never indexed (siteOfSlot stays -1: BuildResolvedMarkers' "absent").
#include "hostio.h"

#include "context.h"   // set_error

#include "bam_batches.h"
#include "bam_io.h"
#include "bam_pileup_kernels.h"
#include "baq_host.h"
#include "baq_stage.h"
#include "bgzf_inflate_kernels.h"
#include "device_util.h"
#include "mplp_conf.h"
#include "tunables.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace vb2 {
namespace {

using MarkersBySeq = std::vector<std::vector<std::pair<int32_t, int32_t>>>;      // per sequence of the panel: (position, slot) ascending

uint8_t nt16(char c)                   // htslib's seq_nt16_table for the letters a .bed's REF column can hold
{
    static const char kCodes[] = "=ACMGRSVTWYHKDBN";
    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    for (int i = 0; i < 16; ++i)
        if (kCodes[i] == c) return (uint8_t)i;
    return 15;
}

// groups x panel slots must fit the 32-bit virtual slot of the second sort's key, with the all-ones key behind them
bool group_slots_fit(size_t num_group, size_t num_slot) { return (uint64_t)num_group * (uint64_t)num_slot <= 0x7ffffffeull; }

// what a site pass leaves on the host: per slot its depth, its offset into the pools and whether the pileup reported it
struct SiteArrays {
    std::vector<uint32_t> depth, off;
    std::vector<uint8_t> rep;
    std::string bases, quals;
};

// The sites of slots [slot0, slot0 + num_slot) of `a` into v, in .bed row order, a position listed twice once; returns
// the reported sites without a base.
int64_t fill_viewer(const Panel& panel, const SiteArrays& a, size_t slot0, PileupViewer* v)
{
    const int32_t num_slot = (int32_t)panel.num_slot();
    int64_t empty_sites = 0;
    for (size_t row = 0; row < panel.PosVec.size(); ++row) {
        const int32_t slot = panel.rowSlot[row];
        if (slot < 0 || slot >= num_slot || !a.rep[slot0 + (size_t)slot] || v->siteOfSlot[(size_t)slot] >= 0) continue;
        const uint32_t n = a.depth[slot0 + (size_t)slot];
        if (n > 0) {
            v->effectiveNumSite++;
            v->numBases += (int)n;
        } else {
            ++empty_sites;
        }
        v->add_site(slot, a.bases.data() + a.off[slot0 + (size_t)slot], a.quals.data() + a.off[slot0 + (size_t)slot], n);
    }
    v->avgDepth = v->effectiveNumSite ? (double)v->numBases / v->effectiveNumSite : 0.0;
    return empty_sites;
}

// one site pass's arrays on the device: per slot (and one behind) range, depth, offset, reported; per entry the quality the
// overlap rule left; the two pools
struct DeviceSites {
    DeviceBuffer qual, range, depth, off, rep, bases, quals;
};

// Stages 2 and 3 of a load: the scan's records up in batches, entries, sort, sites, pools back, the viewer filled.
// With groups (its flat[g]->viewer initialised) also every read group's sites, behind the whole
// sample's and from the same sorted entries: the whole sample's launches and bytes are what they are without it.
// The members are declared in the order the load allocates them, the stream first: it outlives every buffer.  The
// staging buffers of the batches are members too, so that they live as long as they always did.
class DevicePileup {
public:
    struct Out {
        PileupViewer* v;
        vb2_bam_stats* stats;
        vb2_flat_groups* groups;       // may be null
        vb2_baq_stats* baq_stats;      // may be null; written under --ApplyBAQ
    };
    DevicePileup(const Panel& panel, const MplpConf& conf, int32_t num_group)
        : panel_(panel), conf_(conf), num_slot_((int32_t)panel.num_slot()), num_group_(num_group),
          max_depth_(conf.max_depth < 0 ? 0 : conf.max_depth)
    {
    }
    // spans: null without --ApplyBAQ; caller_stream: null = a stream of the load's own
    int run(const bamio::Scan& scan, const MarkersBySeq& by_seq, int device, hipStream_t caller_stream, const baq::Spans* spans,
            const Out& out);

private:
    enum SiteKind { kSample, kGroups };
    int upload_markers(const bamio::Scan& scan, const MarkersBySeq& by_seq);
    int cover_batches(const bamio::Scan& scan, const baq::Spans* spans, vb2_baq_stats* baq_stats);
    int grow_entries(size_t add);
    int sort_by_slot();
    int group_keys_and_sort();
    int alloc_sites(DeviceSites* d, size_t num_site_slot);
    int launch_sites_of(SiteKind kind, bool fill, DeviceSites& d, int32_t num_site_slot);
    int site_pass(SiteKind kind, int32_t num_site_slot, unsigned long long max_bases, const char* too_many, SiteArrays* host,
                  double* t_device_done);
    size_t ne1() const { return std::max<size_t>((size_t)num_entries_, 1); }

    const Panel& panel_;
    const MplpConf& conf_;
    const int32_t num_slot_, num_group_, max_depth_;
    OwnedStream own_stream_;
    hipStream_t s_ = nullptr;
    DeviceBuffer d_tid_lo_, d_pos_, d_slot_, d_refnib_, d_ctr_;
    PileMarkers markers_{};
    PileFilter filter_{};
    PinnedBuffer h_data_, h_desc_, h_total_, h_grp_;
    DeviceBuffer d_grp_, d_desc_, d_count_, d_offset_, d_total_;
    DeviceBufferList d_batches_;       // the batches' bytes stay: the overlap rule compares read names in them
    DeviceBuffer d_entries_, d_keys_;
    size_t cap_entries_ = 0;
    int64_t num_entries_ = 0, num_batch_ = 0;
    DeviceBuffer d_keys2_, d_idx_, d_idx2_, d_temp_, d_sorted_;
    size_t temp_bytes_ = 0;
    DeviceSites sample_, grouped_;
    PileEntry* d_sorted2_ = nullptr;   // the entries in the groups' order: in d_entries_'s array
};

// marker tables: per tid a run of (position, slot), ascending; the REF alleles' codes; the counters
int DevicePileup::upload_markers(const bamio::Scan& scan, const MarkersBySeq& by_seq)
{
    const int32_t n_ref = (int32_t)scan.ref_name.size();
    std::vector<int32_t> h_tid_lo((size_t)n_ref + 1, 0), h_pos, h_slot;
    std::vector<int32_t> seq_of_tid((size_t)n_ref, -1);
    for (size_t c = 0; c < scan.tid_of_seq.size(); ++c)
        if (scan.tid_of_seq[c] >= 0) seq_of_tid[(size_t)scan.tid_of_seq[c]] = (int32_t)c;
    for (int32_t t = 0; t < n_ref; ++t) {
        h_tid_lo[(size_t)t] = (int32_t)h_pos.size();
        if (seq_of_tid[(size_t)t] < 0) continue;
        for (const auto& ps : by_seq[(size_t)seq_of_tid[(size_t)t]]) {
            h_pos.push_back(ps.first);
            h_slot.push_back(ps.second);
        }
    }
    h_tid_lo[(size_t)n_ref] = (int32_t)h_pos.size();
    std::vector<uint8_t> h_refnib((size_t)num_slot_);
    for (int32_t k = 0; k < num_slot_; ++k) h_refnib[(size_t)k] = nt16(panel_.slotRef[(size_t)k]);
    VB2_HIP(hipMalloc(&d_tid_lo_.p, h_tid_lo.size() * 4));
    VB2_HIP(hipMalloc(&d_pos_.p, std::max<size_t>(h_pos.size(), 1) * 4));
    VB2_HIP(hipMalloc(&d_slot_.p, std::max<size_t>(h_slot.size(), 1) * 4));
    VB2_HIP(hipMalloc(&d_refnib_.p, std::max<size_t>(h_refnib.size(), 1)));
    VB2_HIP(hipMalloc(&d_ctr_.p, sizeof(PileCounters)));
    VB2_HIP(hipMemcpyAsync(d_tid_lo_.p, h_tid_lo.data(), h_tid_lo.size() * 4, hipMemcpyHostToDevice, s_));
    if (!h_pos.empty()) {
        VB2_HIP(hipMemcpyAsync(d_pos_.p, h_pos.data(), h_pos.size() * 4, hipMemcpyHostToDevice, s_));
        VB2_HIP(hipMemcpyAsync(d_slot_.p, h_slot.data(), h_slot.size() * 4, hipMemcpyHostToDevice, s_));
    }
    if (num_slot_ > 0) VB2_HIP(hipMemcpyAsync(d_refnib_.p, h_refnib.data(), h_refnib.size(), hipMemcpyHostToDevice, s_));
    VB2_HIP(hipMemsetAsync(d_ctr_.p, 0, sizeof(PileCounters), s_));
    VB2_HIP(hipStreamSynchronize(s_));            // (the host vectors above may go)
    markers_ = PileMarkers{d_tid_lo_.as<int32_t>(), d_pos_.as<int32_t>(), d_slot_.as<int32_t>(), n_ref};
    filter_ = PileFilter{(int32_t)conf_.rflag_filter, conf_.min_mq, (conf_.flag & kMplpNoOrphan) ? 1 : 0};
    return VB2_OK;
}

// room for `add` more entries and keys behind the num_entries_ there are
int DevicePileup::grow_entries(size_t add)
{
    if ((size_t)num_entries_ + add <= cap_entries_) return VB2_OK;
    const size_t want = std::max<size_t>({(size_t)num_entries_ + add, cap_entries_ * 2, (size_t)1 << 16});
    DeviceBuffer ne, nk;
    VB2_HIP(hipMalloc(&ne.p, want * sizeof(PileEntry)));
    VB2_HIP(hipMalloc(&nk.p, want * sizeof(uint64_t)));
    if (num_entries_ > 0) {
        VB2_HIP(hipMemcpyAsync(ne.p, d_entries_.p, (size_t)num_entries_ * sizeof(PileEntry), hipMemcpyDeviceToDevice, s_));
        VB2_HIP(hipMemcpyAsync(nk.p, d_keys_.p, (size_t)num_entries_ * sizeof(uint64_t), hipMemcpyDeviceToDevice, s_));
        VB2_HIP(hipStreamSynchronize(s_));
    }
    std::swap(ne.p, d_entries_.p);
    std::swap(nk.p, d_keys_.p);
    cap_entries_ = want;
    return VB2_OK;
}

// The batches: the kept records' names, CIGARs, bases and qualities, back to back, and their descriptors; per batch the
// upload, under --ApplyBAQ its stage (without it nothing here differs), the cover pass's count, scan
// and fill into the entries.
int DevicePileup::cover_batches(const bamio::Scan& scan, const baq::Spans* spans, vb2_baq_stats* baq_stats)
{
    BatchPlan plan;
    std::string err;
    if (int rc = plan_batches(scan, vb2::tunables().bam_batch_kb, "--BamFile", &plan, &err)) {
        set_error(err);
        return rc;
    }
    VB2_HIP(hipHostMalloc(&h_data_.p, plan.batch_bytes, hipHostMallocDefault));
    VB2_HIP(hipHostMalloc(&h_desc_.p, plan.batch_rec * sizeof(bamio::RecordDesc), hipHostMallocDefault));
    VB2_HIP(hipHostMalloc(&h_total_.p, sizeof(unsigned long long), hipHostMallocDefault));
    if (num_group_ > 0) {
        VB2_HIP(hipHostMalloc(&h_grp_.p, plan.batch_rec * sizeof(uint16_t), hipHostMallocDefault));
        VB2_HIP(hipMalloc(&d_grp_.p, plan.batch_rec * sizeof(uint16_t)));
    }
    VB2_HIP(hipMalloc(&d_desc_.p, plan.batch_rec * sizeof(bamio::RecordDesc)));
    VB2_HIP(hipMalloc(&d_count_.p, plan.batch_rec * 4));
    VB2_HIP(hipMalloc(&d_offset_.p, plan.batch_rec * 4));
    VB2_HIP(hipMalloc(&d_total_.p, sizeof(unsigned long long)));
    const baq::Options baq_opt = baq::options_of(conf_.flag, conf_.capQ_thres);
    std::unique_ptr<BaqStage> baq_stage;
    if (spans) {
        baq_stage.reset(new BaqStage(baq_opt, s_));
        if (int rc = baq_stage->init(*spans, plan.batch_rec, plan.batch_bytes)) return rc;
    }
    RecordBatch b;
    b.bytes = h_data_.as<uint8_t>();
    b.desc = h_desc_.as<bamio::RecordDesc>();
    b.group = h_grp_.as<uint16_t>();
    const bamio::RecordDesc* const d_desc = d_desc_.as<bamio::RecordDesc>();
    for (BatchCursor cur(scan, plan, spans, spans ? &baq_opt : nullptr); !cur.done();) {
        if (int rc = cur.next(&b, "--BamFile", &err)) {
            set_error(err);
            return rc;
        }
        void* d_bytes = nullptr;
        VB2_HIP(hipMalloc(&d_bytes, std::max<size_t>(b.nb, 1)));
        d_batches_.v.push_back(d_bytes);
        const uint8_t* const d_data = static_cast<const uint8_t*>(d_bytes);
        VB2_HIP(hipMemcpyAsync(d_bytes, b.bytes, b.nb, hipMemcpyHostToDevice, s_));
        VB2_HIP(hipMemcpyAsync(d_desc_.p, b.desc, b.nr * sizeof(bamio::RecordDesc), hipMemcpyHostToDevice, s_));
        if (b.group) VB2_HIP(hipMemcpyAsync(d_grp_.p, b.group, b.nr * sizeof(uint16_t), hipMemcpyHostToDevice, s_));
        const uint8_t* adj_qual = nullptr;
        const int16_t* adj_mapq = nullptr;
        if (baq_stage) {
            if (int rc = baq_stage->run(b, d_desc, d_data, nullptr)) return rc;
            adj_qual = baq_stage->adjq();
            adj_mapq = baq_stage->adj_mapq();
        }
        VB2_HIP(launch_cover_count(d_desc, (int64_t)b.nr, d_data, b.nb, filter_, markers_, d_count_.as<uint32_t>(), s_, adj_qual, adj_mapq));
        VB2_HIP(launch_scan_u32(d_count_.as<uint32_t>(), d_offset_.as<uint32_t>(), (int64_t)b.nr, d_total_.as<unsigned long long>(), s_));
        VB2_HIP(hipMemcpyAsync(h_total_.p, d_total_.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s_));
        VB2_HIP(hipStreamSynchronize(s_));       // the staging buffers are free again; the fill below runs under the next copy-in
        const unsigned long long add = *h_total_.as<unsigned long long>();
        if ((unsigned long long)num_entries_ + add >= 0x7fffffffull) {
            set_error("--BamFile: more than 2^31 (record, marker) pairs over the panel");
            return VB2_ERR_INVALID;
        }
        if (int rc = grow_entries((size_t)add)) return rc;
        if (add > 0)
            VB2_HIP(launch_cover_fill(d_desc, (int64_t)b.nr, d_data, b.nb, filter_, markers_, d_offset_.as<uint32_t>(),
                                      d_entries_.as<PileEntry>() + num_entries_, d_keys_.as<uint64_t>() + num_entries_, s_,
                                      d_grp_.as<uint16_t>(), adj_qual, adj_mapq));
        // (d_desc and d_offset are written again only by the next batch's copies, which the stream orders behind this fill)
        num_entries_ += (int64_t)add;
        ++num_batch_;
    }
    VB2_HIP(hipStreamSynchronize(s_));
    if (baq_stage && baq_stats) *baq_stats = baq_stage->stats;
    return VB2_OK;      // (the BAQ stage goes here: before the sort's buffers come)
}

int DevicePileup::alloc_sites(DeviceSites* d, size_t num_site_slot)
{
    VB2_HIP(hipMalloc(&d->range.p, (num_site_slot + 1) * 4));
    VB2_HIP(hipMalloc(&d->depth.p, (num_site_slot + 1) * 4));
    VB2_HIP(hipMalloc(&d->off.p, (num_site_slot + 1) * 4));
    VB2_HIP(hipMalloc(&d->rep.p, num_site_slot + 1));
    VB2_HIP(hipMalloc(&d->qual.p, ne1()));
    return VB2_OK;
}

// the entries by slot, file order within a slot: d_sorted_, and their keys in d_keys2_
int DevicePileup::sort_by_slot()
{
    if (int rc = alloc_sites(&sample_, (size_t)num_slot_)) return rc;
    VB2_HIP(hipMalloc(&d_sorted_.p, ne1() * sizeof(PileEntry)));
    VB2_HIP(hipMalloc(&d_keys2_.p, ne1() * sizeof(uint64_t)));
    if (num_entries_ == 0) return VB2_OK;
    uint64_t* const keys = d_keys_.as<uint64_t>();
    uint64_t* const keys2 = d_keys2_.as<uint64_t>();
    VB2_HIP(hipMalloc(&d_idx_.p, ne1() * 4));
    VB2_HIP(hipMalloc(&d_idx2_.p, ne1() * 4));
    VB2_HIP(sort_entries(nullptr, &temp_bytes_, keys, keys2, d_idx_.as<uint32_t>(), d_idx2_.as<uint32_t>(), num_entries_, s_));
    VB2_HIP(hipMalloc(&d_temp_.p, std::max<size_t>(temp_bytes_, 1)));
    VB2_HIP(launch_iota_u32(d_idx_.as<uint32_t>(), num_entries_, s_));
    VB2_HIP(sort_entries(d_temp_.p, &temp_bytes_, keys, keys2, d_idx_.as<uint32_t>(), d_idx2_.as<uint32_t>(), num_entries_, s_));
    VB2_HIP(launch_gather(d_entries_.as<PileEntry>(), d_idx2_.as<uint32_t>(), d_sorted_.as<PileEntry>(), num_entries_, s_));
    return VB2_OK;
}

// every read group's sites: a second key per sorted entry, a second sort; the site kernel then runs over virtual slots.
// The unsorted entries and their keys have been gathered: their arrays take the second keys and the second gather.
int DevicePileup::group_keys_and_sort()
{
    if (int rc = alloc_sites(&grouped_, (size_t)num_group_ * (size_t)num_slot_)) return rc;
    d_sorted2_ = num_entries_ > 0 ? d_entries_.as<PileEntry>() : d_sorted_.as<PileEntry>();
    if (num_entries_ == 0) return VB2_OK;
    VB2_HIP(launch_group_keys(d_sorted_.as<PileEntry>(), sample_.range.as<uint32_t>(), num_entries_, num_slot_, num_group_, max_depth_,
                              d_keys_.as<uint64_t>(), s_));
    VB2_HIP(launch_iota_u32(d_idx_.as<uint32_t>(), num_entries_, s_));
    VB2_HIP(sort_entries(d_temp_.p, &temp_bytes_, d_keys_.as<uint64_t>(), d_keys2_.as<uint64_t>(), d_idx_.as<uint32_t>(),
                         d_idx2_.as<uint32_t>(), num_entries_, s_));
    VB2_HIP(launch_group_gather(d_sorted_.as<PileEntry>(), sample_.qual.as<uint8_t>(), d_idx2_.as<uint32_t>(), d_sorted2_,
                                grouped_.qual.as<uint8_t>(), num_entries_, s_));
    return VB2_OK;
}

// the site kernel of one kind: counting (fill = false: depth and rep) or filling the pools at the scanned offsets
int DevicePileup::launch_sites_of(SiteKind kind, bool fill, DeviceSites& d, int32_t num_site_slot)
{
    uint32_t* const off = fill ? d.off.as<uint32_t>() : nullptr;
    char* const bases = fill ? d.bases.as<char>() : nullptr;
    char* const quals = fill ? d.quals.as<char>() : nullptr;
    if (kind == kSample)
        VB2_HIP(launch_sites(fill, d_sorted_.as<PileEntry>(), d.range.as<uint32_t>(), d.qual.as<uint8_t>(), num_site_slot, max_depth_,
                             conf_.min_baseQ, d_refnib_.as<uint8_t>(), d.depth.as<uint32_t>(), d.rep.as<uint8_t>(), off, bases, quals,
                             d_ctr_.as<PileCounters>(), s_));
    else
        VB2_HIP(launch_group_sites(fill, d_sorted2_, d.range.as<uint32_t>(), d.qual.as<uint8_t>(), num_site_slot, num_slot_,
                                   conf_.min_baseQ, d_refnib_.as<uint8_t>(), d.depth.as<uint32_t>(), d.rep.as<uint8_t>(), off, bases, quals,
                                   s_));
    return VB2_OK;
}

// The sites of the sorted entries (the whole sample's slots, with the overlap rule first; or the groups' virtual slots):
// ranges, count, scan, the total to the host, the two pools, fill, everything back.  More than max_bases bases end the
// load with `too_many`.  *t_device_done: the clock between the last launch's end and the copies back.
int DevicePileup::site_pass(SiteKind kind, int32_t num_site_slot, unsigned long long max_bases, const char* too_many, SiteArrays* host,
                            double* t_device_done)
{
    DeviceSites& d = kind == kSample ? sample_ : grouped_;
    VB2_HIP(launch_site_ranges(d_keys2_.as<uint64_t>(), num_entries_, num_site_slot, d.range.as<uint32_t>(), s_));
    if (kind == kSample)
        VB2_HIP(launch_overlap(d_sorted_.as<PileEntry>(), d.range.as<uint32_t>(), num_entries_, max_depth_,
                               (conf_.flag & kMplpSmartOverlaps) ? 1 : 0, d.qual.as<uint8_t>(), d_ctr_.as<PileCounters>(), s_));
    if (int rc = launch_sites_of(kind, false, d, num_site_slot)) return rc;
    VB2_HIP(launch_scan_u32(d.depth.as<uint32_t>(), d.off.as<uint32_t>(), num_site_slot, d_total_.as<unsigned long long>(), s_));
    VB2_HIP(hipMemcpyAsync(h_total_.p, d_total_.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s_));
    VB2_HIP(hipStreamSynchronize(s_));
    const unsigned long long total = *h_total_.as<unsigned long long>();
    if (total > max_bases) {
        set_error(too_many);
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipMalloc(&d.bases.p, std::max<size_t>((size_t)total, 1)));
    VB2_HIP(hipMalloc(&d.quals.p, std::max<size_t>((size_t)total, 1)));
    if (int rc = launch_sites_of(kind, true, d, num_site_slot)) return rc;
    VB2_HIP(hipStreamSynchronize(s_));
    *t_device_done = now_s();

    const size_t n = (size_t)num_site_slot;
    host->depth.assign(n, 0u);
    host->off.assign(n, 0u);
    host->rep.assign(n, 0);
    host->bases.assign((size_t)total, '\0');
    host->quals.assign((size_t)total, '\0');
    if (n > 0) {
        VB2_HIP(hipMemcpy(host->depth.data(), d.depth.p, n * 4, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(host->off.data(), d.off.p, n * 4, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(host->rep.data(), d.rep.p, n, hipMemcpyDeviceToHost));
    }
    if (total > 0) {
        VB2_HIP(hipMemcpy(&host->bases[0], d.bases.p, (size_t)total, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(&host->quals[0], d.quals.p, (size_t)total, hipMemcpyDeviceToHost));
    }
    return VB2_OK;
}

int DevicePileup::run(const bamio::Scan& scan, const MarkersBySeq& by_seq, int device, hipStream_t caller_stream, const baq::Spans* spans,
                      const Out& out)
{
    const double t0 = now_s();
    if (!group_slots_fit((size_t)num_group_, (size_t)num_slot_)) {      // (read_bam_groups has said so already)
        set_error("--PerReadGroup: read groups x panel positions exceed 2^31 - 2");
        return VB2_ERR_INVALID;
    }
    if (device >= 0) VB2_HIP(hipSetDevice(device));
    if (!caller_stream) VB2_HIP(hipStreamCreateWithFlags(&own_stream_.s, hipStreamNonBlocking));
    s_ = caller_stream ? caller_stream : own_stream_.s;
    if (int rc = upload_markers(scan, by_seq)) return rc;
    if (int rc = cover_batches(scan, spans, out.baq_stats)) return rc;
    if (int rc = sort_by_slot()) return rc;
    SiteArrays sites;
    double t1 = 0;
    if (int rc = site_pass(kSample, num_slot_, 0x7fffffffull, "pileup too large: more than 2 GiB of bases at the panel's sites", &sites, &t1))
        return rc;
    const unsigned long long total_bases = sites.bases.size();
    PileCounters ctr{0, 0};
    VB2_HIP(hipMemcpy(&ctr, d_ctr_.p, sizeof(ctr), hipMemcpyDeviceToHost));
    const int64_t empty_sites = fill_viewer(panel_, sites, 0, out.v);
    if (out.stats) {
        out.stats->entries = num_entries_;
        out.stats->batches = num_batch_;
        out.stats->sites = out.v->num_site();
        out.stats->empty_sites = empty_sites;
        out.stats->pairs_resolved = (int64_t)ctr.pairs_resolved;
        out.stats->capped_sites = (int64_t)ctr.capped_sites;
        out.stats->seconds_device = t1 - t0;
        out.stats->seconds_copyback = now_s() - t1;
    }
    if (num_group_ == 0 || num_slot_ == 0) return VB2_OK;

    const double g0 = now_s();
    double g1 = 0;
    if (int rc = group_keys_and_sort()) return rc;
    // (the groups partition a subset of the whole sample's bases)
    if (int rc = site_pass(kGroups, num_group_ * num_slot_, total_bases,
                           "--PerReadGroup: internal error: the groups hold more bases than the whole sample", &sites, &g1))
        return rc;
    for (int32_t g = 0; g < num_group_; ++g)
        fill_viewer(panel_, sites, (size_t)g * (size_t)num_slot_, &out.groups->flat[(size_t)g]->viewer);
    out.groups->seconds_device = g1 - g0;
    out.groups->seconds_copyback = now_s() - g1;
    return VB2_OK;
}

// the panel's markers per sequence name, (position, slot) ascending
void markers_by_sequence(const Panel& panel, std::vector<bamio::SeqMarkers>* seqs, MarkersBySeq* by_seq)
{
    by_seq->assign(panel.chrNames.size(), {});
    for (size_t k = 0; k < panel.num_slot(); ++k) (*by_seq)[(size_t)panel.slotChr[k]].emplace_back(panel.slotPos[k], (int32_t)k);
    seqs->resize(panel.chrNames.size());
    for (size_t c = 0; c < by_seq->size(); ++c) {
        std::sort((*by_seq)[c].begin(), (*by_seq)[c].end());
        (*seqs)[c].name = panel.chrNames[c];
        for (const auto& ps : (*by_seq)[c]) (*seqs)[c].pos.push_back(ps.first);
    }
}

int reader_threads()
{
    const int t = vb2::tunables().bam_threads;
    return std::max(1, std::min(t > 0 ? t : usable_cpu_count(), 16));
}

void host_stats(const bamio::Scan& scan, vb2_bam_stats* st)
{
    std::memset(st, 0, sizeof(*st));
    st->blocks = scan.stats.blocks;
    st->bytes_inflated = scan.stats.bytes_inflated;
    st->records_seen = scan.stats.records_seen;
    st->records_kept = scan.stats.records_kept;
    st->long_cigar_skipped = scan.stats.long_cigar_skipped;
    st->chunks = scan.stats.chunks;
    st->seconds_index = scan.stats.seconds_index;
    st->seconds_inflate = scan.stats.seconds_inflate;
}

// what read_bam and read_bam_groups ask of the one reader below
struct BamRequest {
    const std::string& bam_path;
    const std::string& ref_path;              // read under --ApplyBAQ alone
    const Panel& panel;
    const std::shared_ptr<Panel>* shared;     // of the groups' vb2_flats; null without groups
    const vb2_mpileup_opts* mp;
    int device;
    const BamReadHow* how;                    // may be null
};

// --PerReadGroup: the header's groups into groups->info, a vb2_flat with an initialised viewer per group
int prepare_groups(const bamio::Scan& scan, const Panel& panel, const std::shared_ptr<Panel>& shared, vb2_flat_groups* groups)
{
    if (!group_slots_fit(scan.groups.size(), panel.num_slot())) {      // before anything is sized by the product
        set_error("--PerReadGroup: " + std::to_string(scan.groups.size()) + " read groups x " + std::to_string(panel.num_slot()) +
                  " panel positions exceed 2^31 - 2, the range of the per-group site index");
        return VB2_ERR_INVALID;
    }
    groups->info.resize(scan.groups.size());
    for (size_t g = 0; g < scan.groups.size(); ++g) {
        vb2_flat_groups::Info& gi = groups->info[g];
        gi.id = scan.groups[g].id;
        gi.sm = scan.groups[g].sm;
        gi.lb = scan.groups[g].lb;
        gi.pu = scan.groups[g].pu;
    }
    for (const bamio::Chunk& ch : scan.chunks)
        for (const uint16_t g : ch.group)
            if (g != bamio::kNoGroup) ++groups->info[g].records;
    groups->unassigned = scan.stats.records_unassigned;
    groups->flat.clear();
    for (size_t g = 0; g < scan.groups.size(); ++g) {
        groups->flat.emplace_back(new vb2_flat(shared));
        PileupViewer& gv = groups->flat.back()->viewer;
        gv.SEQ_SM = scan.groups[g].sm.empty() ? scan.sample : scan.groups[g].sm;
        gv.init(panel);
        gv.numBases = 0;
        gv.effectiveNumSite = 0;
    }
    if (scan.stats.records_unassigned > 0)
        std::fprintf(stderr, "NOTICE - --PerReadGroup: %lld of %lld records over the panel's markers belong to no read group of the "
                             "header (no RG:Z field, or an ID it lacks); they count in the whole sample only\n",
                     (long long)scan.stats.records_unassigned, (long long)scan.stats.records_kept);
    return VB2_OK;
}

// Stage 1 of a load: the file and its index, before any device is touched for an input that cannot be read.  Under tunable
// bam_inflate the planned blocks are inflated on the device; nothing of that exists without the
// tunable, and the inflater's staging buffers are gone when this returns: before the pileup's come.
int scan_for_load(const BamRequest& rq, const std::vector<bamio::SeqMarkers>& seqs, bool want_groups, bamio::Scan* scan)
{
    hipStream_t const stream = rq.how ? static_cast<hipStream_t>(rq.how->stream) : nullptr;
    const int threads = rq.how && rq.how->threads > 0 ? std::min(rq.how->threads, 16) : reader_threads();
    std::unique_ptr<DeviceInflater> inflater;
    if (vb2::tunables().bam_inflate != 0) {
        if (usable_device_count() < 1) {
            set_error("--BamFile: bam_inflate = 1 asks for the device inflate and no gfx950 device is visible");
            return VB2_ERR_NO_DEVICE;
        }
        inflater.reset(new DeviceInflater(rq.device, stream, (size_t)std::max(vb2::tunables().bam_batch_kb, 1) << 10));
    }
    std::string err;
    if (int rc = bamio::scan(rq.bam_path, seqs, threads, scan, &err, want_groups, inflater.get())) {
        set_error(err);
        return rc;                     // bamio's codes are the ABI's
    }
    return VB2_OK;
}

// read_bam, and read_bam_groups with groups != nullptr
int read_bam_impl(const BamRequest& rq, PileupViewer* v, vb2_bam_stats* stats, vb2_flat_groups* groups)
{
    MplpConf conf;
    conf.apply(rq.mp);
    const int bam_adjust = rq.how ? rq.how->bam_adjust : 0;
    if (bam_adjust != 0 && bam_adjust != 1) {
        set_error("--BamFile: bam_adjust is " + std::to_string(bam_adjust) + "; it is 0 (records as they are) or 1 (--ApplyBAQ)");
        return VB2_ERR_INVALID;
    }
    std::vector<bamio::SeqMarkers> seqs;
    MarkersBySeq by_seq;
    markers_by_sequence(rq.panel, &seqs, &by_seq);
    bamio::Scan scan;
    if (int rc = scan_for_load(rq, seqs, groups != nullptr, &scan)) return rc;
    if (groups)
        if (int rc = prepare_groups(scan, rq.panel, *rq.shared, groups)) return rc;
    vb2_bam_stats local;
    if (!stats) stats = &local;
    host_stats(scan, stats);
    v->SEQ_SM = scan.sample;
    v->init(rq.panel);
    v->numBases = 0;
    v->effectiveNumSite = 0;
    if (usable_device_count() < 1) {
        set_error("--BamFile: no gfx950 device is visible; the pileup of the decoded records runs on the GPU only "
                  "(there is no CPU fallback)");
        return VB2_ERR_NO_DEVICE;
    }
    // --ApplyBAQ: the spans of the FASTA the records can touch (not opened when the options ask for neither BAQ nor the cap)
    baq::Spans spans;
    if (bam_adjust) {
        std::string err;
        if (int rc = baq::load_spans(scan, rq.ref_path, baq::options_of(conf.flag, conf.capQ_thres), &spans, &err)) {
            set_error(err);
            return rc;
        }
    }
    DevicePileup pileup(rq.panel, conf, groups ? (int32_t)groups->flat.size() : 0);
    return pileup.run(scan, by_seq, rq.device, rq.how ? static_cast<hipStream_t>(rq.how->stream) : nullptr, bam_adjust ? &spans : nullptr,
                      DevicePileup::Out{v, stats, groups, bam_adjust ? rq.how->baq_stats : nullptr});
}

// vb2_baq_records(where = 0): baq_core.h's sequential host driver over every record
void baq_records_on_host(const bamio::Scan& scan, const baq::Spans& spans, const baq::Options& opt, BaqRecords* out)
{
    vb2_baq_stats& st = out->stats;
    st.seconds_fasta = spans.seconds;
    st.fasta_bytes = spans.bytes_read;
    std::vector<double> scratch;
    std::vector<uint8_t> q;
    for (size_t ci = 0; ci < scan.chunks.size(); ++ci) {
        const bamio::Chunk& ch = scan.chunks[ci];
        for (size_t ri = 0; ri < ch.recs.size(); ++ri) {
            const bamio::RecordDesc& d = ch.recs[ri];
            const uint8_t* bq = nullptr;
            baq::Task t = baq::make_task(scan, ci, ri, spans, opt, &bq);
            if (t.kind == 1) t.bq_off = 0;
            q.assign((size_t)d.l_seq, 0);
            int32_t c4[4];
            st.undefined_rows += baq::run_record(d, ch.bytes.data() + d.data, t, spans.codes.data(), bq, opt, q.data(), c4, &scratch);
            out->append(q.data(), d.l_seq, baq::finish_record(d.mapq, t, c4, opt, &st), c4);
        }
    }
}

// vb2_baq_records(where = 1): the device stage over the load's batches
int baq_records_on_device(const bamio::Scan& scan, const baq::Spans& spans, const baq::Options& opt, int device, BaqRecords* out)
{
    if (device >= 0) VB2_HIP(hipSetDevice(device));
    OwnedStream st;
    VB2_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    hipStream_t s = st.s;
    BatchPlan plan;
    std::string err;
    if (int rc = plan_batches(scan, vb2::tunables().bam_batch_kb, "vb2_baq_records", &plan, &err)) {
        set_error(err);
        return rc;
    }
    std::vector<uint8_t> hd(plan.batch_bytes);
    std::vector<bamio::RecordDesc> hr(plan.batch_rec);
    DeviceBuffer d_data, d_desc;
    VB2_HIP(hipMalloc(&d_data.p, plan.batch_bytes));
    VB2_HIP(hipMalloc(&d_desc.p, plan.batch_rec * sizeof(bamio::RecordDesc)));
    BaqStage stage(opt, s);
    if (int rc = stage.init(spans, plan.batch_rec, plan.batch_bytes)) return rc;
    RecordBatch b;
    b.bytes = hd.data();
    b.desc = hr.data();
    for (BatchCursor cur(scan, plan, &spans, &opt); !cur.done();) {
        if (int rc = cur.next(&b, "vb2_baq_records", &err)) {
            set_error(err);
            return rc;
        }
        VB2_HIP(hipMemcpyAsync(d_data.p, b.bytes, b.nb, hipMemcpyHostToDevice, s));
        VB2_HIP(hipMemcpyAsync(d_desc.p, b.desc, b.nr * sizeof(bamio::RecordDesc), hipMemcpyHostToDevice, s));
        VB2_HIP(hipStreamSynchronize(s));
        if (int rc = stage.run(b, d_desc.as<bamio::RecordDesc>(), d_data.as<uint8_t>(), out)) return rc;
    }
    out->stats = stage.stats;
    return VB2_OK;
}

}  // namespace

int read_bam(const std::string& bam_path, const std::string& ref_path, const Panel& panel, PileupViewer* v, const vb2_mpileup_opts* mp,
             int device, vb2_bam_stats* stats, const BamReadHow* how)
{
    return read_bam_impl(BamRequest{bam_path, ref_path, panel, nullptr, mp, device, how}, v, stats, nullptr);
}

int read_bam_groups(const std::string& bam_path, const std::shared_ptr<Panel>& panel, PileupViewer* v, const vb2_mpileup_opts* mp,
                    int device, vb2_bam_stats* stats, vb2_flat_groups* groups, const std::string& ref_path, const BamReadHow* how)
{
    if (!panel || !groups) {
        set_error("read_bam_groups: invalid argument");
        return VB2_ERR_INVALID;
    }
    return read_bam_impl(BamRequest{bam_path, ref_path, *panel, &panel, mp, device, how}, v, stats, groups);
}

// vb2_baq_records: the scan, the spans, and per record the host driver (where 0) or the device stage in the load's batches
int baq_records_file(const std::string& bam_path, const std::string& bed_path, const std::string& ref_path, const vb2_mpileup_opts* mp,
                     int where, int device, BaqRecords* out)
{
    if (where != 0 && where != 1) {
        set_error("vb2_baq_records: where is 0 (host driver) or 1 (device stage)");
        return VB2_ERR_INVALID;
    }
    MplpConf conf;
    conf.apply(mp);
    const baq::Options opt = baq::options_of(conf.flag, conf.capQ_thres);
    Panel panel;
    if (int rc = read_bed(bed_path, &panel)) return rc;
    std::vector<bamio::SeqMarkers> seqs;
    MarkersBySeq by_seq;
    markers_by_sequence(panel, &seqs, &by_seq);
    bamio::Scan scan;
    std::string err;
    if (int rc = bamio::scan(bam_path, seqs, reader_threads(), &scan, &err)) {
        set_error(err);
        return rc;
    }
    baq::Spans spans;
    if (int rc = baq::load_spans(scan, ref_path, opt, &spans, &err)) {
        set_error(err);
        return rc;
    }
    *out = BaqRecords{};
    if (where == 0) {
        baq_records_on_host(scan, spans, opt, out);
        return VB2_OK;
    }
    if (usable_device_count() < 1) {
        set_error("vb2_baq_records: where = 1 runs the device stage and no gfx950 device is visible");
        return VB2_ERR_NO_DEVICE;
    }
    return baq_records_on_device(scan, spans, opt, device, out);
}

bool bam_support() { return true; }

// Stage 1 alone (vb2_bam_scan): no device
int bam_scan_file(const std::string& bam_path, const std::string& bed_path, std::vector<uint64_t>* voffsets, vb2_bam_stats* stats,
                  std::string* sample, std::vector<std::string>* group_ids, std::vector<uint16_t>* groups)
{
    Panel panel;
    if (int rc = read_bed(bed_path, &panel)) return rc;
    std::vector<bamio::SeqMarkers> seqs;
    MarkersBySeq by_seq;
    markers_by_sequence(panel, &seqs, &by_seq);
    bamio::Scan scan;
    std::string err;
    const bool want_groups = group_ids && groups;
    if (int rc = bamio::scan(bam_path, seqs, reader_threads(), &scan, &err, want_groups)) {
        set_error(err);
        return rc;
    }
    host_stats(scan, stats);
    *sample = scan.sample;
    voffsets->clear();
    for (const bamio::Chunk& ch : scan.chunks) voffsets->insert(voffsets->end(), ch.voffset.begin(), ch.voffset.end());
    if (want_groups) {
        group_ids->clear();
        groups->clear();
        for (const bamio::ReadGroup& g : scan.groups) group_ids->push_back(g.id);
        for (const bamio::Chunk& ch : scan.chunks) groups->insert(groups->end(), ch.group.begin(), ch.group.end());
    }
    return VB2_OK;
}

}  // namespace vb2
