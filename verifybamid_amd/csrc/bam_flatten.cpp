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
// TWO READERS, one per build.  The default build has the built-in one at the end of this file: the
// host stage of bam_io.cpp (BGZF, header, .bai, records; plain C++ and zlib), the per-marker pileup of the decoded records on
// the device (bam_pileup_kernels.hip), the pools back into the PileupViewer.  It applies BAQ and the mapQ cap only under
// bam_adjust = 1 (--ApplyBAQ: fasta_io.cpp, baq_host.cpp, baq_stage.cpp, baq_kernels.hip) and
// takes the panel's REF allele as the reference base; it is pinned to tests/bam_ref.py's restatement and to the reference's
// golden files (tests/test_bam_gpu.py).
// The htslib reader below NEEDS htslib (>= 1.10: hts_pos_t), which neither this build image nor the GPU box has (probed
// in round 3: no htslib/sam.h, no libhts anywhere on either).  It is compiled only on an explicit opt-in,
// `cmake -DVB2_WITH_HTSLIB=ON` (default OFF since round 3: a machine that happens to have libhts must not silently ship an
// unvalidated reader).  STATUS: written against htslib's public API, NOT compiled and NOT validated anywhere: parity at
// this boundary is UNPINNED -- validate with `--OutputPileup` against the reference's expected/result.Pileup where htslib
// and a BAM exist before relying on it.
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

#ifdef VB2_WITH_HTSLIB
#include <htslib/faidx.h>
#include <htslib/hts.h>
#include <htslib/sam.h>

#include <cctype>
#include <cstring>
#include <string>
#include <vector>

namespace vb2 {
namespace {

// the reference's mode bits of mplp.flag (SimplePileupViewer.h:14-24) -- `--incl-flags` stores its value THERE
// (main.cpp:185-186), not in a required-read-flags mask: kept
constexpr int kMplpNoOrphan = 1 << 3, kMplpRealn = 1 << 4, kMplpIllumina13 = 1 << 7, kMplpRedoBaq = 1 << 6,
              kMplpSmartOverlaps = 1 << 10;

struct MplpConf {                      // main.cpp:81-96
    int min_mq = 2, min_baseQ = 13, capQ_thres = 40, max_depth = 8000;
    int flag = kMplpRealn | kMplpSmartOverlaps;
    uint32_t rflag_filter = BAM_FUNMAP | BAM_FSECONDARY | BAM_FQCFAIL | BAM_FDUP;
    void apply(const vb2_mpileup_opts* mp)      // main.cpp:176-187, 208-211
    {
        if (!mp || !mp->given) return;
        min_baseQ = mp->min_bq;
        min_mq = mp->min_mq;
        capQ_thres = mp->adjust_mq;
        max_depth = mp->max_depth;
        flag = mp->incl_flags;
        if (mp->no_orphans) flag |= kMplpNoOrphan;
        else flag &= ~kMplpNoOrphan;
        rflag_filter = (uint32_t)mp->excl_flags;
    }
};

struct Aux {
    samFile* fp = nullptr;
    sam_hdr_t* hdr = nullptr;
    hts_itr_t* iter = nullptr;
    faidx_t* fai = nullptr;
    char* ref = nullptr;               // sequence of ref_tid (cached: consecutive markers share it)
    int ref_tid = -1;
    hts_pos_t ref_len = 0;
    MplpConf conf;
};

bool fetch_ref(Aux* a, int tid)
{
    if (!a->fai) return false;
    if (tid == a->ref_tid) return a->ref != nullptr;
    free(a->ref);
    a->ref = nullptr;
    a->ref_tid = tid;
    hts_pos_t len = 0;
    a->ref = faidx_fetch_seq64(a->fai, sam_hdr_tid2name(a->hdr, tid), 0, HTS_POS_MAX, &len);
    a->ref_len = a->ref ? len : 0;
    return a->ref != nullptr;
}

// the pileup engine's read source: same order of tests as mplp_func (SimplePileupViewer.cpp:172-237)
int next_read(void* data, bam1_t* b)
{
    Aux* a = static_cast<Aux*>(data);
    int ret;
    for (;;) {
        ret = a->iter ? sam_itr_next(a->fp, a->iter, b) : sam_read1(a->fp, a->hdr, b);
        if (ret < 0) break;
        if (b->core.tid < 0 || (b->core.flag & BAM_FUNMAP)) continue;
        if (a->conf.rflag_filter & b->core.flag) continue;
        if (a->conf.flag & kMplpIllumina13) {                          // SimplePileupViewer.cpp:203-208
            uint8_t* qual = bam_get_qual(b);
            for (int i = 0; i < b->core.l_qseq; ++i) qual[i] = qual[i] > 31 ? qual[i] - 31 : 0;
        }
        const bool has_ref = fetch_ref(a, b->core.tid);
        if (has_ref && a->ref_len <= b->core.pos) continue;            // read outside the reference sequence
        if (has_ref && (a->conf.flag & kMplpRealn))                    // BAQ
            sam_prob_realn(b, a->ref, a->ref_len, (a->conf.flag & kMplpRedoBaq) ? 7 : 3);
        if (has_ref && a->conf.capQ_thres > 10) {
            const int q = sam_cap_mapq(b, a->ref, a->ref_len, a->conf.capQ_thres);
            if (q < 0) continue;
            if (b->core.qual > q) b->core.qual = (uint8_t)q;
        }
        if (b->core.qual < a->conf.min_mq) continue;
        if ((a->conf.flag & kMplpNoOrphan) && (b->core.flag & BAM_FPAIRED) && !(b->core.flag & BAM_FPROPER_PAIR)) continue;
        break;
    }
    return ret;
}

std::string sample_name(sam_hdr_t* hdr)     // @RG SM: (SimplePileupViewer.cpp:296-314; several samples are an error there)
{
    const char* text = sam_hdr_str(hdr);
    std::string sm;
    for (const char* p = text ? std::strstr(text, "@RG") : nullptr; p; p = std::strstr(p + 3, "@RG")) {
        const char* eol = std::strchr(p, '\n');
        const char* t = std::strstr(p, "\tSM:");
        if (!t || (eol && t > eol)) continue;
        t += 4;
        const char* e = t;
        while (*e && *e != '\t' && *e != '\n') ++e;
        const std::string one(t, e);
        if (sm.empty()) sm = one;
        else if (sm != one) return std::string();       // more than one sample
    }
    return sm.empty() ? std::string("DefaultSampleName") : sm;
}

}  // namespace

int read_bam(const std::string& bam_path, const std::string& ref_path, const Panel& panel, PileupViewer* v,
             const vb2_mpileup_opts* mp, int, vb2_bam_stats*, const BamReadHow*)
{
    Aux a;
    a.conf.apply(mp);
    hts_idx_t* idx = nullptr;
    struct Cleanup {                       // every exit path releases what was opened so far
        Aux& a;
        hts_idx_t*& idx;
        ~Cleanup()
        {
            if (a.iter) hts_itr_destroy(a.iter);
            free(a.ref);
            if (a.fai) fai_destroy(a.fai);
            if (idx) hts_idx_destroy(idx);
            if (a.hdr) sam_hdr_destroy(a.hdr);
            if (a.fp) sam_close(a.fp);
        }
    } cleanup{a, idx};
    a.fp = sam_open(bam_path.c_str(), "rb");
    if (!a.fp) { set_error("failed to open " + bam_path); return VB2_ERR_IO; }
    if (hts_set_fai_filename(a.fp, ref_path.c_str()) != 0) { set_error("failed to process " + ref_path); return VB2_ERR_IO; }
    a.hdr = sam_hdr_read(a.fp);
    if (!a.hdr) { set_error("fail to read the header of " + bam_path); return VB2_ERR_IO; }
    idx = sam_index_load(a.fp, bam_path.c_str());
    if (!idx) { set_error("fail to load index for " + bam_path); return VB2_ERR_IO; }
    a.fai = fai_load(ref_path.c_str());
    v->SEQ_SM = sample_name(a.hdr);
    if (v->SEQ_SM.empty()) {
        set_error("This BAM or CRAM file contains more than 1 sample, please demultiplex or separate first!");
        return VB2_ERR_INVALID;
    }
    v->init(panel);
    v->numBases = 0;
    std::string bases, quals;
    // one region per panel marker, in .bed order (the reference jumps region by region too)
    for (size_t row = 0; row < panel.PosVec.size(); ++row) {
        const auto& marker = panel.PosVec[row];
        const std::string& chr = marker.first;
        const int pos1 = marker.second;                                   // 1-based
        const int tid = sam_hdr_name2tid(a.hdr, chr.c_str());
        if (tid < 0) continue;
        const int32_t slot = panel.rowSlot[row];
        if (v->siteOfSlot[slot] >= 0) continue;                           // duplicated marker: skipped (cpp:424-427)
        bases.clear();
        quals.clear();
        bool reported = false;             // the pileup engine produced this position (>= 1 alignment over it)
        a.iter = sam_itr_queryi(idx, tid, pos1 - 1, pos1);
        if (a.iter) {
            bam_plp_t plp = bam_plp_init(next_read, &a);
            bam_plp_set_maxcnt(plp, a.conf.max_depth);
            if (a.conf.flag & kMplpSmartOverlaps) bam_plp_init_overlaps(plp);
            int ptid, ppos, n;
            const bam_pileup1_t* pl;
            while ((pl = bam_plp_auto(plp, &ptid, &ppos, &n)) != nullptr) {
                if (ptid != tid || ppos != pos1 - 1) continue;
                reported = true;
                const bool has_ref = fetch_ref(&a, tid);
                for (int j = 0; j < n; ++j) {
                    const bam_pileup1_t* p = pl + j;
                    const int q = p->qpos < p->b->core.l_qseq ? bam_get_qual(p->b)[p->qpos] : 0;
                    if (q < a.conf.min_baseQ) continue;                   // SimplePileupViewer.cpp:457, 467
                    // the quality of EVERY read that passes min-BQ, deleted ones included (:462-470) ...
                    quals.push_back((char)(q + 33 < 126 ? q + 33 : 126));
                    if (p->is_del) continue;                              // ... but a base only where there is one (:32)
                    int c = p->qpos < p->b->core.l_qseq ? seq_nt16_str[bam_seqi(bam_get_seq(p->b), p->qpos)] : 'N';
                    const bool rev = bam_is_rev(p->b);
                    if (has_ref) {                                        // pileup_seq, SimplePileupViewer.cpp:32-40
                        const int rb = ppos < a.ref_len ? a.ref[ppos] : 'N';
                        if (c == '=' || seq_nt16_table[c] == seq_nt16_table[rb]) c = rev ? ',' : '.';
                        else c = rev ? std::tolower(c) : std::toupper(c);
                    } else {
                        c = c == '=' ? (rev ? ',' : '.') : (rev ? std::tolower(c) : std::toupper(c));
                    }
                    bases.push_back((char)c);
                }
            }
            bam_plp_destroy(plp);
            hts_itr_destroy(a.iter);
            a.iter = nullptr;
        }
        if (!reported) continue;           // never seen by the reference's loop: not indexed (posIndex, :427-438)
        if (!bases.empty()) {
            v->effectiveNumSite++;
            v->numBases += (int)bases.size();
        }
        // bases.size() <= quals.size(): the pairing is by index, like the reference's (header of this file)
        v->add_site(slot, bases.data(), quals.data(), bases.size());
    }
    v->avgDepth = v->effectiveNumSite ? (double)v->numBases / v->effectiveNumSite : 0.0;
    return VB2_OK;
}

int read_bam_groups(const std::string&, const std::shared_ptr<Panel>&, PileupViewer*, const vb2_mpileup_opts*, int, vb2_bam_stats*,
                    vb2_flat_groups*, const std::string&, const BamReadHow*)
{
    set_error("--PerReadGroup: this library reads BAM through htslib (VB2_WITH_HTSLIB); read groups are the built-in reader's");
    return VB2_ERR_INVALID;
}

bool bam_support() { return true; }

int baq_records_file(const std::string&, const std::string&, const std::string&, const vb2_mpileup_opts*, int, int, BaqRecords*)
{
    set_error("vb2_baq_records: this library reads BAM through htslib (VB2_WITH_HTSLIB), which applies BAQ itself");
    return VB2_ERR_INVALID;
}

int bam_scan_file(const std::string&, const std::string&, std::vector<uint64_t>*, vb2_bam_stats*, std::string*,
                  std::vector<std::string>*, std::vector<uint16_t>*)
{
    set_error("vb2_bam_scan: this library reads BAM through htslib (VB2_WITH_HTSLIB); the built-in reader's host stage is not in it");
    return VB2_ERR_INVALID;
}

}  // namespace vb2

#else   // ---- built without htslib: the built-in reader ----

#include "bam_io.h"
#include "bam_pileup_kernels.h"
#include "baq_host.h"
#include "baq_stage.h"
#include "bgzf_inflate_kernels.h"
#include "device_util.h"
#include "tunables.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace vb2 {
namespace {

constexpr int kMplpNoOrphan = 1 << 3, kMplpRealn = 1 << 4, kMplpSmartOverlaps = 1 << 10;

struct MplpConf {                      // main.cpp:81-96
    int min_mq = 2, min_baseQ = 13, capQ_thres = 40, max_depth = 8000;
    int flag = kMplpRealn | kMplpSmartOverlaps;
    uint32_t rflag_filter = 4 | 256 | 512 | 1024;      // UNMAP | SECONDARY | QCFAIL | DUP
    void apply(const vb2_mpileup_opts* mp)      // main.cpp:176-187, 208-211
    {
        if (!mp || !mp->given) return;
        min_baseQ = mp->min_bq;
        min_mq = mp->min_mq;
        capQ_thres = mp->adjust_mq;
        max_depth = mp->max_depth;
        flag = mp->incl_flags;
        if (mp->no_orphans) flag |= kMplpNoOrphan;
        else flag &= ~kMplpNoOrphan;
        rflag_filter = (uint32_t)mp->excl_flags;
    }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

uint8_t nt16(char c)                   // htslib's seq_nt16_table for the letters a .bed's REF column can hold
{
    static const char kCodes[] = "=ACMGRSVTWYHKDBN";
    if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    for (int i = 0; i < 16; ++i)
        if (kCodes[i] == c) return (uint8_t)i;
    return 15;
}

// device, pinned and stream handles that every exit path releases
struct Dev {
    void* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct Pinned {
    void* p = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); }
};
struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
};
struct DevList {
    std::vector<void*> v;
    ~DevList() { for (void* p : v) (void)hipFree(p); }
};

// groups x panel slots must fit the 32-bit virtual slot of the second sort's key, with the all-ones key behind them
bool group_slots_fit(size_t num_group, size_t num_slot) { return (uint64_t)num_group * (uint64_t)num_slot <= 0x7ffffffeull; }

// Stages 2 and 3: the scan's records up in batches, entries, sort, sites, pools back, the viewer filled.
// groups (may be null; its flat[g]->viewer initialised): also every read group's sites, behind the
// whole sample's and from the same sorted entries: the whole sample's launches and bytes are what they are without it.
int device_pileup(const bamio::Scan& scan, const std::vector<std::vector<std::pair<int32_t, int32_t>>>& by_seq, const Panel& panel,
                  const MplpConf& conf, int device, PileupViewer* v, vb2_bam_stats* stats, vb2_flat_groups* groups = nullptr,
                  hipStream_t caller_stream = nullptr, const baq::Spans* spans = nullptr, vb2_baq_stats* baq_stats = nullptr)
{
    const double t0 = now_s();
    const int32_t num_slot = (int32_t)panel.num_slot();
    const int32_t num_group = groups ? (int32_t)groups->flat.size() : 0;
    if (!group_slots_fit((size_t)num_group, (size_t)num_slot)) {      // (read_bam_groups has said so already)
        set_error("--PerReadGroup: read groups x panel positions exceed 2^31 - 2");
        return VB2_ERR_INVALID;
    }
    const int32_t n_ref = (int32_t)scan.ref_name.size();
    if (device >= 0) VB2_HIP(hipSetDevice(device));
    StreamHolder st;
    if (!caller_stream) VB2_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    hipStream_t s = caller_stream ? caller_stream : st.s;

    // marker tables: per tid a run of (position, slot), ascending
    std::vector<int32_t> h_tid_lo((size_t)n_ref + 1, 0), h_pos, h_slot;
    {
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
    }
    std::vector<uint8_t> h_refnib((size_t)num_slot);
    for (int32_t k = 0; k < num_slot; ++k) h_refnib[(size_t)k] = nt16(panel.slotRef[(size_t)k]);
    Dev d_tid_lo, d_pos, d_slot, d_refnib, d_ctr;
    VB2_HIP(hipMalloc(&d_tid_lo.p, h_tid_lo.size() * 4));
    VB2_HIP(hipMalloc(&d_pos.p, std::max<size_t>(h_pos.size(), 1) * 4));
    VB2_HIP(hipMalloc(&d_slot.p, std::max<size_t>(h_slot.size(), 1) * 4));
    VB2_HIP(hipMalloc(&d_refnib.p, std::max<size_t>(h_refnib.size(), 1)));
    VB2_HIP(hipMalloc(&d_ctr.p, sizeof(PileCounters)));
    VB2_HIP(hipMemcpyAsync(d_tid_lo.p, h_tid_lo.data(), h_tid_lo.size() * 4, hipMemcpyHostToDevice, s));
    if (!h_pos.empty()) {
        VB2_HIP(hipMemcpyAsync(d_pos.p, h_pos.data(), h_pos.size() * 4, hipMemcpyHostToDevice, s));
        VB2_HIP(hipMemcpyAsync(d_slot.p, h_slot.data(), h_slot.size() * 4, hipMemcpyHostToDevice, s));
    }
    if (num_slot > 0) VB2_HIP(hipMemcpyAsync(d_refnib.p, h_refnib.data(), h_refnib.size(), hipMemcpyHostToDevice, s));
    VB2_HIP(hipMemsetAsync(d_ctr.p, 0, sizeof(PileCounters), s));
    VB2_HIP(hipStreamSynchronize(s));            // (the host vectors above may go)
    const PileMarkers markers{d_tid_lo.as<int32_t>(), d_pos.as<int32_t>(), d_slot.as<int32_t>(), n_ref};
    const PileFilter filter{(int32_t)conf.rflag_filter, conf.min_mq, (conf.flag & kMplpNoOrphan) ? 1 : 0};
    const int32_t max_depth = conf.max_depth < 0 ? 0 : conf.max_depth;

    // ---- batches: the kept records' names, CIGARs, bases and qualities, back to back, and their descriptors ----
    auto var_bytes = [](const bamio::RecordDesc& d) {
        return (size_t)d.l_read_name + 4 * (size_t)d.n_cigar + ((size_t)d.l_seq + 1) / 2 + (size_t)d.l_seq;
    };
    size_t largest = 0, total_rec = 0;
    for (const bamio::Chunk& ch : scan.chunks) {
        total_rec += ch.recs.size();
        for (const bamio::RecordDesc& d : ch.recs) largest = std::max(largest, var_bytes(d));
    }
    const size_t batch_bytes = std::max<size_t>((size_t)std::max(vb2::tunables().bam_batch_kb, 1) << 10, largest);
    if (batch_bytes > 0xfff00000ull) { set_error("--BamFile: bam_batch_kb asks for batches of 4 GiB or more"); return VB2_ERR_INVALID; }
    // a batch closes when its bytes are full; its records are bounded by its bytes (a record has at least a name)
    // ... or when its descriptors weigh as much as its bytes would
    const size_t batch_rec = std::min<size_t>(std::max<size_t>(total_rec, 1), std::max<size_t>(batch_bytes / sizeof(bamio::RecordDesc), 1));
    Pinned h_data, h_desc, h_total;
    VB2_HIP(hipHostMalloc(&h_data.p, batch_bytes, hipHostMallocDefault));
    VB2_HIP(hipHostMalloc(&h_desc.p, batch_rec * sizeof(bamio::RecordDesc), hipHostMallocDefault));
    VB2_HIP(hipHostMalloc(&h_total.p, sizeof(unsigned long long), hipHostMallocDefault));
    Pinned h_grp;
    Dev d_grp;
    if (num_group > 0) {
        VB2_HIP(hipHostMalloc(&h_grp.p, batch_rec * sizeof(uint16_t), hipHostMallocDefault));
        VB2_HIP(hipMalloc(&d_grp.p, batch_rec * sizeof(uint16_t)));
    }
    uint16_t* const hg = static_cast<uint16_t*>(h_grp.p);
    Dev d_desc, d_count, d_offset, d_total;
    VB2_HIP(hipMalloc(&d_desc.p, batch_rec * sizeof(bamio::RecordDesc)));
    VB2_HIP(hipMalloc(&d_count.p, batch_rec * 4));
    VB2_HIP(hipMalloc(&d_offset.p, batch_rec * 4));
    VB2_HIP(hipMalloc(&d_total.p, sizeof(unsigned long long)));
    DevList d_batches;                            // the batches' bytes stay: the overlap rule compares read names in them
    Dev d_entries, d_keys;
    size_t cap_entries = 0;
    int64_t num_entries = 0, num_batch = 0;
    uint8_t* const hd = static_cast<uint8_t*>(h_data.p);
    bamio::RecordDesc* const hr = static_cast<bamio::RecordDesc*>(h_desc.p);
    // --ApplyBAQ: a stage between a batch's upload and its cover pass; without it nothing below differs
    const baq::Options baq_opt = baq::options_of(conf.flag, conf.capQ_thres);
    std::unique_ptr<BaqStage> baq_stage;
    std::vector<baq::Task> baq_tasks;
    std::vector<uint8_t> baq_extra;
    if (spans) {
        baq_stage.reset(new BaqStage(baq_opt, s));
        if (int rc = baq_stage->init(*spans, batch_rec, batch_bytes)) return rc;
    }

    size_t ci = 0, ri = 0;                        // next record: scan.chunks[ci].recs[ri]
    auto skip_empty = [&] { while (ci < scan.chunks.size() && ri >= scan.chunks[ci].recs.size()) { ++ci; ri = 0; } };
    skip_empty();
    while (ci < scan.chunks.size()) {
        size_t nb = 0, nr = 0;
        baq_tasks.clear();
        baq_extra.clear();
        while (ci < scan.chunks.size() && nr < batch_rec) {
            const bamio::Chunk& ch = scan.chunks[ci];
            const bamio::RecordDesc& d = ch.recs[ri];
            const size_t vb = var_bytes(d);
            if ((size_t)d.data > ch.bytes.size() || vb > ch.bytes.size() - d.data) {      // (bam_io.cpp has checked this)
                set_error("--BamFile: internal error: a record passes its chunk");
                return VB2_ERR_INVALID;
            }
            if (nb + vb > batch_bytes) break;
            std::memcpy(hd + nb, ch.bytes.data() + d.data, vb);
            hr[nr] = d;
            hr[nr].data = (uint32_t)nb;
            if (hg) hg[nr] = ri < ch.group.size() ? ch.group[ri] : bamio::kNoGroup;
            if (baq_stage) {
                const uint8_t* bq = nullptr;
                baq::Task t = baq::make_task(scan, ci, ri, *spans, baq_opt, &bq);
                if (t.kind == 1 && bq) {
                    t.bq_off = (uint32_t)baq_extra.size();
                    baq_extra.insert(baq_extra.end(), bq, bq + d.l_seq);
                }
                baq_tasks.push_back(t);
            }
            nb += vb;
            ++nr;
            ++ri;
            skip_empty();
        }
        void* d_data = nullptr;
        VB2_HIP(hipMalloc(&d_data, std::max<size_t>(nb, 1)));
        d_batches.v.push_back(d_data);
        VB2_HIP(hipMemcpyAsync(d_data, hd, nb, hipMemcpyHostToDevice, s));
        VB2_HIP(hipMemcpyAsync(d_desc.p, hr, nr * sizeof(bamio::RecordDesc), hipMemcpyHostToDevice, s));
        if (hg) VB2_HIP(hipMemcpyAsync(d_grp.p, hg, nr * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        const uint8_t* adj_qual = nullptr;
        const int16_t* adj_mapq = nullptr;
        if (baq_stage) {
            if (int rc = baq_stage->run(baq_tasks, baq_extra, hr, nr, d_desc.as<bamio::RecordDesc>(), static_cast<const uint8_t*>(d_data),
                                        nb, nullptr, nullptr, nullptr, nullptr))
                return rc;
            adj_qual = baq_stage->adjq();
            adj_mapq = baq_stage->adj_mapq();
        }
        VB2_HIP(launch_cover_count(d_desc.as<bamio::RecordDesc>(), (int64_t)nr, static_cast<const uint8_t*>(d_data), nb, filter,
                                   markers, d_count.as<uint32_t>(), s, adj_qual, adj_mapq));
        VB2_HIP(launch_scan_u32(d_count.as<uint32_t>(), d_offset.as<uint32_t>(), (int64_t)nr, d_total.as<unsigned long long>(), s));
        VB2_HIP(hipMemcpyAsync(h_total.p, d_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        VB2_HIP(hipStreamSynchronize(s));        // the staging buffers are free again; the fill below runs under the next copy-in
        const unsigned long long add = *static_cast<unsigned long long*>(h_total.p);
        if ((unsigned long long)num_entries + add >= 0x7fffffffull) {
            set_error("--BamFile: more than 2^31 (record, marker) pairs over the panel");
            return VB2_ERR_INVALID;
        }
        if ((size_t)num_entries + add > cap_entries) {
            const size_t want = std::max<size_t>({(size_t)num_entries + (size_t)add, cap_entries * 2, (size_t)1 << 16});
            Dev ne, nk;
            VB2_HIP(hipMalloc(&ne.p, want * sizeof(PileEntry)));
            VB2_HIP(hipMalloc(&nk.p, want * sizeof(uint64_t)));
            if (num_entries > 0) {
                VB2_HIP(hipMemcpyAsync(ne.p, d_entries.p, (size_t)num_entries * sizeof(PileEntry), hipMemcpyDeviceToDevice, s));
                VB2_HIP(hipMemcpyAsync(nk.p, d_keys.p, (size_t)num_entries * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
                VB2_HIP(hipStreamSynchronize(s));
            }
            std::swap(ne.p, d_entries.p);
            std::swap(nk.p, d_keys.p);
            cap_entries = want;
        }
        if (add > 0)
            VB2_HIP(launch_cover_fill(d_desc.as<bamio::RecordDesc>(), (int64_t)nr, static_cast<const uint8_t*>(d_data), nb, filter,
                                      markers, d_offset.as<uint32_t>(), d_entries.as<PileEntry>() + num_entries,
                                      d_keys.as<uint64_t>() + num_entries, s, d_grp.as<uint16_t>(), adj_qual, adj_mapq));
        // (d_desc and d_offset are written again only by the next batch's copies, which the stream orders behind this fill)
        num_entries += (int64_t)add;
        ++num_batch;
    }
    VB2_HIP(hipStreamSynchronize(s));
    if (baq_stage && baq_stats) *baq_stats = baq_stage->stats;
    baq_stage.reset();

    // ---- sort by slot (file order within a slot), the overlap rule, the sites ----
    Dev d_keys2, d_idx, d_idx2, d_temp, d_sorted, d_qual, d_range, d_depth, d_off, d_rep, d_bases, d_quals;
    const size_t ne1 = std::max<size_t>((size_t)num_entries, 1), ns1 = (size_t)num_slot + 1;
    VB2_HIP(hipMalloc(&d_range.p, ns1 * 4));
    VB2_HIP(hipMalloc(&d_depth.p, ns1 * 4));
    VB2_HIP(hipMalloc(&d_off.p, ns1 * 4));
    VB2_HIP(hipMalloc(&d_rep.p, ns1));
    VB2_HIP(hipMalloc(&d_qual.p, ne1));
    VB2_HIP(hipMalloc(&d_sorted.p, ne1 * sizeof(PileEntry)));
    VB2_HIP(hipMalloc(&d_keys2.p, ne1 * sizeof(uint64_t)));
    size_t temp_bytes = 0;
    if (num_entries > 0) {
        VB2_HIP(hipMalloc(&d_idx.p, ne1 * 4));
        VB2_HIP(hipMalloc(&d_idx2.p, ne1 * 4));
        VB2_HIP(sort_entries(nullptr, &temp_bytes, d_keys.as<uint64_t>(), d_keys2.as<uint64_t>(), d_idx.as<uint32_t>(),
                             d_idx2.as<uint32_t>(), num_entries, s));
        VB2_HIP(hipMalloc(&d_temp.p, std::max<size_t>(temp_bytes, 1)));
        VB2_HIP(launch_iota_u32(d_idx.as<uint32_t>(), num_entries, s));
        VB2_HIP(sort_entries(d_temp.p, &temp_bytes, d_keys.as<uint64_t>(), d_keys2.as<uint64_t>(), d_idx.as<uint32_t>(),
                             d_idx2.as<uint32_t>(), num_entries, s));
        VB2_HIP(launch_gather(d_entries.as<PileEntry>(), d_idx2.as<uint32_t>(), d_sorted.as<PileEntry>(), num_entries, s));
    }
    VB2_HIP(launch_site_ranges(d_keys2.as<uint64_t>(), num_entries, num_slot, d_range.as<uint32_t>(), s));
    VB2_HIP(launch_overlap(d_sorted.as<PileEntry>(), d_range.as<uint32_t>(), num_entries, max_depth,
                           (conf.flag & kMplpSmartOverlaps) ? 1 : 0, d_qual.as<uint8_t>(), d_ctr.as<PileCounters>(), s));
    VB2_HIP(launch_sites(false, d_sorted.as<PileEntry>(), d_range.as<uint32_t>(), d_qual.as<uint8_t>(), num_slot, max_depth,
                         conf.min_baseQ, d_refnib.as<uint8_t>(), d_depth.as<uint32_t>(), d_rep.as<uint8_t>(), nullptr, nullptr,
                         nullptr, d_ctr.as<PileCounters>(), s));
    VB2_HIP(launch_scan_u32(d_depth.as<uint32_t>(), d_off.as<uint32_t>(), num_slot, d_total.as<unsigned long long>(), s));
    VB2_HIP(hipMemcpyAsync(h_total.p, d_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    VB2_HIP(hipStreamSynchronize(s));
    const unsigned long long total_bases = *static_cast<unsigned long long*>(h_total.p);
    if (total_bases > 0x7fffffffull) {
        set_error("pileup too large: more than 2 GiB of bases at the panel's sites");
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipMalloc(&d_bases.p, std::max<size_t>((size_t)total_bases, 1)));
    VB2_HIP(hipMalloc(&d_quals.p, std::max<size_t>((size_t)total_bases, 1)));
    VB2_HIP(launch_sites(true, d_sorted.as<PileEntry>(), d_range.as<uint32_t>(), d_qual.as<uint8_t>(), num_slot, max_depth,
                         conf.min_baseQ, d_refnib.as<uint8_t>(), d_depth.as<uint32_t>(), d_rep.as<uint8_t>(), d_off.as<uint32_t>(),
                         d_bases.as<char>(), d_quals.as<char>(), d_ctr.as<PileCounters>(), s));
    VB2_HIP(hipStreamSynchronize(s));
    const double t1 = now_s();

    // ---- stage 3: the pools back, the sites in .bed row order ----
    std::vector<uint32_t> depth((size_t)num_slot), off((size_t)num_slot);
    std::vector<uint8_t> rep((size_t)num_slot);
    std::string bases((size_t)total_bases, '\0'), quals((size_t)total_bases, '\0');
    PileCounters ctr{0, 0};
    if (num_slot > 0) {
        VB2_HIP(hipMemcpy(depth.data(), d_depth.p, (size_t)num_slot * 4, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(off.data(), d_off.p, (size_t)num_slot * 4, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(rep.data(), d_rep.p, (size_t)num_slot, hipMemcpyDeviceToHost));
    }
    if (total_bases > 0) {
        VB2_HIP(hipMemcpy(&bases[0], d_bases.p, (size_t)total_bases, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(&quals[0], d_quals.p, (size_t)total_bases, hipMemcpyDeviceToHost));
    }
    VB2_HIP(hipMemcpy(&ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
    int64_t empty_sites = 0;
    for (size_t row = 0; row < panel.PosVec.size(); ++row) {
        const int32_t slot = panel.rowSlot[row];
        if (slot < 0 || slot >= num_slot || !rep[(size_t)slot] || v->siteOfSlot[(size_t)slot] >= 0) continue;
        const uint32_t n = depth[(size_t)slot];
        if (n > 0) {
            v->effectiveNumSite++;
            v->numBases += (int)n;
        } else {
            ++empty_sites;
        }
        v->add_site(slot, bases.data() + off[(size_t)slot], quals.data() + off[(size_t)slot], n);
    }
    v->avgDepth = v->effectiveNumSite ? (double)v->numBases / v->effectiveNumSite : 0.0;
    if (stats) {
        stats->entries = num_entries;
        stats->batches = num_batch;
        stats->sites = v->num_site();
        stats->empty_sites = empty_sites;
        stats->pairs_resolved = (int64_t)ctr.pairs_resolved;
        stats->capped_sites = (int64_t)ctr.capped_sites;
        stats->seconds_device = t1 - t0;
        stats->seconds_copyback = now_s() - t1;
    }
    if (num_group == 0 || num_slot == 0) return VB2_OK;

    // ---- every read group's sites: a second key per sorted entry, a second sort, the site kernel over virtual slots ----
    const double g0 = now_s();
    const int32_t num_vslot = num_group * num_slot;
    const size_t nv1 = (size_t)num_vslot + 1;
    Dev d_qual2, d_range2, d_depth2, d_off2, d_rep2, d_gbases, d_gquals;
    VB2_HIP(hipMalloc(&d_range2.p, nv1 * 4));
    VB2_HIP(hipMalloc(&d_depth2.p, nv1 * 4));
    VB2_HIP(hipMalloc(&d_off2.p, nv1 * 4));
    VB2_HIP(hipMalloc(&d_rep2.p, nv1));
    VB2_HIP(hipMalloc(&d_qual2.p, ne1));
    // (the unsorted entries and their keys have been gathered: their arrays take the second keys and the second gather)
    PileEntry* const d_sorted2 = num_entries > 0 ? d_entries.as<PileEntry>() : d_sorted.as<PileEntry>();
    if (num_entries > 0) {
        VB2_HIP(launch_group_keys(d_sorted.as<PileEntry>(), d_range.as<uint32_t>(), num_entries, num_slot, num_group, max_depth,
                                  d_keys.as<uint64_t>(), s));
        VB2_HIP(launch_iota_u32(d_idx.as<uint32_t>(), num_entries, s));
        VB2_HIP(sort_entries(d_temp.p, &temp_bytes, d_keys.as<uint64_t>(), d_keys2.as<uint64_t>(), d_idx.as<uint32_t>(),
                             d_idx2.as<uint32_t>(), num_entries, s));
        VB2_HIP(launch_group_gather(d_sorted.as<PileEntry>(), d_qual.as<uint8_t>(), d_idx2.as<uint32_t>(), d_sorted2,
                                    d_qual2.as<uint8_t>(), num_entries, s));
    }
    VB2_HIP(launch_site_ranges(d_keys2.as<uint64_t>(), num_entries, num_vslot, d_range2.as<uint32_t>(), s));
    VB2_HIP(launch_group_sites(false, d_sorted2, d_range2.as<uint32_t>(), d_qual2.as<uint8_t>(), num_vslot, num_slot, conf.min_baseQ,
                               d_refnib.as<uint8_t>(), d_depth2.as<uint32_t>(), d_rep2.as<uint8_t>(), nullptr, nullptr, nullptr, s));
    VB2_HIP(launch_scan_u32(d_depth2.as<uint32_t>(), d_off2.as<uint32_t>(), num_vslot, d_total.as<unsigned long long>(), s));
    VB2_HIP(hipMemcpyAsync(h_total.p, d_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    VB2_HIP(hipStreamSynchronize(s));
    const unsigned long long group_bases = *static_cast<unsigned long long*>(h_total.p);
    if (group_bases > total_bases) {      // the groups partition a subset of the whole sample's bases
        set_error("--PerReadGroup: internal error: the groups hold more bases than the whole sample");
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipMalloc(&d_gbases.p, std::max<size_t>((size_t)group_bases, 1)));
    VB2_HIP(hipMalloc(&d_gquals.p, std::max<size_t>((size_t)group_bases, 1)));
    VB2_HIP(launch_group_sites(true, d_sorted2, d_range2.as<uint32_t>(), d_qual2.as<uint8_t>(), num_vslot, num_slot, conf.min_baseQ,
                               d_refnib.as<uint8_t>(), d_depth2.as<uint32_t>(), d_rep2.as<uint8_t>(), d_off2.as<uint32_t>(),
                               d_gbases.as<char>(), d_gquals.as<char>(), s));
    VB2_HIP(hipStreamSynchronize(s));
    const double g1 = now_s();
    depth.assign((size_t)num_vslot, 0u);
    off.assign((size_t)num_vslot, 0u);
    rep.assign((size_t)num_vslot, 0);
    bases.assign((size_t)group_bases, '\0');
    quals.assign((size_t)group_bases, '\0');
    VB2_HIP(hipMemcpy(depth.data(), d_depth2.p, (size_t)num_vslot * 4, hipMemcpyDeviceToHost));
    VB2_HIP(hipMemcpy(off.data(), d_off2.p, (size_t)num_vslot * 4, hipMemcpyDeviceToHost));
    VB2_HIP(hipMemcpy(rep.data(), d_rep2.p, (size_t)num_vslot, hipMemcpyDeviceToHost));
    if (group_bases > 0) {
        VB2_HIP(hipMemcpy(&bases[0], d_gbases.p, (size_t)group_bases, hipMemcpyDeviceToHost));
        VB2_HIP(hipMemcpy(&quals[0], d_gquals.p, (size_t)group_bases, hipMemcpyDeviceToHost));
    }
    for (int32_t g = 0; g < num_group; ++g) {      // as the whole sample's stage 3: .bed row order, a position listed twice once
        PileupViewer& gv = groups->flat[(size_t)g]->viewer;
        const size_t v0 = (size_t)g * (size_t)num_slot;
        for (size_t row = 0; row < panel.PosVec.size(); ++row) {
            const int32_t slot = panel.rowSlot[row];
            if (slot < 0 || slot >= num_slot || !rep[v0 + (size_t)slot] || gv.siteOfSlot[(size_t)slot] >= 0) continue;
            const uint32_t n = depth[v0 + (size_t)slot];
            if (n > 0) {
                gv.effectiveNumSite++;
                gv.numBases += (int)n;
            }
            gv.add_site(slot, bases.data() + off[v0 + (size_t)slot], quals.data() + off[v0 + (size_t)slot], n);
        }
        gv.avgDepth = gv.effectiveNumSite ? (double)gv.numBases / gv.effectiveNumSite : 0.0;
    }
    groups->seconds_device = g1 - g0;
    groups->seconds_copyback = now_s() - g1;
    return VB2_OK;
}

// the panel's markers per sequence name, (position, slot) ascending
void markers_by_sequence(const Panel& panel, std::vector<bamio::SeqMarkers>* seqs,
                         std::vector<std::vector<std::pair<int32_t, int32_t>>>* by_seq)
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

}  // namespace

// read_bam, and read_bam_groups with groups != nullptr
static int read_bam_impl(const std::string& bam_path, const Panel& panel, PileupViewer* v, const vb2_mpileup_opts* mp, int device,
                         vb2_bam_stats* stats, vb2_flat_groups* groups, const std::shared_ptr<Panel>& shared, const BamReadHow* how = nullptr,
                         const std::string& ref_path = std::string())
{
    MplpConf conf;
    conf.apply(mp);
    const int bam_adjust = how ? how->bam_adjust : 0;
    if (bam_adjust != 0 && bam_adjust != 1) {
        set_error("--BamFile: bam_adjust is " + std::to_string(bam_adjust) + "; it is 0 (records as they are) or 1 (--ApplyBAQ)");
        return VB2_ERR_INVALID;
    }
    std::vector<bamio::SeqMarkers> seqs;
    std::vector<std::vector<std::pair<int32_t, int32_t>>> by_seq;
    markers_by_sequence(panel, &seqs, &by_seq);
    // the file and its index first: no device is touched for an input that cannot be read
    bamio::Scan scan;
    std::string err;
    hipStream_t const stream = how ? static_cast<hipStream_t>(how->stream) : nullptr;
    const int threads = how && how->threads > 0 ? std::min(how->threads, 16) : reader_threads();
    // tunable bam_inflate: the planned blocks on the device.  Nothing of it exists without the
    // tunable, and the scan is then the one it was.
    std::unique_ptr<DeviceInflater> inflater;
    if (vb2::tunables().bam_inflate != 0) {
        if (usable_device_count() < 1) {
            set_error("--BamFile: bam_inflate = 1 asks for the device inflate and no gfx950 device is visible");
            return VB2_ERR_NO_DEVICE;
        }
        inflater.reset(new DeviceInflater(device, stream, (size_t)std::max(vb2::tunables().bam_batch_kb, 1) << 10));
    }
    if (int rc = bamio::scan(bam_path, seqs, threads, &scan, &err, groups != nullptr, inflater.get())) {
        set_error(err);
        return rc;                     // bamio's codes are the ABI's
    }
    inflater.reset();                  // (its staging buffers go before the pileup's come)
    if (groups) {
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
    }
    vb2_bam_stats local;
    if (!stats) stats = &local;
    host_stats(scan, stats);
    v->SEQ_SM = scan.sample;
    v->init(panel);
    v->numBases = 0;
    v->effectiveNumSite = 0;
    if (usable_device_count() < 1) {
        set_error("--BamFile: no gfx950 device is visible; the pileup of the decoded records runs on the GPU only "
                  "(there is no CPU fallback)");
        return VB2_ERR_NO_DEVICE;
    }
    if (!bam_adjust) return device_pileup(scan, by_seq, panel, conf, device, v, stats, groups, stream);
    // --ApplyBAQ: the spans of the FASTA the records can touch (not opened when the options ask for neither BAQ nor the cap)
    baq::Spans spans;
    if (int rc = baq::load_spans(scan, ref_path, baq::options_of(conf.flag, conf.capQ_thres), &spans, &err)) {
        set_error(err);
        return rc;
    }
    return device_pileup(scan, by_seq, panel, conf, device, v, stats, groups, stream, &spans, how->baq_stats);
}

int read_bam(const std::string& bam_path, const std::string& ref_path, const Panel& panel, PileupViewer* v, const vb2_mpileup_opts* mp,
             int device, vb2_bam_stats* stats, const BamReadHow* how)
{
    return read_bam_impl(bam_path, panel, v, mp, device, stats, nullptr, nullptr, how, ref_path);
}

int read_bam_groups(const std::string& bam_path, const std::shared_ptr<Panel>& panel, PileupViewer* v, const vb2_mpileup_opts* mp,
                    int device, vb2_bam_stats* stats, vb2_flat_groups* groups, const std::string& ref_path, const BamReadHow* how)
{
    if (!panel || !groups) {
        set_error("read_bam_groups: invalid argument");
        return VB2_ERR_INVALID;
    }
    return read_bam_impl(bam_path, *panel, v, mp, device, stats, groups, panel, how, ref_path);
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
    std::vector<std::vector<std::pair<int32_t, int32_t>>> by_seq;
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
    out->qual_off.push_back(0);
    auto var_bytes = [](const bamio::RecordDesc& d) {
        return (size_t)d.l_read_name + 4 * (size_t)d.n_cigar + ((size_t)d.l_seq + 1) / 2 + (size_t)d.l_seq;
    };
    if (where == 0) {
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
                int mq = d.mapq;
                uint8_t oc = t.outcome;
                if (oc == baq::kOutside) {
                    mq = -1;
                } else if (t.cap) {
                    mq = baq::capped_mapq(mq, baq::cap_finish(c4, opt.cap));
                    if (mq < 0) oc = baq::kCapDropped;
                }
                ++st.records;
                switch (oc) {
                case baq::kRealigned: ++st.realigned; break;
                case baq::kAlone: ++st.left_alone; break;
                case baq::kTagApplied: ++st.tag_applied; break;
                case baq::kNoReference: ++st.no_reference; break;
                case baq::kOutside: ++st.dropped_outside; break;
                case baq::kCapDropped: ++st.dropped_cap; break;
                default: ++st.not_asked; break;
                }
                out->qual.insert(out->qual.end(), q.begin(), q.end());
                out->qual_off.push_back(out->qual.size());
                out->mapq.push_back((int16_t)mq);
                out->outcome.push_back(oc);
                out->cap4.insert(out->cap4.end(), c4, c4 + 4);
            }
        }
        return VB2_OK;
    }
    if (usable_device_count() < 1) {
        set_error("vb2_baq_records: where = 1 runs the device stage and no gfx950 device is visible");
        return VB2_ERR_NO_DEVICE;
    }
    if (device >= 0) VB2_HIP(hipSetDevice(device));
    StreamHolder st;
    VB2_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    hipStream_t s = st.s;
    // the batches of device_pileup: closed by tunable bam_batch_kb
    size_t largest = 0, total_rec = 0;
    for (const bamio::Chunk& ch : scan.chunks) {
        total_rec += ch.recs.size();
        for (const bamio::RecordDesc& d : ch.recs) largest = std::max(largest, var_bytes(d));
    }
    const size_t batch_bytes = std::max<size_t>((size_t)std::max(vb2::tunables().bam_batch_kb, 1) << 10, largest);
    if (batch_bytes > 0xfff00000ull) { set_error("vb2_baq_records: bam_batch_kb asks for batches of 4 GiB or more"); return VB2_ERR_INVALID; }
    const size_t batch_rec = std::min<size_t>(std::max<size_t>(total_rec, 1), std::max<size_t>(batch_bytes / sizeof(bamio::RecordDesc), 1));
    std::vector<uint8_t> hd(batch_bytes);
    std::vector<bamio::RecordDesc> hr(batch_rec);
    Dev d_data, d_desc;
    VB2_HIP(hipMalloc(&d_data.p, batch_bytes));
    VB2_HIP(hipMalloc(&d_desc.p, batch_rec * sizeof(bamio::RecordDesc)));
    BaqStage stage(opt, s);
    if (int rc = stage.init(spans, batch_rec, batch_bytes)) return rc;
    std::vector<baq::Task> tasks;
    std::vector<uint8_t> extra;
    size_t ci = 0, ri = 0;
    auto skip_empty = [&] { while (ci < scan.chunks.size() && ri >= scan.chunks[ci].recs.size()) { ++ci; ri = 0; } };
    skip_empty();
    while (ci < scan.chunks.size()) {
        size_t nb = 0, nr = 0;
        tasks.clear();
        extra.clear();
        while (ci < scan.chunks.size() && nr < batch_rec) {
            const bamio::Chunk& ch = scan.chunks[ci];
            const bamio::RecordDesc& d = ch.recs[ri];
            const size_t vb = var_bytes(d);
            if ((size_t)d.data > ch.bytes.size() || vb > ch.bytes.size() - d.data) {
                set_error("vb2_baq_records: internal error: a record passes its chunk");
                return VB2_ERR_INVALID;
            }
            if (nb + vb > batch_bytes) break;
            std::memcpy(hd.data() + nb, ch.bytes.data() + d.data, vb);
            hr[nr] = d;
            hr[nr].data = (uint32_t)nb;
            const uint8_t* bq = nullptr;
            baq::Task t = baq::make_task(scan, ci, ri, spans, opt, &bq);
            if (t.kind == 1 && bq) {
                t.bq_off = (uint32_t)extra.size();
                extra.insert(extra.end(), bq, bq + d.l_seq);
            }
            tasks.push_back(t);
            nb += vb;
            ++nr;
            ++ri;
            skip_empty();
        }
        VB2_HIP(hipMemcpyAsync(d_data.p, hd.data(), nb, hipMemcpyHostToDevice, s));
        VB2_HIP(hipMemcpyAsync(d_desc.p, hr.data(), nr * sizeof(bamio::RecordDesc), hipMemcpyHostToDevice, s));
        VB2_HIP(hipStreamSynchronize(s));
        const size_t q0 = out->qual.size();
        if (int rc = stage.run(tasks, extra, hr.data(), nr, d_desc.as<bamio::RecordDesc>(), d_data.as<uint8_t>(), nb, &out->cap4, &out->mapq,
                               &out->outcome, &out->qual))
            return rc;
        size_t at = q0;
        for (size_t r = 0; r < nr; ++r) {
            at += (size_t)hr[r].l_seq;
            out->qual_off.push_back(at);
        }
    }
    out->stats = stage.stats;
    return VB2_OK;
}

bool bam_support() { return true; }

// Stage 1 alone (vb2_bam_scan): no device
int bam_scan_file(const std::string& bam_path, const std::string& bed_path, std::vector<uint64_t>* voffsets, vb2_bam_stats* stats,
                  std::string* sample, std::vector<std::string>* group_ids, std::vector<uint16_t>* groups)
{
    Panel panel;
    if (int rc = read_bed(bed_path, &panel)) return rc;
    std::vector<bamio::SeqMarkers> seqs;
    std::vector<std::vector<std::pair<int32_t, int32_t>>> by_seq;
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

#endif
