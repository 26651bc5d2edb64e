// hostio.h -- host-side input adapters and writers for the --SVDPrefix /
// --PileupFile flow: the "flatten once" stage that feeds vb2_ctx_create.
//
// Mirrors (file:line relative to the reference root):
//   ReadChooseBed / ReadMatrixUD / ReadMean / ReadAF   ContaminationEstimator.cpp:342-487
//   SimplePileupViewer::ReadPileup                     SimplePileupViewer.cpp:711-833
//   BuildResolvedMarkers                               ContaminationEstimator.cpp:67-86
//   IsSanityCheckOK                                    ContaminationEstimator.cpp:543-587
//   .Ancestry / .selfSM / .Pileup writers              ContaminationEstimator.cpp:168-188, main.cpp:336-411
#ifndef VB2_HOSTIO_H_
#define VB2_HOSTIO_H_

#include <cstdint>
#include <functional>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/vb2_abi.h"

struct vb2_flat_groups;

namespace vb2 {

// The .bed rows name positions; a position listed twice is ONE entry of the reference's
// ChooseBed[chr][pos] map (the later row's alleles win, cpp:433).  Here every distinct (chr, pos)
// gets a dense id in order of first appearance -- a "slot" -- so that everything per position is a
// flat array: one hash lookup per pileup line, none per marker afterwards.
struct Panel {
    int numPC = 0;
    uint32_t NumMarker = 0;                               // rows of .UD (cpp:366)
    std::vector<double> UD;                               // NumMarker x numPC
    std::vector<double> means;
    std::vector<std::pair<std::string, int>> PosVec;      // cpp:432 (pos is 1-based)
    // ChooseBed (cpp:433) as slots
    std::unordered_map<std::string, std::unordered_map<int, int32_t>> slotOf;   // (chr, pos) -> slot
    std::vector<int32_t> rowSlot;                         // PosVec row -> slot
    std::vector<char> slotRef, slotAlt;                   // ChooseBed[chr][pos].first / .second
    std::vector<int32_t> slotPos, slotChr;                // the slot's position; index into chrNames
    std::vector<std::string> chrNames;
    bool isAFknown = false;
    std::unordered_map<std::string, std::unordered_map<uint32_t, double>> knownAF;
    std::vector<double> slotAF;                           // knownAF[chr][pos] per slot (0 where the AF file has no row)
    size_t num_slot() const { return slotPos.size(); }
    int32_t find_slot(const std::string& chr, int pos) const
    {
        auto c = slotOf.find(chr);
        if (c == slotOf.end()) return -1;
        auto s = c->second.find(pos);
        return s == c->second.end() ? -1 : s->second;
    }
    void finish();                                        // after read_bed (+ read_known_af): slotAF
};

// SimplePileupViewer.h:84-147: baseInfo / qualInfo / posIndex.  A "site" is a pileup line whose
// position is in the .bed, numbered in order of appearance (the reference's global index); its
// parsed bases and qualities sit back to back in two pools instead of one std::string each.
struct PileupViewer {
    std::string basePool, qualPool;
    std::vector<uint32_t> siteOff{0};                     // site s owns [siteOff[s], siteOff[s + 1])
    std::vector<int32_t> siteOfSlot;                      // panel slot -> site, -1 = not in the pileup (posIndex)
    std::string SEQ_SM = "DefaultSampleName";
    int numBases = 0;
    int effectiveNumSite = 0;
    double avgDepth = 0;
    double sdDepth = 0;
    void init(const Panel& p)
    {
        siteOfSlot.assign(p.num_slot(), -1);
        siteOff.assign(1, 0u);
        basePool.clear();
        qualPool.clear();
    }
    int num_site() const { return (int)siteOff.size() - 1; }
    int32_t site_of(int32_t slot) const { return slot >= 0 && (size_t)slot < siteOfSlot.size() ? siteOfSlot[slot] : -1; }
    uint32_t depth(int32_t site) const { return siteOff[site + 1] - siteOff[site]; }
    const char* bases(int32_t site) const { return basePool.data() + siteOff[site]; }
    const char* quals(int32_t site) const { return qualPool.data() + siteOff[site]; }
    // a new site for `slot` with n parsed (base, quality) pairs
    void add_site(int32_t slot, const char* b, const char* q, size_t n)
    {
        if (basePool.size() + n > 0xffffffffull)      // (32-bit site offsets; the callers turn this into VB2_ERR_INVALID)
            throw std::length_error("pileup too large: more than 4 GiB of bases at the panel's sites");
        siteOfSlot[slot] = num_site();
        basePool.append(b, n);
        qualPool.append(q, n);
        siteOff.push_back((uint32_t)basePool.size());
    }
};

int read_bed(const std::string& path, Panel* p);
int read_ud(const std::string& path, Panel* p);
int read_mean(const std::string& path, Panel* p);
int read_known_af(const std::string& path, Panel* p);
int read_pileup(const std::string& path, const Panel& panel, PileupViewer* v);
// BAM input (bam_flatten.cpp): the built-in reader -- BGZF, header, .bai and records on the host (bam_io.cpp), the pileup
// on `device` (bam_pileup_kernels.hip) --, or htslib's where the library was configured with
// VB2_WITH_HTSLIB.  SimplePileupViewer.cpp:172-557 with main.cpp:81-96's defaults; BAQ and the mapQ cap under
// BamReadHow::bam_adjust alone.
// mp: the reference's "Pileup Options" (main.cpp:176-187), nullptr or given == 0 = its defaults (main.cpp:81-96);
// stats (may be null): what vb2_flat_bam_stats reports.  The file and its index are opened before any device is touched.
// how: what a caller that runs many loads at once decides for one of them (null: the tunables and a stream of its own)
struct BamReadHow {
    int threads = 0;          // host pool that inflates and walks: 0 = tunable bam_threads
    void* stream = nullptr;   // hipStream_t of the device stage (and of the device inflate): null = one made for the load
    // --ApplyBAQ (vb2_run_args.bam_adjust = 1): the built-in reader applies the shift, BAQ and the cap
    // the options ask for from the FASTA at ref_path; baq_stats (may be null) gets what vb2_flat_baq_stats reports
    int bam_adjust = 0;
    vb2_baq_stats* baq_stats = nullptr;
};
int read_bam(const std::string& bam_path, const std::string& ref_path, const Panel& panel, PileupViewer* v,
             const vb2_mpileup_opts* mp = nullptr, int device = -1, vb2_bam_stats* stats = nullptr, const BamReadHow* how = nullptr);
// A line of a cohort's list (vb2_cohort_args.pileup_paths): by its name a BAM (".bam": the built-in reader), a CRAM
// (".cram": refused with cram_message) or a text pileup (anything else; a file that starts with the CRAM magic is refused
// like a ".cram" name).
enum class ListEntry { kText = 0, kBam = 1, kCram = 2 };
ListEntry classify_list_entry(const std::string& path);
bool has_cram_magic(const std::string& path);
std::string cram_message(const std::string& path);
// The vb2_bam_stats of the .bam lines of the process's most recent cohort run (vb2_cohort_bam_stats), and the most .bam
// lines that were between "file opened" and "context created" at once on one device in it.
void cohort_bam_stats_reset(int num_sample);
void cohort_bam_stats_put(int sample, const vb2_bam_stats& st);
bool cohort_bam_stats_get(int sample, vb2_bam_stats* out);
void cohort_bam_peak_note(int inflight);
int cohort_bam_peak();
// the host pool of one BAM load among `readers` loads at once: the process keeps to 16 busy host threads
inline int cohort_bam_pool(int readers) { return readers >= 16 ? 1 : (readers < 1 ? 16 : 16 / readers); }
// read_bam, and every read group of the header beside the whole sample (built-in reader only):
// groups->info and groups->flat are filled, one vb2_flat per @RG line over `panel` with its viewer's sites added; the whole sample's viewer and stats are what
// read_bam gives.  VB2_ERR_INVALID for a header whose groups x panel slots pass 2^31 - 2, before any device is touched.
int read_bam_groups(const std::string& bam_path, const std::shared_ptr<Panel>& panel, PileupViewer* v, const vb2_mpileup_opts* mp,
                    int device, vb2_bam_stats* stats, vb2_flat_groups* groups, const std::string& ref_path = std::string(),
                    const BamReadHow* how = nullptr);
bool bam_support();
// vb2_baq_records: what --ApplyBAQ makes of the records the scan sends up (where 0: the host driver, 1: the device stage)
struct BaqRecords;      // baq_host.h
int baq_records_file(const std::string& bam_path, const std::string& bed_path, const std::string& ref_path, const vb2_mpileup_opts* mp,
                     int where, int device, BaqRecords* out);
// the host stage alone over the markers of a .bed (vb2_bam_scan): the fetched records' virtual offsets, ascending;
// group_ids / groups (both or neither): the header's @RG IDs and the records' group numbers (vb2_bam_scan_ex)
int bam_scan_file(const std::string& bam_path, const std::string& bed_path, std::vector<uint64_t>* voffsets, vb2_bam_stats* stats,
                  std::string* sample, std::vector<std::string>* group_ids = nullptr, std::vector<uint16_t>* groups = nullptr);
bool sanity_check(const Panel& p, PileupViewer* v);

}  // namespace vb2

// The flattened, panel-ordered arrays behind a vb2_input (owned here).
struct vb2_flat {
    std::shared_ptr<vb2::Panel> panel_ptr;    // one panel can serve a whole cohort of samples
    vb2::Panel& panel;                        // = *panel_ptr
    vb2_flat() : panel_ptr(std::make_shared<vb2::Panel>()), panel(*panel_ptr) {}
    explicit vb2_flat(std::shared_ptr<vb2::Panel> shared) : panel_ptr(std::move(shared)), panel(*panel_ptr) {}
    vb2_flat(const vb2_flat&) = delete;
    vb2_flat& operator=(const vb2_flat&) = delete;
    vb2::PileupViewer viewer;
    std::vector<int64_t> read_off;
    std::string bases, quals;
    std::vector<char> alt_base;
    std::vector<double> known_af;
    int32_t num_site = 0;
    bool sanity_disabled = true;
    bool from_bam = false;                    // bam_stats holds the load's counts and times
    vb2_bam_stats bam_stats{};
    bool with_baq = false;                    // loaded with bam_adjust = 1: baq_stats holds the stage's
    vb2_baq_stats baq_stats{};
    vb2_input input{};
    void resolve();          // BuildResolvedMarkers -> input
};

// The read groups of one BAM (vb2_flat_load_groups): per @RG line of the header, in header order, a vb2_flat over the whole
// sample's panel.
struct vb2_flat_groups {
    struct Info {
        std::string id, sm, lb, pu;
        int64_t records = 0;                  // kept records that name the group
        int32_t status = VB2_OK;              // VB2_OK, VB2_ERR_SANITY, or VB2_GROUP_NO_BASE
    };
    std::vector<Info> info;
    std::vector<std::unique_ptr<vb2_flat>> flat;
    int64_t unassigned = 0;                   // kept records of no group
    double seconds_device = 0, seconds_copyback = 0;      // of the groups' part of the load alone
};

namespace vb2 {
// <prefix>.selfRG: .selfSM's header and one row per group; est[g] is read where searched[g] != 0
int write_selfrg(const std::string& prefix, const vb2_flat_groups& groups, const vb2_estimate* est, const uint8_t* searched);
int write_ancestry(const std::string& prefix, int numPC, const double* pc, const double* pc2);
int write_selfsm(const std::string& prefix, const vb2_flat& f, const vb2_estimate& est,
                 bool pileup_input);
int write_pileup(const std::string& prefix, const vb2_flat& f);      // <prefix>.Pileup
void print_summary(const char* title, int numPC, const vb2_estimate& est);
// <prefix>.PairFit (vb2_cohort_run_paired): names [num_sample], fit [num_pair]
int write_pair_fit(const std::string& prefix, int num_pair, const char* const* names, const vb2_pair_fit* fit);
// <prefix>.PairCI (--PairInterval): ci / ci_status [num_pair], the interval of pair p's refit and its own code
int write_pair_ci(const std::string& prefix, int num_pair, const char* const* names, const vb2_pair_fit* fit, const vb2_interval* ci,
                  const int32_t* ci_status);
// VB2_ERR_INVALID with a message for an index out of range, a sample paired with itself or a tumour listed twice
int check_pairs(const char* who, int num_sample, int num_pair, const int32_t* tumour, const int32_t* normal);
// The tables' one way to a file: opens `name`, lets body write, closes; VB2_ERR_IO with the reference's message for a
// file that cannot be opened or for one whose stream failed by the time it is closed.
int write_text_file(const std::string& name, const std::function<void(std::ostream&)>& body);
}  // namespace vb2

#endif
