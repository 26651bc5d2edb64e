// abi_input.cpp -- the input side of the extern "C" surface declared in include/vb2_abi.h: a sample's loaded files
// (vb2_flat_*), the BAM reader's diagnostics (vb2_baq_*, vb2_bam_scan_*, vb2_bgzf_inflate*, vb2_fasta_fetch) and what a
// cohort run reports about its BAM lines.  Contexts, searches and runs: abi.cpp.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "baq_host.h"
#include "bgzf_inflate_kernels.h"
#include "context.h"
#include "fasta_io.h"
#include "guard.h"
#include "hostio.h"
#include "run.h"
#include "tunables.h"

using vb2::set_error;

struct vb2_baq_result {
    vb2::BaqRecords r;
};

struct vb2_bam_scan_result {
    std::vector<uint64_t> voffset;
    vb2_bam_stats stats;
    std::string sample;
    std::vector<std::string> group_id;      // with VB2_BAM_SCAN_GROUPS
    std::vector<uint16_t> group;            // ... parallel to voffset
};

extern "C" {

int vb2_flat_load(const vb2_run_args* a, vb2_flat** out) { return vb2::flat_load(a, out, nullptr); }

int vb2_flat_load_groups(const vb2_run_args* a, vb2_flat** whole, vb2_flat_groups** groups)
{
    if (!groups || !whole) {
        set_error("vb2_flat_load_groups: invalid argument");
        return VB2_ERR_INVALID;
    }
    *groups = nullptr;
    *whole = nullptr;
    std::unique_ptr<vb2_flat_groups> g(new (std::nothrow) vb2_flat_groups());
    if (!g) return VB2_ERR_NOMEM;
    const int rc = vb2::flat_load(a, whole, g.get());
    if (*whole) *groups = g.release();
    return rc;
}

int32_t vb2_flat_groups_count(const vb2_flat_groups* g) { return g ? (int32_t)g->info.size() : 0; }

const char* vb2_flat_groups_id(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->info.size() ? g->info[(size_t)i].id.c_str() : nullptr;
}

int64_t vb2_flat_groups_records(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->info.size() ? g->info[(size_t)i].records : 0;
}

int32_t vb2_flat_groups_status(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->info.size() ? g->info[(size_t)i].status : (int32_t)VB2_ERR_INVALID;
}

const vb2_flat* vb2_flat_groups_flat(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->flat.size() ? g->flat[(size_t)i].get() : nullptr;
}

int64_t vb2_flat_groups_unassigned(const vb2_flat_groups* g) { return g ? g->unassigned : 0; }

int vb2_flat_groups_seconds(const vb2_flat_groups* g, double* seconds_device, double* seconds_copyback)
{
    if (!g || !seconds_device || !seconds_copyback) return VB2_ERR_INVALID;
    *seconds_device = g->seconds_device;
    *seconds_copyback = g->seconds_copyback;
    return VB2_OK;
}

void vb2_flat_groups_free(vb2_flat_groups* g) { delete g; }

const vb2_input* vb2_flat_input(const vb2_flat* f) { return f ? &f->input : nullptr; }

int vb2_flat_stats(const vb2_flat* f, vb2_run_result* out)
{
    if (!f || !out) return VB2_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->num_marker = (int32_t)f->panel.NumMarker;
    out->num_site = f->num_site;
    out->num_bases = f->viewer.numBases;
    out->avg_depth = f->viewer.avgDepth;
    out->sd_depth = f->viewer.sdDepth;
    return VB2_OK;
}

void vb2_flat_free(vb2_flat* f) { delete f; }

int vb2_flat_bam_stats(const vb2_flat* f, vb2_bam_stats* out)
{
    if (!f || !out || !f->from_bam) {
        set_error("vb2_flat_bam_stats: not a vb2_flat loaded from a BAM");
        return VB2_ERR_INVALID;
    }
    *out = f->bam_stats;
    return VB2_OK;
}

int vb2_flat_baq_stats(const vb2_flat* f, vb2_baq_stats* out)
{
    if (!f || !out || !f->with_baq) {
        set_error("vb2_flat_baq_stats: not a vb2_flat loaded from a BAM with bam_adjust = 1");
        return VB2_ERR_INVALID;
    }
    *out = f->baq_stats;
    return VB2_OK;
}

int vb2_baq_records(const char* bam_path, const char* bed_path, const char* reference_path, const vb2_mpileup_opts* opts, int where,
                    int device, vb2_baq_result** out)
{
    if (!bam_path || !bed_path || !out) {
        set_error("vb2_baq_records: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        std::unique_ptr<vb2_baq_result> r(new vb2_baq_result());
        if (int rc = vb2::baq_records_file(bam_path, bed_path, reference_path ? reference_path : "", opts, where, device, &r->r)) return rc;
        *out = r.release();
        return VB2_OK;
    });
}

int64_t vb2_baq_result_num(const vb2_baq_result* r) { return r ? (int64_t)r->r.outcome.size() : 0; }
int64_t vb2_baq_result_qual_bytes(const vb2_baq_result* r) { return r ? (int64_t)r->r.qual.size() : 0; }

int vb2_baq_result_copy(const vb2_baq_result* r, uint64_t* qual_off, uint8_t* qual, int16_t* mapq, uint8_t* outcome, int32_t* cap4)
{
    if (!r) return VB2_ERR_INVALID;
    const vb2::BaqRecords& b = r->r;
    if (qual_off) std::copy(b.qual_off.begin(), b.qual_off.end(), qual_off);
    if (qual) std::copy(b.qual.begin(), b.qual.end(), qual);
    if (mapq) std::copy(b.mapq.begin(), b.mapq.end(), mapq);
    if (outcome) std::copy(b.outcome.begin(), b.outcome.end(), outcome);
    if (cap4) std::copy(b.cap4.begin(), b.cap4.end(), cap4);
    return VB2_OK;
}

int vb2_baq_result_stats(const vb2_baq_result* r, vb2_baq_stats* out)
{
    if (!r || !out) return VB2_ERR_INVALID;
    *out = r->r.stats;
    return VB2_OK;
}

void vb2_baq_result_free(vb2_baq_result* r) { delete r; }

int vb2_baq_case(const uint8_t* ref, int32_t l_ref, const uint8_t* query, const uint8_t* qual, int32_t l_query, int32_t bw, int32_t* state,
                 uint8_t* q, int32_t* undefined)
{
    if (l_query < 0 || l_ref < 0 || bw < 0 || (l_query > 0 && (!query || !qual || !state || !q)) || (l_ref > 0 && !ref)) {
        set_error("vb2_baq_case: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        const int u = vb2::baq::run_case(ref, l_ref, query, qual, l_query, bw, state, q);
        if (undefined) *undefined = u;
        return VB2_OK;
    });
}

int32_t vb2_baq_quantise(double z) { return vb2::baq::quantise(vb2::baq::tables().thresh, z); }

uint64_t vb2_baq_work_bytes(int32_t l_ref, int32_t l_query, int32_t bw) { return vb2::baq::work_bytes(l_ref, l_query, bw); }

int vb2_fasta_fetch(const char* fasta_path, const char* name, int64_t beg, int64_t end, uint8_t* out, int64_t* length)
{
    if (!fasta_path || !name) {
        set_error("vb2_fasta_fetch: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        vb2::fasta::Index idx;
        std::string err;
        if (int rc = vb2::fasta::open_index(fasta_path, &idx, &err)) {
            set_error(err);
            return rc;
        }
        const int s = idx.find(name);
        if (s < 0) {
            set_error(std::string("--Reference: ") + fasta_path + " has no sequence " + name);
            return VB2_ERR_INVALID;
        }
        if (length) *length = idx.seqs[(size_t)s].length;
        if (!out) return VB2_OK;
        if (beg < 0 || end < beg || end > idx.seqs[(size_t)s].length) {
            set_error("vb2_fasta_fetch: the span passes the sequence");
            return VB2_ERR_INVALID;
        }
        if (int rc = vb2::fasta::fetch_nt16(idx, s, beg, end, out, &err)) {
            set_error(err);
            return rc;
        }
        return VB2_OK;
    });
}

int vb2_bam_scan_ex(const char* bam_path, const char* bed_path, uint32_t flags, vb2_bam_scan_result** out)
{
    if (!bam_path || !bed_path || !out || (flags & ~VB2_BAM_SCAN_GROUPS)) {
        set_error("vb2_bam_scan: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        std::unique_ptr<vb2_bam_scan_result> s(new vb2_bam_scan_result());
        const bool want = (flags & VB2_BAM_SCAN_GROUPS) != 0;
        if (int rc = vb2::bam_scan_file(bam_path, bed_path, &s->voffset, &s->stats, &s->sample, want ? &s->group_id : nullptr,
                                        want ? &s->group : nullptr))
            return rc;
        *out = s.release();
        return VB2_OK;
    });
}

int vb2_bam_scan(const char* bam_path, const char* bed_path, vb2_bam_scan_result** out) { return vb2_bam_scan_ex(bam_path, bed_path, 0, out); }

int32_t vb2_bam_scan_num_group(const vb2_bam_scan_result* scan) { return scan ? (int32_t)scan->group_id.size() : 0; }

const char* vb2_bam_scan_group_id(const vb2_bam_scan_result* scan, int32_t group)
{
    return scan && group >= 0 && (size_t)group < scan->group_id.size() ? scan->group_id[(size_t)group].c_str() : nullptr;
}

int64_t vb2_bam_scan_record_groups(const vb2_bam_scan_result* scan, uint16_t* group, int64_t capacity)
{
    if (!scan) return VB2_ERR_INVALID;
    const int64_t n = (int64_t)scan->group.size();
    for (int64_t i = 0; group && i < n && i < capacity; ++i) group[i] = scan->group[(size_t)i];
    return n;
}

int vb2_bam_scan_stats(const vb2_bam_scan_result* scan, vb2_bam_stats* out)
{
    if (!scan || !out) return VB2_ERR_INVALID;
    *out = scan->stats;
    return VB2_OK;
}

int64_t vb2_bam_scan_records(const vb2_bam_scan_result* scan, uint64_t* voffset, int64_t capacity)
{
    if (!scan) return VB2_ERR_INVALID;
    const int64_t n = (int64_t)scan->voffset.size();
    for (int64_t i = 0; voffset && i < n && i < capacity; ++i) voffset[i] = scan->voffset[(size_t)i];
    return n;
}

const char* vb2_bam_scan_sample(const vb2_bam_scan_result* scan) { return scan ? scan->sample.c_str() : ""; }

void vb2_bam_scan_free(vb2_bam_scan_result* scan) { delete scan; }

int vb2_bgzf_inflate(const uint8_t* file_bytes, int64_t n_bytes, int32_t device, uint8_t* out, int64_t out_capacity, int64_t* out_bytes,
                     int32_t* block_status, int32_t status_capacity, int32_t* num_block)
{
    if (n_bytes < 0 || (!file_bytes && n_bytes > 0) || out_capacity < 0 || (!out && out_capacity > 0) || !out_bytes || status_capacity < 0 ||
        (!block_status && status_capacity > 0) || !num_block) {
        set_error("vb2_bgzf_inflate: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out_bytes = 0;
    *num_block = 0;
    return vb2::guarded([&]() -> int {
        if (vb2::usable_device_count() < 1) {
            set_error("vb2_bgzf_inflate: no gfx950 device is visible (the host's inflate is zlib's, not this entry's)");
            return VB2_ERR_NO_DEVICE;
        }
        std::string err;
        const size_t batch = (size_t)std::max(vb2::tunables().bam_batch_kb, 1) << 10;
        const int rc = vb2::bgzf_inflate_buffer(file_bytes, (uint64_t)n_bytes, device, batch, out, out_capacity, out_bytes, block_status,
                                                status_capacity, num_block, &err);
        if (rc) set_error(err);
        return rc;                     // bamio's codes are the ABI's
    });
}

int vb2_cohort_bam_stats(int32_t sample, vb2_bam_stats* out)
{
    if (!out || !vb2::cohort_bam_stats_get(sample, out)) {
        set_error("vb2_cohort_bam_stats: not a sample of the last cohort run that was read from a BAM");
        return VB2_ERR_INVALID;
    }
    return VB2_OK;
}

// (tests) how a cohort treats a line of its list (0 text, 1 BAM, 2 CRAM, by name and by the CRAM magic), the host pool
// of one of its BAM loads among `readers` reader threads, and the most BAM loads in flight on one device in the last run
int vb2_debug_list_entry_kind(const char* path)
{
    if (!path) return -1;
    vb2::ListEntry k = vb2::classify_list_entry(path);
    if (k == vb2::ListEntry::kText && vb2::has_cram_magic(path)) k = vb2::ListEntry::kCram;
    return (int)k;
}
int vb2_debug_cohort_bam_pool(int readers) { return vb2::cohort_bam_pool(readers); }
int vb2_debug_cohort_bam_peak(void) { return vb2::cohort_bam_peak(); }

int vb2_bgzf_inflate_stats(vb2_bgzf_stats* out, int32_t reset)
{
    if (!out && !reset) return VB2_ERR_INVALID;
    vb2::InflateTotals t;
    vb2::inflate_totals(&t, reset != 0);
    if (out) {
        out->blocks = t.blocks;
        out->refused = t.refused;
        out->batches = t.batches;
        out->bytes_raw = t.bytes_raw;
        out->bytes_inflated = t.bytes_inflated;
        out->seconds_upload = t.seconds_upload;
        out->seconds_kernel = t.seconds_kernel;
        out->seconds_copyback = t.seconds_copyback;
        out->seconds_stage = t.seconds_stage;
    }
    return VB2_OK;
}

}  // extern "C"
