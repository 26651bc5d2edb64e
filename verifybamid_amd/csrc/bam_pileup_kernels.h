// bam_pileup_kernels.h -- the device stage of the built-in BAM reader (bam_pileup_kernels.hip):
// decoded records -> one entry per (record, covered marker) in file order -> the per-site bases and qualities of a
// PileupViewer.
#ifndef VB2_BAM_PILEUP_KERNELS_H_
#define VB2_BAM_PILEUP_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "bam_io.h"

namespace vb2 {

// One record over one marker.  bits: the base's 4-bit code | reverse << 4 | deleted (D or N) << 5 | pair-eligible << 6
// | (mate position >= own position) << 7.
struct PileEntry {
    uint64_t name;          // device address of the read name in its batch's bytes (kept until the sites are written)
    uint64_t hash;          // FNV-1a of the name
    uint32_t order;         // the record's file-order number
    int32_t slot;           // the marker's panel slot
    uint8_t qual;
    uint8_t bits;
    uint8_t l_name;
    uint8_t pad0;
    uint16_t group;         // the record's read group (bamio::kNoGroup = none); 0 in a load that was not asked for groups
    uint8_t pad[2];
};
static_assert(sizeof(PileEntry) == 32, "entries are 32 bytes");
constexpr uint8_t kEntryReverse = 16, kEntryDeleted = 32, kEntryEligible = 64, kEntryMateAhead = 128;

struct PileFilter {         // mplp_func's read filter (SimplePileupViewer.cpp:172-237); BAQ and the mapQ cap reach it as adjusted values
    int32_t excl_flags, min_mq, no_orphans;
};

// The markers of the BAM's sequences: tid t owns [tid_lo[t], tid_lo[t + 1]) of pos (1-based, ascending) and slot.
struct PileMarkers {
    const int32_t* tid_lo;
    const int32_t* pos;
    const int32_t* slot;
    int32_t n_ref;
};

struct PileCounters {       // device-side statistics, added to by the kernels
    unsigned long long pairs_resolved, capped_sites;
};

// Pass 1 of a batch: count[r] = markers record r covers (0 for a filtered record).  data: the batch's record bytes.
// adj_qual / adj_mapq (both or neither; --ApplyBAQ): the qualities after BAQ, at the offsets `data`
// has the records' own, and the mapQ after the cap per record, below zero for a dropped read.  Without them the kernels
// are the instantiations they were.
hipError_t launch_cover_count(const bamio::RecordDesc* desc, int64_t num_rec, const uint8_t* data, uint64_t data_bytes,
                              PileFilter f, PileMarkers m, uint32_t* count, hipStream_t s, const uint8_t* adj_qual = nullptr,
                              const int16_t* adj_mapq = nullptr);
// offset = exclusive scan of count [n], *total = its sum (a single workgroup walks the array)
hipError_t launch_scan_u32(const uint32_t* count, uint32_t* offset, int64_t n, unsigned long long* total, hipStream_t s);
// Pass 2: record r's entries go to entries[offset[r] ...], and their sort keys slot << 32 | order to keys[...].
// group (may be null): the records' read groups, parallel to desc; null leaves every entry's group 0.
hipError_t launch_cover_fill(const bamio::RecordDesc* desc, int64_t num_rec, const uint8_t* data, uint64_t data_bytes,
                             PileFilter f, PileMarkers m, const uint32_t* offset, PileEntry* entries, uint64_t* keys,
                             hipStream_t s, const uint16_t* group = nullptr, const uint8_t* adj_qual = nullptr,
                             const int16_t* adj_mapq = nullptr);

// Sorts the keys with the entries' indices: keys_out ascending, idx_out the permutation (n < 2^31).  temp / temp_bytes as
// hipcub wants them: call with temp == nullptr to learn temp_bytes.
hipError_t sort_entries(void* temp, size_t* temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* idx_in,
                        uint32_t* idx_out, int64_t n, hipStream_t s);
hipError_t launch_iota_u32(uint32_t* idx, int64_t n, hipStream_t s);
hipError_t launch_gather(const PileEntry* entries, const uint32_t* perm, PileEntry* sorted, int64_t n, hipStream_t s);
// range[s] = first sorted entry of a slot >= s, s in [0, num_slot]: slot s owns the sorted entries [range[s], range[s + 1])
hipError_t launch_site_ranges(const uint64_t* keys, int64_t n, int32_t num_slot, uint32_t* range, hipStream_t s);

// The mate-overlap rule over the sorted entries: qual_out[i] = entry i's quality afterwards.  smart == 0: qualities as
// they are.  The depth cap applies first: entries behind a site's first max_depth are left alone.
hipError_t launch_overlap(const PileEntry* sorted, const uint32_t* range, int64_t n, int32_t max_depth, int32_t smart,
                          uint8_t* qual_out, PileCounters* ctr, hipStream_t s);

// Per slot: fill == false: depth[slot] = bases the site stores, reported[slot] = some record spans it; fill == true: the
// characters at base_pool / qual_pool + offset[slot].  ref_nib: the 4-bit code of the panel's REF allele per slot.
hipError_t launch_sites(bool fill, const PileEntry* sorted, const uint32_t* range, const uint8_t* qual, int32_t num_slot,
                        int32_t max_depth, int32_t min_bq, const uint8_t* ref_nib, uint32_t* depth, uint8_t* reported,
                        const uint32_t* offset, char* base_pool, char* qual_pool, PileCounters* ctr, hipStream_t s);

// ---- per-read-group sites ----
// A group's site is a "virtual slot" v = group * num_slot + slot, v < num_group * num_slot <= 2^31 - 2.
// Per sorted entry i: keys[i] = v << 32 | order when the entry lies within its site's first max_depth entries and has a
// group below num_group, all ones otherwise (those sort behind every virtual slot and belong to nobody).
hipError_t launch_group_keys(const PileEntry* sorted, const uint32_t* range, int64_t n, int32_t num_slot, int32_t num_group,
                             int32_t max_depth, uint64_t* keys, hipStream_t s);
// sorted2[i] = sorted[perm[i]], qual2[i] = qual[perm[i]] (the quality after the overlap rule travels with its entry)
hipError_t launch_group_gather(const PileEntry* sorted, const uint8_t* qual, const uint32_t* perm, PileEntry* sorted2,
                               uint8_t* qual2, int64_t n, hipStream_t s);
// launch_sites over virtual slots: no depth cap (it was applied to the whole site), the REF nibble of slot v % num_slot,
// no counters.  range: launch_site_ranges of the second sort's keys with num_vslot for num_slot.
hipError_t launch_group_sites(bool fill, const PileEntry* sorted2, const uint32_t* range, const uint8_t* qual2, int32_t num_vslot,
                              int32_t num_slot, int32_t min_bq, const uint8_t* ref_nib, uint32_t* depth, uint8_t* reported,
                              const uint32_t* offset, char* base_pool, char* qual_pool, hipStream_t s);

}  // namespace vb2

#endif
