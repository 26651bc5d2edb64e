// bam_pileup_kernels.hip -- per-marker pileup of decoded BAM records (bam_pileup_kernels.h).
//
//   bam_cover_kernel    one thread per record: read filter, first marker at or behind the record's start, ONE walk of the
//                       CIGAR, an entry per covered marker.  Two passes (count, scan, fill), so that the entries are in
//                       file order without atomics.
//   (radix sort)        entries by slot << 32 | file order: stable by slot, whatever the sort does with equal keys.
//   bam_overlap_kernel  one thread per entry: the mate-overlap rule, a chain per read name led by the name's first
//                       eligible entry of the site, so that every quality has exactly one writer.
//   bam_site_kernel     one wave per site: depth cap, min-BQ, characters, the deletion quirk; in-order compaction with
//                       ballots, so a site of any depth comes out in file order.  Two passes (depth, scan, characters).
// Per read group, behind the above and only when asked for:
//   bam_group_key_kernel one thread per sorted entry: a second key (group * num_slot + slot) << 32 | file order for the
//                       entries under the cap that have a group, all ones for the rest.
//   (radix sort)        again, and bam_group_gather_kernel: the entries and their qualities after the overlap rule.
//   bam_site_kernel     its GROUPS form over the virtual slots group * num_slot + slot: no cap, REF of slot % num_slot.
//
// Records are not aligned in the stream: every multi-byte field is put together from bytes.  The host stage has checked
// that a record's name, CIGAR, bases and qualities lie inside its bytes (bam_io.cpp); the cover kernel checks the same
// against the batch's size once more and drops a record that fails.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "bam_pileup_kernels.h"

namespace vb2 {
namespace {

constexpr int kBlock = 256;

__device__ inline uint32_t rd32(const uint8_t* p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ inline uint64_t fnv1a(const uint8_t* p, int n)
{
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

template <bool FILL, bool ADJ>
__global__ __launch_bounds__(kBlock) void bam_cover_kernel(const bamio::RecordDesc* __restrict__ desc, int64_t num_rec,
                                                            const uint8_t* __restrict__ data, uint64_t data_bytes, PileFilter f,
                                                            PileMarkers m, uint32_t* __restrict__ count,
                                                            const uint32_t* __restrict__ offset, PileEntry* __restrict__ entries,
                                                            uint64_t* __restrict__ keys, const uint16_t* __restrict__ group,
                                                            const uint8_t* __restrict__ adj_qual, const int16_t* __restrict__ adj_mapq)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= num_rec) return;
    bamio::RecordDesc d = desc[r];
    uint32_t n = 0;
    // --ApplyBAQ: the mapQ after the cap, below zero for a read the stage dropped; the qualities
    // after BAQ lie in adj_qual where `data` has the record's own
    bool dropped = false;
    if (ADJ) {
        const int mq = adj_mapq[r];
        dropped = mq < 0;
        d.mapq = (uint8_t)(dropped ? 0 : mq);
    }
    // mplp_func's order: unmapped, the exclusion flags, mapQ, orphans
    bool pass = !(d.flag & 4) && d.tid >= 0 && d.tid < m.n_ref && !dropped;
    pass = pass && !(d.flag & f.excl_flags);
    pass = pass && (int32_t)d.mapq >= f.min_mq;
    pass = pass && !(f.no_orphans && (d.flag & 1) && !(d.flag & 2));
    const uint64_t l_seq = d.l_seq < 0 ? 0 : (uint64_t)d.l_seq;
    const uint64_t need = (uint64_t)d.l_read_name + 4ull * d.n_cigar + (l_seq + 1) / 2 + l_seq;
    pass = pass && d.l_seq >= 0 && d.pos >= 0 && (uint64_t)d.data <= data_bytes && need <= data_bytes - d.data;
    if (pass) {
        int32_t lo = m.tid_lo[d.tid];
        const int32_t hi = m.tid_lo[d.tid + 1];
        {   // first marker whose 1-based position is > pos (0-based), i.e. at or behind the record's first base
            int32_t a = lo, b = hi;
            while (a < b) {
                const int32_t mid = a + ((b - a) >> 1);
                if (m.pos[mid] <= d.pos) a = mid + 1;
                else b = mid;
            }
            lo = a;
        }
        const uint8_t* name = data + d.data;
        const uint8_t* cig = name + d.l_read_name;
        const uint8_t* seq = cig + 4ull * d.n_cigar;
        const uint8_t* qual = seq + (l_seq + 1) / 2;
        if (ADJ) qual = adj_qual + (qual - data);
        uint64_t hash = 0;
        bool hashed = false;
        uint32_t out = 0;
        uint16_t grp = 0;
        if (FILL) {
            out = offset[r];
            if (group) grp = group[r];
        }
        int64_t x = d.pos, y = 0;           // reference and query offsets at the start of the operation
        int32_t mi = lo;
        for (uint32_t k = 0; k < d.n_cigar && mi < hi; ++k) {
            const uint32_t c = rd32(cig + 4ull * k);
            const uint32_t op = c & 15;
            const int64_t len = c >> 4;
            const bool match = op == 0 || op == 7 || op == 8;
            const bool skip = op == 2 || op == 3;
            if (match || skip) {
                while (mi < hi && (int64_t)m.pos[mi] - 1 < x + len) {
                    if (FILL) {
                        const int64_t t = (int64_t)m.pos[mi] - 1;
                        const int64_t qpos = match ? y + (t - x) : y;
                        const bool have = qpos < (int64_t)l_seq;
                        PileEntry e;
                        if (!hashed) {
                            hash = fnv1a(name, d.l_read_name);
                            hashed = true;
                        }
                        e.name = (uint64_t)(uintptr_t)name;
                        e.hash = hash;
                        e.order = d.order;
                        e.slot = m.slot[mi];
                        e.qual = have ? qual[qpos] : (uint8_t)0;
                        uint8_t bits = 15;
                        if (match && have) bits = (uint8_t)((seq[qpos >> 1] >> ((qpos & 1) ? 0 : 4)) & 15);
                        if (d.flag & 16) bits |= kEntryReverse;
                        if (skip) bits |= kEntryDeleted;
                        if (!skip && (d.flag & 1) && (d.flag & 2) && !(d.flag & 8) && d.mate_same) bits |= kEntryEligible;
                        if (d.mpos >= d.pos) bits |= kEntryMateAhead;
                        e.bits = bits;
                        e.l_name = d.l_read_name;
                        e.pad0 = 0;
                        e.group = grp;
                        e.pad[0] = e.pad[1] = 0;
                        entries[out + n] = e;
                        keys[out + n] = ((uint64_t)(uint32_t)e.slot << 32) | d.order;
                    }
                    ++n;
                    ++mi;
                }
                x += len;
                if (match) y += len;
            } else if (op == 1 || op == 4) {
                y += len;
            }                                // H, P (and the codes the specification leaves unused) consume nothing
        }
    }
    if (!FILL) count[r] = n;
}

// One workgroup walks the array, 1024 elements a round, and carries the sum.
__global__ __launch_bounds__(1024) void bam_scan_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n,
                                                         unsigned long long* __restrict__ total)
{
    __shared__ uint32_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const uint32_t v = i < n ? in[i] : 0u;
        uint32_t x = v;
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const uint32_t up = __shfl_up(x, dlt);
            if (lane >= dlt) x += up;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < 16; ++k) {
            const uint32_t s = wsum[k];
            if (k < w) before += s;
            all += s;
        }
        if (i < n) out[i] = (uint32_t)(carry + before + (x - v));
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(kBlock) void bam_iota_kernel(uint32_t* __restrict__ idx, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void bam_gather_kernel(const PileEntry* __restrict__ entries, const uint32_t* __restrict__ perm,
                                                             PileEntry* __restrict__ sorted, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) sorted[i] = entries[perm[i]];
}

// range[s] = first sorted entry whose slot is >= s, for s in [0, num_slot]
__global__ __launch_bounds__(kBlock) void bam_range_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t num_slot,
                                                            uint32_t* __restrict__ range)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s > num_slot) return;
    const uint64_t want = (uint64_t)s << 32;
    int64_t a = 0, b = n;
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (keys[mid] < want) a = mid + 1;
        else b = mid;
    }
    range[s] = (uint32_t)a;
}

__device__ inline bool same_read(const PileEntry& a, uint64_t hash, uint8_t l_name, const uint8_t* name)
{
    if (a.hash != hash || a.l_name != l_name) return false;
    const uint8_t* p = (const uint8_t*)(uintptr_t)a.name;
    for (int i = 0; i < l_name; ++i)
        if (p[i] != name[i]) return false;
    return true;
}

// The mate-overlap rule.  Within a site the entries of one read name form a chain in file order, and the rule touches a
// chain at a time: an eligible entry either meets the chain's pending entry -- both get their new qualities, nothing is
// pending any more -- or becomes pending itself when its mate lies ahead.  The thread of a chain's first entry walks it
// and writes every quality of the chain; threads of later entries of a chain write nothing; an entry that is not
// eligible keeps its quality.  So every qual_out has one writer.
__global__ __launch_bounds__(kBlock) void bam_overlap_kernel(const PileEntry* __restrict__ sorted, const uint32_t* __restrict__ range,
                                                              int64_t n, int32_t max_depth, int32_t smart,
                                                              uint8_t* __restrict__ qual_out, PileCounters* __restrict__ ctr)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const PileEntry e = sorted[i];
    const int64_t lo = range[e.slot], hi = range[e.slot + 1];
    const int64_t cap = hi - lo > (int64_t)max_depth ? lo + max_depth : hi;
    if (!smart || i >= cap || !(e.bits & kEntryEligible)) {
        qual_out[i] = e.qual;
        return;
    }
    const uint8_t* name = (const uint8_t*)(uintptr_t)e.name;
    for (int64_t j = lo; j < i; ++j) {
        if (sorted[j].hash != e.hash) continue;
        const PileEntry a = sorted[j];
        if ((a.bits & kEntryEligible) && same_read(a, e.hash, e.l_name, name)) return;      // not the chain's first
    }
    int64_t pending = -1;
    uint8_t pq = 0, pbits = 0;
    unsigned long long pairs = 0;
    for (int64_t j = i; j < cap; ++j) {
        PileEntry a = e;
        if (j != i) {
            if (sorted[j].hash != e.hash) continue;
            a = sorted[j];
            if (!(a.bits & kEntryEligible) || !same_read(a, e.hash, e.l_name, name)) continue;
        }
        if (pending >= 0) {
            int qa = pq, qb = a.qual;
            if ((pbits & 15) == (a.bits & 15)) {
                qa = qa + qb < 200 ? qa + qb : 200;
                qb = 0;
            } else if (qa >= qb) {
                qa = (int)(0.8 * (double)qa);
                qb = 0;
            } else {
                qb = (int)(0.8 * (double)qb);
                qa = 0;
            }
            qual_out[pending] = (uint8_t)qa;
            qual_out[j] = (uint8_t)qb;
            pending = -1;
            ++pairs;
        } else if (a.bits & kEntryMateAhead) {
            pending = j;
            pq = a.qual;
            pbits = a.bits;
        } else {
            qual_out[j] = a.qual;
        }
    }
    if (pending >= 0) qual_out[pending] = pq;
    if (pairs) atomicAdd(&ctr->pairs_resolved, pairs);
}

// One wave per site.  Lane l of round k looks at the site's entry 64 k + l; the ballots of "contributes a base" and
// "contributes a quality" give every lane its place behind what the lanes before it and the rounds before this one wrote.
// GROUPS: the slots are virtual (group * ref_slots + slot): the cap was applied to the whole site before, the REF nibble is
// that of slot % ref_slots, and nothing is counted.
template <bool FILL, bool GROUPS>
__global__ __launch_bounds__(kBlock) void bam_site_kernel(const PileEntry* __restrict__ sorted, const uint32_t* __restrict__ range,
                                                           const uint8_t* __restrict__ qual, int32_t num_slot, int32_t max_depth,
                                                           int32_t ref_slots, int32_t min_bq, const uint8_t* __restrict__ ref_nib,
                                                           uint32_t* __restrict__ depth, uint8_t* __restrict__ reported,
                                                           const uint32_t* __restrict__ offset, char* __restrict__ base_pool,
                                                           char* __restrict__ qual_pool, PileCounters* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (slot >= num_slot) return;                  // (whole waves leave: the ballots below see full rounds)
    const int64_t lo = range[slot], hi = range[slot + 1];
    const int64_t cap = !GROUPS && hi - lo > (int64_t)max_depth ? lo + max_depth : hi;
    const uint32_t nb_total = FILL ? depth[slot] : 0u;
    const uint64_t off = FILL ? offset[slot] : 0u;
    const uint8_t rn = FILL ? ref_nib[GROUPS ? (int64_t)((int32_t)slot % ref_slots) : slot] : (uint8_t)0;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t nb = 0, nq = 0;
    for (int64_t base = lo; base < cap; base += 64) {
        const int64_t j = base + lane;
        const bool valid = j < cap;
        uint8_t q = 0, bits = 0;
        if (valid) {
            q = qual[j];
            bits = sorted[j].bits;
        }
        const bool keep_q = valid && (int32_t)q >= min_bq;
        const bool keep_b = keep_q && !(bits & kEntryDeleted);
        const unsigned long long bq = __ballot(keep_q), bb = __ballot(keep_b);
        if (FILL) {
            if (keep_b) {
                const uint32_t nib = bits & 15;
                const bool rev = (bits & kEntryReverse) != 0;
                char c;
                if (nib == 0 || nib == rn) c = rev ? ',' : '.';
                else {
                    c = "=ACMGRSVTWYHKDBN"[nib];
                    if (rev) c = (char)(c | 0x20);
                }
                base_pool[off + nb + __popcll(bb & below)] = c;
            }
            if (keep_q) {
                // the deletion quirk: a deleted read's quality stays in the list, and the site stores the first
                // `bases` of them (header of bam_flatten.cpp)
                const uint32_t qi = nq + __popcll(bq & below);
                if (qi < nb_total) qual_pool[off + qi] = (char)(q + 33 < 126 ? q + 33 : 126);
            }
        }
        nb += __popcll(bb);
        nq += __popcll(bq);
    }
    if (!FILL && lane == 0) {
        depth[slot] = nb;
        reported[slot] = hi > lo ? 1 : 0;
        if (!GROUPS && hi - lo > (int64_t)max_depth) atomicAdd(&ctr->capped_sites, 1ull);
    }
}

__global__ __launch_bounds__(kBlock) void bam_group_key_kernel(const PileEntry* __restrict__ sorted, const uint32_t* __restrict__ range,
                                                                int64_t n, int32_t num_slot, int32_t num_group, int32_t max_depth,
                                                                uint64_t* __restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const PileEntry e = sorted[i];
    uint64_t key = ~0ull;
    if (e.slot >= 0 && e.slot < num_slot && (int32_t)e.group < num_group) {
        const int64_t lo = range[e.slot], hi = range[e.slot + 1];
        const int64_t cap = hi - lo > (int64_t)max_depth ? lo + max_depth : hi;
        if (i < cap) key = ((uint64_t)((uint32_t)e.group * (uint32_t)num_slot + (uint32_t)e.slot) << 32) | e.order;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(kBlock) void bam_group_gather_kernel(const PileEntry* __restrict__ sorted, const uint8_t* __restrict__ qual,
                                                                   const uint32_t* __restrict__ perm, PileEntry* __restrict__ sorted2,
                                                                   uint8_t* __restrict__ qual2, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = perm[i];
    sorted2[i] = sorted[j];
    qual2[i] = qual[j];
}

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_cover_count(const bamio::RecordDesc* desc, int64_t num_rec, const uint8_t* data, uint64_t data_bytes,
                              PileFilter f, PileMarkers m, uint32_t* count, hipStream_t s, const uint8_t* adj_qual,
                              const int16_t* adj_mapq)
{
    if (num_rec <= 0) return hipSuccess;
    if (adj_qual && adj_mapq)
        bam_cover_kernel<false, true><<<blocks_for(num_rec, kBlock), kBlock, 0, s>>>(desc, num_rec, data, data_bytes, f, m, count, nullptr,
                                                                                      nullptr, nullptr, nullptr, adj_qual, adj_mapq);
    else
        bam_cover_kernel<false, false><<<blocks_for(num_rec, kBlock), kBlock, 0, s>>>(desc, num_rec, data, data_bytes, f, m, count, nullptr,
                                                                                       nullptr, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_cover_fill(const bamio::RecordDesc* desc, int64_t num_rec, const uint8_t* data, uint64_t data_bytes,
                             PileFilter f, PileMarkers m, const uint32_t* offset, PileEntry* entries, uint64_t* keys,
                             hipStream_t s, const uint16_t* group, const uint8_t* adj_qual, const int16_t* adj_mapq)
{
    if (num_rec <= 0) return hipSuccess;
    if (adj_qual && adj_mapq)
        bam_cover_kernel<true, true><<<blocks_for(num_rec, kBlock), kBlock, 0, s>>>(desc, num_rec, data, data_bytes, f, m, nullptr, offset,
                                                                                     entries, keys, group, adj_qual, adj_mapq);
    else
        bam_cover_kernel<true, false><<<blocks_for(num_rec, kBlock), kBlock, 0, s>>>(desc, num_rec, data, data_bytes, f, m, nullptr, offset,
                                                                                      entries, keys, group, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_scan_u32(const uint32_t* count, uint32_t* offset, int64_t n, unsigned long long* total, hipStream_t s)
{
    bam_scan_kernel<<<1, 1024, 0, s>>>(count, offset, n, total);
    return hipGetLastError();
}

hipError_t sort_entries(void* temp, size_t* temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* idx_in,
                        uint32_t* idx_out, int64_t n, hipStream_t s)
{
    return hipcub::DeviceRadixSort::SortPairs(temp, *temp_bytes, keys_in, keys_out, idx_in, idx_out, (int)n, 0, 64, s);
}

hipError_t launch_iota_u32(uint32_t* idx, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    bam_iota_kernel<<<blocks_for(n, kBlock), kBlock, 0, s>>>(idx, n);
    return hipGetLastError();
}

hipError_t launch_gather(const PileEntry* entries, const uint32_t* perm, PileEntry* sorted, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    bam_gather_kernel<<<blocks_for(n, kBlock), kBlock, 0, s>>>(entries, perm, sorted, n);
    return hipGetLastError();
}

hipError_t launch_site_ranges(const uint64_t* keys, int64_t n, int32_t num_slot, uint32_t* range, hipStream_t s)
{
    bam_range_kernel<<<blocks_for((int64_t)num_slot + 1, kBlock), kBlock, 0, s>>>(keys, n, num_slot, range);
    return hipGetLastError();
}

hipError_t launch_overlap(const PileEntry* sorted, const uint32_t* range, int64_t n, int32_t max_depth, int32_t smart,
                          uint8_t* qual_out, PileCounters* ctr, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    bam_overlap_kernel<<<blocks_for(n, kBlock), kBlock, 0, s>>>(sorted, range, n, max_depth, smart, qual_out, ctr);
    return hipGetLastError();
}

hipError_t launch_sites(bool fill, const PileEntry* sorted, const uint32_t* range, const uint8_t* qual, int32_t num_slot,
                        int32_t max_depth, int32_t min_bq, const uint8_t* ref_nib, uint32_t* depth, uint8_t* reported,
                        const uint32_t* offset, char* base_pool, char* qual_pool, PileCounters* ctr, hipStream_t s)
{
    if (num_slot <= 0) return hipSuccess;
    const unsigned grid = blocks_for(num_slot, kBlock / 64);
    if (fill)
        bam_site_kernel<true, false><<<grid, kBlock, 0, s>>>(sorted, range, qual, num_slot, max_depth, num_slot, min_bq, ref_nib, depth,
                                                              reported, offset, base_pool, qual_pool, ctr);
    else
        bam_site_kernel<false, false><<<grid, kBlock, 0, s>>>(sorted, range, qual, num_slot, max_depth, num_slot, min_bq, ref_nib, depth,
                                                               reported, offset, base_pool, qual_pool, ctr);
    return hipGetLastError();
}

hipError_t launch_group_keys(const PileEntry* sorted, const uint32_t* range, int64_t n, int32_t num_slot, int32_t num_group,
                             int32_t max_depth, uint64_t* keys, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    bam_group_key_kernel<<<blocks_for(n, kBlock), kBlock, 0, s>>>(sorted, range, n, num_slot, num_group, max_depth, keys);
    return hipGetLastError();
}

hipError_t launch_group_gather(const PileEntry* sorted, const uint8_t* qual, const uint32_t* perm, PileEntry* sorted2,
                               uint8_t* qual2, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    bam_group_gather_kernel<<<blocks_for(n, kBlock), kBlock, 0, s>>>(sorted, qual, perm, sorted2, qual2, n);
    return hipGetLastError();
}

hipError_t launch_group_sites(bool fill, const PileEntry* sorted2, const uint32_t* range, const uint8_t* qual2, int32_t num_vslot,
                              int32_t num_slot, int32_t min_bq, const uint8_t* ref_nib, uint32_t* depth, uint8_t* reported,
                              const uint32_t* offset, char* base_pool, char* qual_pool, hipStream_t s)
{
    if (num_vslot <= 0 || num_slot <= 0) return hipSuccess;
    const unsigned grid = blocks_for(num_vslot, kBlock / 64);
    if (fill)
        bam_site_kernel<true, true><<<grid, kBlock, 0, s>>>(sorted2, range, qual2, num_vslot, 0, num_slot, min_bq, ref_nib, depth,
                                                             reported, offset, base_pool, qual_pool, nullptr);
    else
        bam_site_kernel<false, true><<<grid, kBlock, 0, s>>>(sorted2, range, qual2, num_vslot, 0, num_slot, min_bq, ref_nib, depth,
                                                              reported, offset, base_pool, qual_pool, nullptr);
    return hipGetLastError();
}

}  // namespace vb2
