// baq_kernels.hip -- base alignment quality and the cap's CIGAR walk on the device (baq_kernels.h).
//
//   baq_kernel   one wave per workgroup, 16 lanes per record, four records per wave.  The HMM is baq_core.h's, the same
//                statements the host's sequential driver runs: M and I of a row a cell per lane, the deletion chain, the
//                row sum and the MAP by the group's lane 0 in the reference's order.  The forward matrix, the two backward
//                rows and the scaling factors of a record sit in its group's quarter of the workgroup's LDS (LDS tier) or
//                in the group's slab of global memory (global tier); the host sorts the records into the tiers, so no
//                wave holds both.  The four groups of a wave walk max(l_query) rows together, so that every barrier is
//                reached by all 64 lanes.
// One writer per output byte, no atomics.  A record whose bytes would pass the batch, or whose workspace would pass its
// slot, is skipped (the host has checked both).
#include <hip/hip_runtime.h>

#include "baq_core.h"
#include "baq_kernels.h"

namespace vb2 {
namespace {

struct WaveSync {
    __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(kBaqLanes* kBaqGroups) void baq_kernel(BaqBatch b, const uint32_t* __restrict__ list, int64_t n,
                                                                     uint8_t* __restrict__ slab, uint64_t stride)
{
    extern __shared__ double baq_lds[];
    const int lane = threadIdx.x & (kBaqLanes - 1), g = threadIdx.x / kBaqLanes;
    uint8_t* const base = slab ? slab + ((uint64_t)blockIdx.x * kBaqGroups + (uint64_t)g) * stride
                               : reinterpret_cast<uint8_t*>(baq_lds) + (uint64_t)g * stride;
    const WaveSync sync;
    for (int64_t first = (int64_t)blockIdx.x * kBaqGroups; first < n; first += (int64_t)gridDim.x * kBaqGroups) {
        const int64_t li = first + g;
        bool have = li < n;
        const uint32_t r = have ? list[li] : 0u;
        bamio::RecordDesc d{};
        baq::Task t{};
        if (have) {
            d = b.desc[r];
            t = b.tasks[r];
            const uint64_t l_seq = d.l_seq < 0 ? 0 : (uint64_t)d.l_seq;
            const uint64_t need = (uint64_t)d.l_read_name + 4ull * d.n_cigar + (l_seq + 1) / 2 + l_seq;
            have = d.l_seq >= 0 && (uint64_t)d.data <= b.data_bytes && need <= b.data_bytes - d.data;
            if (have && t.kind == 2 && baq::work_bytes(t.l_ref, d.l_seq, t.bw) > stride) have = false;
            if (have && t.kind == 2) {
                const int64_t at = (int64_t)t.span_off + ((int64_t)t.xb - (int64_t)t.span_beg);
                if (t.l_ref < 0 || at < 0 || (uint64_t)at + (uint64_t)t.l_ref > b.span_bytes) have = false;
            }
            if (have && t.kind == 1 && (t.bq_off > b.extra_bytes || l_seq > b.extra_bytes - t.bq_off)) have = false;
        }
        const bool hmm = have && t.kind == 2;
        const int mine = hmm ? d.l_seq : 0;
        int rows = 0;
        for (int k = 0; k < kBaqGroups; ++k) {
            const int other = __shfl(mine, k * kBaqLanes);
            rows = other > rows ? other : rows;
        }
        const uint8_t* cig = b.data + d.data + d.l_read_name;
        const uint8_t* seq = cig + 4ull * d.n_cigar;
        const uint8_t* qual = seq + ((uint64_t)(have ? d.l_seq : 0) + 1) / 2;
        uint8_t* out = b.adjq + (qual - b.data);
        if (have) {
            baq::copy_quals(qual, d.l_seq, b.illumina, out, lane, kBaqLanes);
            if (t.kind == 1) baq::apply_bq_tag(b.extra + t.bq_off, d.l_seq, out, lane, kBaqLanes);      // (a lane's own bytes)
        }
        const baq::Work w = baq::carve(base, hmm ? t.l_ref : 0, hmm ? d.l_seq : 0, hmm ? t.bw : 0);
        const baq::Ref ref{b.spans + t.span_off + (int64_t)(t.xb - t.span_beg), 1};
        const baq::Query qy{nullptr, seq, qual, b.illumina};
        const int und = baq::glocal(ref, hmm ? t.l_ref : 0, qy, hmm ? d.l_seq : 0, t.bw, b.tables, w, lane, kBaqLanes, rows, sync);
        if (have && lane == 0) {
            if (hmm) baq::extend_apply(d.pos, d.l_seq, cig, d.n_cigar, t.xb, w, out);
            int32_t c4[4] = {0, 0, 0, 0};
            if (t.cap) baq::cap_walk(d.pos, cig, d.n_cigar, seq, out, d.l_seq, b.spans + t.span_off, t.span_beg, t.ref_len, c4);
            b.cap4[4ull * r + 0] = c4[0];
            b.cap4[4ull * r + 1] = c4[1];
            b.cap4[4ull * r + 2] = c4[2];
            b.cap4[4ull * r + 3] = c4[3];
            b.undefined[r] = und;
        }
        __syncthreads();      // the workspace changes hands
    }
}

}  // namespace

hipError_t launch_baq(const BaqBatch& b, const uint32_t* list, int64_t n, uint8_t* slab, uint64_t stride, uint32_t lds_bytes,
                      int grid, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (grid < 1) grid = 1;
    const uint32_t lds = slab ? 0u : lds_bytes;
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(baq_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(baq_kernel, dim3((unsigned)grid), dim3(kBaqLanes * kBaqGroups), lds, s, b, list, n, slab, stride);
    return hipGetLastError();
}

}  // namespace vb2
