// related_kernels.hip -- gfx950 kernels behind --FindRelated: which samples of a cohort are the
// same individual, or first- or second-degree relatives?
//
// A sample's row holds, per marker and as float32 (source_marginal_kernel's related instantiation, at the fitted point),
//     q[g]  the posterior of its own genotype,
//     h[g]  = q[g] / GF2[g], its own-genotype likelihood relative to a random individual,
//     t[g'] = sum_g q[g] T_p[g][g'], the genotype distribution of a relative sharing one allele identical by descent.
// For target i and partner j, over the markers both count,
//     d2 = q_i . h_j      d1 = t_i . h_j      K_r(i, j) = sum_m log max(k0_r + k1_r d1 + k2_r d2, 1e-30)
// with (k0, k1, k2) = DUP (0, 0, 1), PO (0, 1, 0), FS (1/4, 1/2, 1/4), D2 (1/2, 1/2, 0).
//
//   * related_pair_kernel: source_pair_kernel's discipline.  A workgroup takes 16 targets x 16 partners x one stripe of
//     kPairStripe markers; the rows go through LDS 64 markers at a time as 16-byte records -- (q0 q1 q2 t0) and (t1 t2 counted
//     counted) per target, (h0 h1 h2 counted) per partner --, so a thread's marker costs three ds_read_b128 (with a word
//     of the second record unused the compiler reads 12 bytes, at twice the LDS cycles of 16: the target's flag fills it,
//     and the pair count reads that copy).  "Counted" is staged as 1.0f / 0.0f: a pair's flag is one multiply.  One thread
//     per pair forms the two dots and the four mixtures in FP32 (FMAs), floors them, takes log2 (one v_log_f32 each: the
//     floored value is a normal float) and keeps four FP64 sums, marker after marker.
//   * related_reduce_kernel adds a pair's stripes in stripe order and multiplies each sum by ln 2, once.
// No atomics: a pair's four values are the same bits from call to call and whatever else the set holds.
#include "related_kernels.h"

#include <hip/hip_runtime.h>

namespace vb2 {
namespace {

constexpr int kThreads = 256;
static_assert(kPairTile * kPairTile == kThreads && kPairTile * kPairChunk % kThreads == 0, "one thread per pair of the tile");
// Records of one marker, padded to 17 samples: a staging wave writes one sample's 64 markers, 17 records (68 dwords) apart,
// so the eight lanes of a ds_write_b128 group fall into eight different 4-bank slots (stride 16: all into one).  The wave's
// reads are 16 consecutive records (partners) and 4 records broadcast (targets): conflict-free with or without the pad.
constexpr int kPad = kPairTile + 1;
constexpr double kLn2 = 0.693147180559945309417232121458;

__global__ void __launch_bounds__(kThreads)
related_pair_kernel(const float* const* __restrict__ rows, const size_t q_offset, const int n, const long long num_marker,
                    double* __restrict__ part_k, int32_t* __restrict__ part_n)
{
    __shared__ float4 sa[kPairChunk * kPad];       // target: q0 q1 q2 t0
    __shared__ float4 sb[kPairChunk * kPad];       // target: t1 t2 counted counted
    __shared__ float4 sh[kPairChunk * kPad];       // partner: h0 h1 h2 counted
    const int tid = threadIdx.x;
    const int tj = tid & (kPairTile - 1), ti = tid >> 4;
    const int i0 = blockIdx.y * kPairTile, j0 = blockIdx.x * kPairTile;
    const long long m_begin = (long long)blockIdx.z * kPairStripe;
    const long long m_end = m_begin + kPairStripe < num_marker ? m_begin + kPairStripe : num_marker;
    const size_t plane = (size_t)num_marker * 3;
    double acc[kNumRelation] = {0.0, 0.0, 0.0, 0.0};
    float cnt = 0.0f;                              // (at most kPairStripe: exact)
    for (long long mc = m_begin; mc < m_end; mc += kPairChunk) {
        const int nm = (int)(m_end - mc < kPairChunk ? m_end - mc : kPairChunk);
        __syncthreads();
        for (int e = tid; e < kPairTile * kPairChunk; e += kThreads) {
            const int s = e / kPairChunk, mm = e - s * kPairChunk;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, h = a;
            if (mm < nm) {
                const float* ri = i0 + s < n ? rows[i0 + s] : nullptr;
                const float* rj = j0 + s < n ? rows[j0 + s] : nullptr;
                const size_t at = q_offset + (size_t)(mc + mm) * 3;
                if (ri) {
                    const float* q = ri + at;
                    const float* t = ri + at + 2 * plane;
                    a = make_float4(q[0], q[1], q[2], t[0]);
                    // a counted marker has a non-zero q (sum q = 1) and a non-zero h (sum GF2 h = 1); both are non-negative
                    const float counted = q[0] + q[1] + q[2] > 0.0f ? 1.0f : 0.0f;
                    b = make_float4(t[1], t[2], counted, counted);
                }
                if (rj) {
                    const float* hp = rj + at + plane;
                    h = make_float4(hp[0], hp[1], hp[2], hp[0] + hp[1] + hp[2] > 0.0f ? 1.0f : 0.0f);
                }
            }
            sa[mm * kPad + s] = a;
            sb[mm * kPad + s] = b;
            sh[mm * kPad + s] = h;
        }
        __syncthreads();
        for (int mm = 0; mm < nm; ++mm) {
            const float4 a = sa[mm * kPad + ti], b = sb[mm * kPad + ti], h = sh[mm * kPad + tj];
            const float d2 = fmaf(a.z, h.z, fmaf(a.y, h.y, a.x * h.x));
            const float d1 = fmaf(b.y, h.z, fmaf(b.x, h.y, a.w * h.x));
            float v[kNumRelation];
            v[VB2_REL_DUP] = d2;
            v[VB2_REL_PO] = d1;
            v[VB2_REL_FS] = fmaf(0.25f, d2, fmaf(0.5f, d1, 0.25f));
            v[VB2_REL_D2] = fmaf(0.5f, d1, 0.5f);
            const float both = b.z * h.w;
#pragma unroll
            for (int r = 0; r < kNumRelation; ++r) {
                const float x = v[r] > kRelatedFloor ? v[r] : kRelatedFloor;
                acc[r] += (double)(both * __builtin_amdgcn_logf(x));       // log2 of a normal float
            }
            cnt += b.w * h.w;
        }
    }
    const int i = i0 + ti, j = j0 + tj;
    if (i < n && j < n) {
        const size_t at = ((size_t)blockIdx.z * (size_t)n + (size_t)i) * (size_t)n + (size_t)j;
#pragma unroll
        for (int r = 0; r < kNumRelation; ++r) part_k[at * kNumRelation + r] = acc[r];
        part_n[at] = (int32_t)cnt;
    }
}

__global__ void __launch_bounds__(kThreads)
related_reduce_kernel(const float* const* __restrict__ rows, const int n, const int num_stripe, const double* __restrict__ part_k,
                      const int32_t* __restrict__ part_n, double* __restrict__ llr, int32_t* __restrict__ shared)
{
    const size_t nn = (size_t)n * (size_t)n;
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= nn) return;
    const int i = (int)(at / (size_t)n), j = (int)(at - (size_t)i * (size_t)n);
    double s[kNumRelation] = {0.0, 0.0, 0.0, 0.0};
    int c = 0;
    for (int z = 0; z < num_stripe; ++z) {        // stripe order: fixed
#pragma unroll
        for (int r = 0; r < kNumRelation; ++r) s[r] += part_k[((size_t)z * nn + at) * kNumRelation + r];
        c += part_n[(size_t)z * nn + at];
    }
    const bool none = i == j || rows[i] == nullptr || rows[j] == nullptr;
#pragma unroll
    for (int r = 0; r < kNumRelation; ++r) llr[at * kNumRelation + r] = none ? __builtin_nan("") : s[r] * kLn2;
    shared[at] = none ? 0 : c;
}

}  // namespace

hipError_t launch_related_pairs(const float* const* d_rows, size_t q_offset, int n, int64_t num_marker, double* part_k,
                                int32_t* part_n, double* llr, int32_t* shared, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int nt = (n + kPairTile - 1) / kPairTile;
    const int ns = source_num_stripe(num_marker);
    if (ns > 65535 || nt > 65535) return hipErrorInvalidValue;
    if (ns > 0) {
        const dim3 grid((unsigned)nt, (unsigned)nt, (unsigned)ns), block(kThreads);
        hipLaunchKernelGGL(related_pair_kernel, grid, block, 0, stream, d_rows, q_offset, n, (long long)num_marker, part_k, part_n);
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    const size_t nn = (size_t)n * (size_t)n;
    const dim3 rgrid((unsigned)((nn + kThreads - 1) / kThreads)), block(kThreads);
    hipLaunchKernelGGL(related_reduce_kernel, rgrid, block, 0, stream, d_rows, n, ns, part_k, part_n, llr, shared);
    return hipGetLastError();
}

}  // namespace vb2
