// conditioned_kernels.hip -- gfx950 kernels for the log-likelihood given a hypothesised contaminant,
//     LLK(theta | h) = sum_m log sum_g1 P_h[m][g1] sum_g2 GF2[g2] W[g1][g2],
// P_h[m] the hypothesis's genotype triple of the marker (float32; the genotype posterior of another sample of the cohort)
// where it is not all zero and the Hardy-Weinberg prior GF1(pc1) where it is.  DESIGN.md section 13.  Like deriv_kernels.hip
// and weighted_kernels.hip this file walks the layouts the context already holds (llk_kernels.h: DeviceLayout), in both
// forms, with a body of its own, and makes no second copy of the reads: every hypothesis reads the one resident sample.
//
//   * prior_permute_kernel: the hypotheses' rows (panel order, [M][3]) into the context's sorted order as three planes per
//     hypothesis, [3][m_pad] -- structure of arrays, so that the marker kernel's thread of sorted position tg * 256 + tid
//     reads three coalesced floats.
//   * llk_conditioned_marker_kernel<PD, K>: one workgroup per (stripe of 16-tile groups, point).  It builds the point's table
//     in LDS -- per table row the six off-diagonal genotype pairs' P^n (probability domain) or log p (run words) -- and one
//     thread per marker walks the marker's steps or runs, forms L = P' W GF2 in the reference's order (h:307-309) and, where
//     L > 0 (h:310), takes log L.  The 256 values of a tile group are summed by a fixed tree into partial[point][group].
//     K = 2, 4: the projection loops unrolled for that --NumPC (the evaluation kernels' KSEL); K = 0: any --NumPC.
//   * llk_conditioned_reduce_kernel: one workgroup per point sums the point's partial sums -- thread t takes groups t,
//     t + 256, ..., then the same tree.  Which workgroup walked a group does not enter: a point's result is the same bits
//     whatever else the launch holds, however many workgroups share the point, and from one call to the next.
#include "conditioned_kernels.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vb2 {
namespace {

constexpr int kThreads = 256;                     // 16 micro-tiles of 16 markers per tile group
constexpr int kRowDoubles = 6;                    // the six off-diagonal genotype pairs (the diagonal: the context's constants)
constexpr double kMinAf = 0.00005, kMaxAf = 0.99995;   // h:94-95

// off-diagonal genotype pairs, in the reference's (g1 outer, g2 inner) order (as llk_kernels.hip numbers them)
__device__ __forceinline__ void pair_g(int p, int& g1, int& g2)
{
    g1 = p >> 1;
    const int lo = p & 1;
    g2 = lo + (lo >= g1 ? 1 : 0);
}

// h:223-224 for one class / quality / pair: p = alpha u_g1 + (1 - alpha) u_g2 in the reference's expression order; a negative
// p (alpha outside [0, 1]) is NaN, and the marker is left out.  The class is ref; alt reads the pair mirrored (h:164-177).
__device__ __forceinline__ double entry_of(double alpha, double p_err, int g1, int g2)
{
    const double p_ok = 1.0 - p_err;
    const double e1 = (double)g1 * (1.0 / 6.0), e2 = (double)g2 * (1.0 / 6.0);
    const double n1 = 1.0 - 0.5 * (double)g1, n2 = 1.0 - 0.5 * (double)g2;
    const double one_minus_alpha = 1.0 - alpha;
    const double p = (alpha * e1 + one_minus_alpha * e2) * p_err + (alpha * n1 + one_minus_alpha * n2) * p_ok;
    return p >= 0.0 ? p : __builtin_nan("");
}

// GF (h:186-192)
__device__ __forceinline__ void gf_of(double af, double* gf)
{
    if (af < kMinAf) af = kMinAf;
    if (af > kMaxAf) af = kMaxAf;
    gf[0] = (1 - af) * (1 - af);
    gf[1] = 2 * (af) * (1 - af);
    gf[2] = af * af;
}

// fixed tree over the workgroup's 256 values; the sum is in part[0] after the call (all threads must arrive)
__device__ __forceinline__ void tree_sum(double* part, int tid)
{
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
}

template <bool PD, int K>
__global__ void __launch_bounds__(kThreads)
llk_conditioned_marker_kernel(const DeviceLayout L, const double* __restrict__ points, const int32_t* __restrict__ hyp_of,
                              const float* __restrict__ planes, double* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];      // [nrow][6 pairs], then the tree's [256]
    const int tid = threadIdx.x;
    const int pt = (int)blockIdx.y, bx = (int)blockIdx.x, nbx = (int)gridDim.x;
    const int k = K ? K : L.num_pc, stride = 2 * k + 1;
    const double* prow = points + (size_t)pt * stride;
    const double alpha = prow[2 * k];
    const int nrow = L.num_code + 1;
    const size_t mp = (size_t)L.m_pad;
    const float* hrow = planes + (size_t)hyp_of[pt] * 3 * mp;
    double* part = tab + (size_t)nrow * kRowDoubles;

    // ---- the point's table ----
    const int num_single = PD ? L.num_prim - L.num_pair : L.num_prim;
    for (int e = tid; e < num_single * 6; e += kThreads) {
        const int pi = e / 6, p = e - pi * 6;
        const double2 rec = L.prim[pi];
        const uint32_t pr = (uint32_t)__double_as_longlong(rec.y);
        const int first = (int)(pr & 0xffffu), twin = (int)(pr >> 16);
        int g1, g2;
        pair_g(p, g1, g2);
        if constexpr (PD) {
            // record = a quality, class ref: {pErr, first row | K << 16 | rows from P^n to P^(n+1), a signed byte, << 24}
            const double v = entry_of(alpha, rec.x, g1, g2);
            const int kq = twin & 0xff, rstep = (int)(int8_t)(twin >> 8);
            double r = v;
            for (int n = 1; n <= kq; ++n) {
                const int row = first + (n - 1) * rstep;
                if (row >= 0 && row < nrow) tab[(size_t)row * kRowDoubles + p] = r;
                r *= v;
            }
        } else {
            // record = a code: {signed pErr (alt < 0), code | twin << 16}; the alt twin's row is this one mirrored (pair 5 - p)
            if (rec.x < 0.0) { g1 = 2 - g1; g2 = 2 - g2; }
            const double lv = log(entry_of(alpha, fabs(rec.x), g1, g2));
            if (first < nrow) tab[(size_t)first * kRowDoubles + p] = lv;
            if (twin != 0xffff && twin < nrow) tab[(size_t)twin * kRowDoubles + (5 - p)] = lv;
        }
    }
    for (int e = tid; e < kRowDoubles; e += kThreads)           // padding row: P = 1 (log domain: 0)
        tab[(size_t)L.num_code * kRowDoubles + e] = PD ? 1.0 : 0.0;
    if constexpr (PD) {
        // window rows: the product of two rows (level 1 uses rows of level 0)
        for (int level = 0; level < 2; ++level) {
            const int nrec = level == 0 ? L.num_pair - L.num_pair2 : L.num_pair2;
            const int base = num_single + (level == 0 ? 0 : L.num_pair - L.num_pair2);
            __syncthreads();
            for (int e = tid; e < nrec * 6; e += kThreads) {
                const int pi = e / 6, p = e - pi * 6;
                const double2 rec = L.prim[base + pi];
                const uint32_t ab = (uint32_t)__double_as_longlong(rec.x), dst = (uint32_t)__double_as_longlong(rec.y);
                const uint32_t ra = ab & 0xffffu, rb = ab >> 16;
                if (ra >= (uint32_t)nrow || rb >= (uint32_t)nrow || dst >= (uint32_t)nrow) continue;
                tab[(size_t)dst * kRowDoubles + p] = tab[(size_t)ra * kRowDoubles + p] * tab[(size_t)rb * kRowDoubles + p];
            }
        }
    }
    __syncthreads();

    // ---- one thread per marker of the sorted order, one partial sum per tile group ----
    const int m = tid & 15;
    const int ntile_grp = (L.num_mt + 15) / 16;
    const bool kaf = L.known_af != nullptr;
    for (int tg = bx; tg < ntile_grp; tg += nbx) {
        const int mt = tg * 16 + (tid >> 4);
        const size_t pos = (size_t)mt * 16 + (size_t)m;
        double val = 0.0;
        if (mt < L.num_mt && pos < (size_t)L.num_active) {      // no weights: every counted marker is walked
            const uint2 rec = L.mt_rec[mt];
            // the hypothesis's triple of this marker: three coalesced floats, in flight under the walk
            const float h0 = hrow[pos], h1 = hrow[mp + pos], h2 = hrow[2 * mp + pos];
            double acc[6];
            for (int p = 0; p < 6; ++p) acc[p] = PD ? 1.0 : L.ediag[pos];       // log domain: c_other, summed here
            if constexpr (PD) {
                // {ref steps | all steps << 16}; a step = a 16-bit byte offset of its row (+ kPdAltOffset for class alt), two per word
                const uint32_t s1 = rec.y & 0xffffu, s2 = rec.y >> 16;
                const uint16_t* c16 = reinterpret_cast<const uint16_t*>(L.codes);
                for (uint32_t s = 0; s < s2; ++s) {
                    const bool alt = s >= s1;
                    uint32_t off = c16[(((size_t)rec.x + (s >> 1)) * 16 + (size_t)m) * 2 + (s & 1u)];
                    if (alt) off -= (uint32_t)kPdAltOffset;
                    uint32_t row = off / (uint32_t)L.row_bytes;
                    row = row < (uint32_t)nrow ? row : (uint32_t)L.num_code;
                    const double* t = tab + (size_t)row * kRowDoubles;
#pragma unroll
                    for (int p = 0; p < 6; ++p) acc[p] *= t[alt ? 5 - p : p];
                }
            } else {
                // {first row, rows}; a row = two run words, run = row byte offset | top 16 bits of double(count) << 16
                for (uint32_t r = 0; r < rec.y; ++r) {
                    const uint2 rw2 = L.codes[((size_t)rec.x + r) * 16 + (size_t)m];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const uint32_t rw = j ? rw2.y : rw2.x;
                        const double n = __hiloint2double((int)(rw & 0xffff0000u), 0);
                        uint32_t row = (rw & 0xffffu) / (uint32_t)L.row_bytes;
                        row = row < (uint32_t)nrow ? row : (uint32_t)L.num_code;
                        const double* t = tab + (size_t)row * kRowDoubles;
#pragma unroll
                        for (int p = 0; p < 6; ++p) acc[p] = fma(n, t[p], acc[p]);
                    }
                }
            }
            // ---- epilogue: L = P' W GF2, the diagonal of W the context's constants (L as the evaluation kernels define it) ----
            double af1, af2;
            if (kaf) {
                af1 = af2 = L.known_af[pos];
            } else {
                af1 = 0.0; af2 = 0.0;
#pragma unroll
                for (int kk = 0; kk < k; ++kk) {
                    const double u = L.ud[(size_t)kk * mp + pos];
                    af1 = fma(u, prow[kk], af1);
                    af2 = fma(u, prow[k + kk], af2);
                }
                const double mu = L.mu[pos];
                af1 += mu; af1 /= 2.0;
                af2 += mu; af2 /= 2.0;
            }
            double G1[3], G2[3], W[3][3];
            gf_of(af1, G1);
            gf_of(af2, G2);
            // an all-zero triple carries no information: the anonymous model's term, GF1 at the fixed pc1
            const bool given = h0 != 0.0f || h1 != 0.0f || h2 != 0.0f;
            G1[0] = given ? (double)h0 : G1[0];
            G1[1] = given ? (double)h1 : G1[1];
            G1[2] = given ? (double)h2 : G1[2];
            const double cst = PD ? L.ediag[pos] : 0.0;
            for (int g = 0; g < 3; ++g) W[g][g] = L.ediag[(size_t)(1 + g) * mp + pos];
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                int g1, g2;
                pair_g(p, g1, g2);
                W[g1][g2] = PD ? cst * acc[p] : exp(acc[p]);
            }
            double lk = 0.0;
            for (int g1 = 0; g1 < 3; ++g1)
                for (int g2 = 0; g2 < 3; ++g2) lk += W[g1][g2] * G1[g1] * G2[g2];
            if (lk > 0) val = log(lk);
        }
        part[tid] = val;
        tree_sum(part, tid);
        if (tid == 0) partial[(size_t)pt * ntile_grp + tg] = part[0];
        __syncthreads();                                        // part[] is written again in the next round
    }
}

__global__ void __launch_bounds__(kThreads)
llk_conditioned_reduce_kernel(const double* __restrict__ partial, int ntile_grp, double* __restrict__ out)
{
    __shared__ double part[kThreads];
    const int tid = threadIdx.x, pt = (int)blockIdx.x;
    const double* s = partial + (size_t)pt * ntile_grp;
    double sum = 0.0;
    for (int i = tid; i < ntile_grp; i += kThreads) sum += s[i];
    part[tid] = sum;
    tree_sum(part, tid);
    if (tid == 0) out[pt] = part[0];
}

// one thread per (hypothesis, sorted position)
__global__ void __launch_bounds__(kThreads)
prior_permute_kernel(const float* __restrict__ panel, const int32_t* __restrict__ pidx, float* __restrict__ planes,
                     int num_marker, long long num_active, long long m_pad)
{
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pos >= m_pad) return;
    const size_t h = blockIdx.y;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (pos < num_active) {
        const int32_t i = pidx[pos];
        if (i >= 0 && i < num_marker) {
            const float* src = panel + (h * (size_t)num_marker + (size_t)i) * 3;
            v0 = src[0]; v1 = src[1]; v2 = src[2];
        }
    }
    float* dst = planes + h * 3 * (size_t)m_pad + (size_t)pos;
    dst[0] = v0;
    dst[(size_t)m_pad] = v1;
    dst[2 * (size_t)m_pad] = v2;
}

template <bool PD, int K>
void launch_marker(const DeviceLayout& L, dim3 grid, size_t shmem, hipStream_t stream, const double* d_points,
                   const int32_t* d_hyp, const float* d_planes, double* d_partial)
{
    hipLaunchKernelGGL((llk_conditioned_marker_kernel<PD, K>), grid, dim3(kThreads), shmem, stream, L, d_points, d_hyp, d_planes,
                       d_partial);
}

}  // namespace

hipError_t launch_prior_permute(const DeviceLayout& L, int num_marker, int num_hyp, const float* d_panel, const int32_t* d_pidx,
                                float* d_planes, hipStream_t stream)
{
    if (num_hyp <= 0 || L.m_pad <= 0) return hipSuccess;
    if (num_hyp > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((L.m_pad + kThreads - 1) / kThreads), (unsigned)num_hyp);
    hipLaunchKernelGGL(prior_permute_kernel, grid, dim3(kThreads), 0, stream, d_panel, d_pidx, d_planes, num_marker,
                       (long long)L.num_active, (long long)L.m_pad);
    return hipGetLastError();
}

hipError_t launch_llk_conditioned(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_hyp,
                                  const float* d_planes, double* d_partial, double* d_out, hipStream_t stream)
{
    if (num_point <= 0) return hipSuccess;
    if (num_point > kMaxPointsPerLaunch) return hipErrorInvalidValue;
    const int nrow = L.num_code + 1;
    const size_t shmem = ((size_t)nrow * kRowDoubles + kThreads) * sizeof(double);
    if (shmem > 64 * 1024) return hipErrorInvalidValue;      // (at most 189 rows of 6 doubles and the tree: 11 KiB)
    const int ntile_grp = conditioned_tile_groups(L);
    if (ntile_grp > 0) {
        // about four workgroups per CU over the whole launch; each walks a stripe of tile groups with one table
        int gx = (4 * (L.num_cu > 0 ? L.num_cu : 1) + num_point - 1) / num_point;
        gx = gx < ntile_grp ? gx : ntile_grp;
        gx = gx > 0 ? gx : 1;
        const dim3 grid((unsigned)gx, (unsigned)num_point);
        const int ksel = L.known_af ? 0 : (L.num_pc == 2 || L.num_pc == 4) ? L.num_pc : 0;
        if (L.pd) {
            if (ksel == 2) launch_marker<true, 2>(L, grid, shmem, stream, d_points, d_hyp, d_planes, d_partial);
            else if (ksel == 4) launch_marker<true, 4>(L, grid, shmem, stream, d_points, d_hyp, d_planes, d_partial);
            else launch_marker<true, 0>(L, grid, shmem, stream, d_points, d_hyp, d_planes, d_partial);
        } else {
            if (ksel == 2) launch_marker<false, 2>(L, grid, shmem, stream, d_points, d_hyp, d_planes, d_partial);
            else if (ksel == 4) launch_marker<false, 4>(L, grid, shmem, stream, d_points, d_hyp, d_planes, d_partial);
            else launch_marker<false, 0>(L, grid, shmem, stream, d_points, d_hyp, d_planes, d_partial);
        }
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(llk_conditioned_reduce_kernel, dim3((unsigned)num_point), dim3(kThreads), 0, stream, d_partial, ntile_grp,
                       d_out);
    return hipGetLastError();
}

}  // namespace vb2
