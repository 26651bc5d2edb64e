// panel_kernels.hip -- device half of the --RefVCF panel builder (panel.cpp drives it).
//
// The genotype slab is int8, SAMPLE-major: row j = sample j, column m = marker m (rows padded to 64 with zeros, each
// chunk's columns padded to 128 with zeros), so that the Gram's reduction dimension (markers) is contiguous for both
// MFMA operands and the projection's one-thread-per-marker reads are coalesced (adjacent markers = adjacent bytes).
//
//   transpose_chunk   marker-major block from the reader -> the slab's column block
//   row_sums          s_m = sum_j g_mj (int32, exact)
//   gram_chunk        S += G_chunk^T G_chunk over lower-triangle 64x64 tiles, v_mfma_i32_16x16x64_i8, int32 accumulators:
//                     exact while 4 * M < 2^31 (|g| <= 2; the host asserts M < 5e8)
//   mu_from_sums      mu_m = (float)s_m / (float)N, kept as a double
//   sample_dot_mu     c_j += sum_m mu_m g_mj (FP64, fixed summation order)
//   sum_squares       tau = sum_m mu_m^2 (FP64, fixed order)
//   centre_gram       C = S - c 1^T - 1 c^T + tau 1 1^T (FP64), S mirrored from its lower tiles
//   project           UD = G V - mu (1^T V) (FP64), V tile in LDS, one thread per marker
#include <hip/hip_runtime.h>

#include "panel.h"

namespace vb2 {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kT = kGramTile;          // 64: output tile edge
constexpr int kKB = kGramKStep;        // 128: markers per LDS stage (two MFMA k-steps of 64)
constexpr int kLdsPitch = kKB + 16;    // 144 B rows: ds_read_b128 stays aligned, rows start 4 banks apart

__global__ void __launch_bounds__(256) transpose_chunk_kernel(const int8_t* __restrict__ src, int64_t count, int32_t n,
                                                              int8_t* __restrict__ dst, int64_t ld)
{
    __shared__ int8_t t[64][65];
    const int64_t m0 = (int64_t)blockIdx.x * 64;
    const int32_t j0 = blockIdx.y * 64;
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int r = e >> 6, c = e & 63;            // r: marker, c: sample (reads along the sample run of a marker)
        const int64_t m = m0 + r;
        const int32_t j = j0 + c;
        t[r][c] = (m < count && j < n) ? src[m * n + j] : (int8_t)0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int r = e >> 6, c = e & 63;            // r: sample, c: marker (writes along the marker run of a sample)
        const int32_t j = j0 + r;
        const int64_t m = m0 + c;
        if (j < n && m < count) dst[(int64_t)j * ld + m] = t[c][r];
    }
}

__global__ void __launch_bounds__(256) row_sums_kernel(const int8_t* __restrict__ src, int64_t count, int32_t n,
                                                       int32_t* __restrict__ sums)
{
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= count) return;
    const int8_t* row = src + m * n;
    int s = 0;
    for (int32_t j = lane; j < n; j += 64) s += row[j];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) sums[m] = s;
}

__global__ void __launch_bounds__(256) mu_from_sums_kernel(const int32_t* __restrict__ sums, int64_t count, int32_t n,
                                                           double* __restrict__ mu)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // the binary32 quotient of two integers below 2^24, as Eigen's rowwise().mean() rounds it: the FP64 quotient
    // rounded once more to binary32 is the correctly rounded binary32 quotient (53 >= 2 * 24 + 2)
    if (m < count) mu[m] = (double)(float)((double)sums[m] / (double)n);
}

// (tile row, tile column) of the t-th lower-triangle tile, rows in order: t = r(r+1)/2 + c, c <= r
__device__ inline void tri_tile(int t, int* r, int* c)
{
    int rr = (int)((__builtin_sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while ((rr + 1) * (rr + 2) / 2 <= t) ++rr;
    while (rr * (rr + 1) / 2 > t) --rr;
    *r = rr;
    *c = t - rr * (rr + 1) / 2;
}

// One workgroup = one 64 x 64 tile of S (tile row >= tile column), four waves of 32 x 32 = 2 x 2 MFMA 16x16x64 tiles.
// Fragments (the i8 form of the gfx950 16x16 MFMA map): lane l holds row (l & 15) of A and
// column (l & 15) of B with the 16 k of lane group l >> 4; both operands are rows of the sample-major slab, so they
// are read the same way.  Accumulator: column = l & 15, row = 4 (l >> 4) + register.
__global__ void __launch_bounds__(256) gram_chunk_kernel(const int8_t* __restrict__ slab, int64_t ld, int64_t k_len,
                                                         int32_t* __restrict__ S, int32_t n_pad)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[2 * kT * kLdsPitch];
    int8_t* la = lds;
    int8_t* lb = lds + kT * kLdsPitch;
    int tr, tc;
    tri_tile(blockIdx.x, &tr, &tc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int8_t* ga = slab + (int64_t)tr * kT * ld;
    const int8_t* gb = slab + (int64_t)tc * kT * ld;

    v4i acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = v4i{0, 0, 0, 0};

    // staging: 64 rows x 128 B per operand = 512 pieces of 16 B, two per thread
    v4i ra[2], rb[2];
    auto load = [&](int64_t k0) {
        for (int h = 0; h < 2; ++h) {
            const int p = tid + 256 * h, row = p >> 3, col = (p & 7) * 16;
            ra[h] = *reinterpret_cast<const v4i*>(ga + (int64_t)row * ld + k0 + col);
            rb[h] = *reinterpret_cast<const v4i*>(gb + (int64_t)row * ld + k0 + col);
        }
    };
    const int64_t nk = k_len / kKB;
    if (nk > 0) load(0);
    for (int64_t kb = 0; kb < nk; ++kb) {
        __syncthreads();
        for (int h = 0; h < 2; ++h) {
            const int p = tid + 256 * h, row = p >> 3, col = (p & 7) * 16;
            *reinterpret_cast<v4i*>(la + row * kLdsPitch + col) = ra[h];
            *reinterpret_cast<v4i*>(lb + row * kLdsPitch + col) = rb[h];
        }
        __syncthreads();
        if (kb + 1 < nk) load((kb + 1) * kKB);
        for (int ks = 0; ks < 2; ++ks) {
            const int koff = ks * 64 + (lane >> 4) * 16;
            v4i fa[2], fb[2];
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const v4i*>(la + (wr * 32 + i * 16 + (lane & 15)) * kLdsPitch + koff);
                fb[i] = *reinterpret_cast<const v4i*>(lb + (wc * 32 + i * 16 + (lane & 15)) * kLdsPitch + koff);
            }
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }
    // S is accumulated chunk after chunk (launches on one stream: no two touch S at once)
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const int64_t col = (int64_t)tc * kT + wc * 32 + j * 16 + (lane & 15);
            for (int r = 0; r < 4; ++r) {
                const int64_t row = (int64_t)tr * kT + wr * 32 + i * 16 + (lane >> 4) * 4 + r;
                S[row * n_pad + col] += acc[i][j][r];
            }
        }
}

// c_j += sum_m g_jm mu_m over one chunk: one workgroup per sample, fixed strides and a fixed tree
__global__ void __launch_bounds__(256) sample_dot_mu_kernel(const int8_t* __restrict__ slab, int64_t ld, int64_t k_len,
                                                            const double* __restrict__ mu, double* __restrict__ c)
{
    __shared__ double red[256];
    const int32_t j = blockIdx.x;
    const int8_t* row = slab + (int64_t)j * ld;
    double s = 0.0;
    for (int64_t m = threadIdx.x; m < k_len; m += 256) s += (double)row[m] * mu[m];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) c[j] += red[0];
}

__global__ void __launch_bounds__(256) sum_squares_kernel(const double* __restrict__ mu, int64_t m_len, double* __restrict__ tau)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t m = threadIdx.x; m < m_len; m += 256) s += mu[m] * mu[m];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *tau += red[0];
}

__global__ void __launch_bounds__(256) centre_gram_kernel(const int32_t* __restrict__ S, int32_t n_pad, int32_t n,
                                                          const double* __restrict__ c, const double* __restrict__ tau,
                                                          double* __restrict__ C)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int32_t i = (int32_t)(e % n), j = (int32_t)(e / n);      // C column-major (it is symmetric)
    const int32_t s = (i / kT >= j / kT) ? S[(int64_t)i * n_pad + j] : S[(int64_t)j * n_pad + i];
    C[e] = (((double)s - c[i]) - c[j]) + *tau;
}

constexpr int kProjCols = 16;   // V columns per pass
constexpr int kProjRows = 128;  // samples per LDS stage

// UD[m][col0 + q] = sum_j g_jm V[j][col0 + q] - mu_m vsum[col0 + q], q < kc; one thread per marker, samples ascending
__global__ void __launch_bounds__(256) project_kernel(const int8_t* __restrict__ slab, int64_t ld, int64_t k_len, int32_t n,
                                                      const double* __restrict__ V, int32_t k, int32_t col0, int32_t kc,
                                                      const double* __restrict__ mu, const double* __restrict__ vsum,
                                                      double* __restrict__ UD)
{
    __shared__ double vs[kProjRows][kProjCols];
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double acc[kProjCols];
    for (int q = 0; q < kProjCols; ++q) acc[q] = 0.0;
    for (int32_t j0 = 0; j0 < n; j0 += kProjRows) {
        __syncthreads();
        for (int e = threadIdx.x; e < kProjRows * kProjCols; e += 256) {
            const int r = e / kProjCols, q = e % kProjCols;
            vs[r][q] = (j0 + r < n && q < kc) ? V[(int64_t)(j0 + r) * k + col0 + q] : 0.0;
        }
        __syncthreads();
        if (m < k_len) {
            const int32_t jn = min(kProjRows, n - j0);
            for (int32_t r = 0; r < jn; ++r) {
                const double g = (double)slab[(int64_t)(j0 + r) * ld + m];
                for (int q = 0; q < kProjCols; ++q) acc[q] += g * vs[r][q];
            }
        }
    }
    if (m >= k_len) return;
    for (int q = 0; q < kc; ++q) UD[m * k + col0 + q] = acc[q] - mu[m] * vsum[col0 + q];
}

}  // namespace

hipError_t launch_transpose_chunk(const int8_t* src, int64_t count, int32_t n, int8_t* dst, int64_t ld, hipStream_t s)
{
    dim3 grid((unsigned)((count + 63) / 64), (unsigned)((n + 63) / 64));
    hipLaunchKernelGGL(transpose_chunk_kernel, grid, dim3(256), 0, s, src, count, n, dst, ld);
    return hipGetLastError();
}

hipError_t launch_row_sums(const int8_t* src, int64_t count, int32_t n, int32_t* sums, hipStream_t s)
{
    hipLaunchKernelGGL(row_sums_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, src, count, n, sums);
    return hipGetLastError();
}

hipError_t launch_mu_from_sums(const int32_t* sums, int64_t count, int32_t n, double* mu, hipStream_t s)
{
    hipLaunchKernelGGL(mu_from_sums_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, sums, count, n, mu);
    return hipGetLastError();
}

hipError_t launch_gram_chunk(const int8_t* slab, int64_t ld, int64_t k_len, int32_t n_pad, int32_t* S, hipStream_t s)
{
    if (n_pad % kT || k_len % kKB || ld % 16) return hipErrorInvalidValue;
    const int nt = n_pad / kT;
    hipLaunchKernelGGL(gram_chunk_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, slab, ld, k_len, S, n_pad);
    return hipGetLastError();
}

hipError_t launch_sample_dot_mu(const int8_t* slab, int64_t ld, int64_t k_len, int32_t n, const double* mu, double* c,
                                hipStream_t s)
{
    hipLaunchKernelGGL(sample_dot_mu_kernel, dim3((unsigned)n), dim3(256), 0, s, slab, ld, k_len, mu, c);
    return hipGetLastError();
}

hipError_t launch_sum_squares(const double* mu, int64_t m, double* tau, hipStream_t s)
{
    hipLaunchKernelGGL(sum_squares_kernel, dim3(1), dim3(256), 0, s, mu, m, tau);
    return hipGetLastError();
}

hipError_t launch_centre_gram(const int32_t* S, int32_t n_pad, int32_t n, const double* c, const double* tau, double* C,
                              hipStream_t s)
{
    const int64_t e = (int64_t)n * n;
    hipLaunchKernelGGL(centre_gram_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, S, n_pad, n, c, tau, C);
    return hipGetLastError();
}

hipError_t launch_project(const int8_t* slab, int64_t ld, int64_t k_len, int32_t n, const double* V, int32_t k,
                          const double* mu, const double* vsum, double* UD, hipStream_t s)
{
    for (int32_t col0 = 0; col0 < k; col0 += kProjCols) {
        const int32_t kc = min(kProjCols, k - col0);
        hipLaunchKernelGGL(project_kernel, dim3((unsigned)((k_len + 255) / 256)), dim3(256), 0, s, slab, ld, k_len, n, V, k,
                           col0, kc, mu, vsum, UD);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vb2
