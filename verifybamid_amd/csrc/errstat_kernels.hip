// errstat_kernels.hip -- gfx950 kernels for the E-step of the error-rate fit (vb2_abi.h section 3h).
//
// Every read has a latent indicator "this read is an error".  With eps the error rate of the read's clamped quality,
// E / N = P(class | genotype, error / no error) (h:164-177) and M_E = alpha E[g1][c] + (1 - alpha) E[g2][c], M_N likewise,
//     p(read | g1, g2) = M_E eps + M_N (1 - eps)                                                     (h:223-225)
//     r = sum over (g1, g2) of  w(g1, g2) M_E eps / p,     w = GF1[g1] GF2[g2] W[g1][g2] / L
// the posterior over the genotype pairs taken from ALL the marker's reads.  A class-other read is an error for certain.
// Per quality: n = the reads of the counted markers, s = the sum of their r.
//
// One thread per marker of the panel order, two passes over its reads.  Pass one adds the nine logarithms of a read from a
// table in LDS (2 classes x 94 qualities x 9 pairs, and the class-other term per quality) and forms w with the largest sum
// subtracted, so depth never underflows the weights; whether the marker counts is the reference's rule on its own double L
// (h:307-310).  Pass two takes r = w . R[class][quality] from a second table and bins it.
//
// n, s and the log-likelihood are the same bits whatever the grid and from call to call.  r is binned in fixed point --
// floor(r 2^32) and the next 32 bits, each added with a 64-bit integer LDS atomic to the workgroup's bins, stored to a slab
// and summed by errstat_reduce_kernel: integer addition is associative.  What a read loses is below 2^-64.  The
// log-likelihood is one fixed tree per group of 256 markers and one fixed-order sum over the groups.
#include "errstat_kernels.h"

#include <hip/hip_runtime.h>

namespace vb2 {
namespace {

constexpr int kT = kErrThreads;
constexpr int kQ = kErrNumQual;
constexpr double kMinAf = 0.00005, kMaxAf = 0.99995;      // h:94-95
constexpr double kTwo32 = 4294967296.0;

// P(class | genotype, error) and P(class | genotype, no error), class 0 ref, 1 alt (h:164-177)
__device__ __forceinline__ double cond_err(int g, int c) { return (double)(c == 0 ? g : 2 - g) * (1.0 / 6.0); }
__device__ __forceinline__ double cond_ok(int g, int c) { return c == 0 ? 1.0 - 0.5 * (double)g : 0.5 * (double)g; }

__device__ __forceinline__ void gf_of(double af, double* gf)
{
    if (af < kMinAf) af = kMinAf;
    if (af > kMaxAf) af = kMaxAf;
    gf[0] = (1 - af) * (1 - af);
    gf[1] = 2 * (af) * (1 - af);
    gf[2] = af * af;
}

// fixed tree over the workgroup's 256 values (as walk::tree_sum of marker_walk.h)
__device__ __forceinline__ void tree_sum(double* part, int tid)
{
    __syncthreads();
    for (int h = kT / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
}

// classifyBase (h:180-184): '.' ',' -> ref; toupper(base) == toupper(alt) -> alt; else other
__device__ __forceinline__ int class_of(unsigned b, unsigned alt_up)
{
    if (b == '.' || b == ',') return 0;
    const unsigned up = (b >= 'a' && b <= 'z') ? b - 32u : b;
    return up == alt_up ? 1 : 2;
}

__device__ __forceinline__ int clamp_qual(unsigned qc)
{
    int q = (int)qc - 33;
    q = q < 0 ? 0 : q;
    return q > 93 ? 93 : q;
}

template <int K>
__global__ void __launch_bounds__(kT)
errstat_marker_kernel(const ErrStatInput in, const ErrStatPoint* __restrict__ point, unsigned long long* __restrict__ slab,
                      double* __restrict__ partial)
{
    __shared__ double tab_l[2 * kQ * 9];          // log p [class][quality][pair]
    __shared__ double tab_r[2 * kQ * 9];          // M_E eps / p
    __shared__ double other_l[kQ];                // log(2/3 eps)
    __shared__ unsigned long long bins[kErrBinWords];
    __shared__ double part[kT];
    const int tid = threadIdx.x;
    const int bx = (int)blockIdx.x, nbx = (int)gridDim.x;
    const int k = K ? K : in.num_pc;
    const double alpha = point->alpha;

    // ---- the launch's tables ----
    for (int e = tid; e < 2 * kQ * 9; e += kT) {
        const int c = e / (kQ * 9), rem = e - c * (kQ * 9), q = rem / 9, p = rem - q * 9;
        const int g1 = p / 3, g2 = p - 3 * g1;
        const double eps = point->err[q];
        const double one_minus_alpha = 1.0 - alpha;
        const double me = (alpha * cond_err(g1, c) + one_minus_alpha * cond_err(g2, c)) * eps;
        const double mn = (alpha * cond_ok(g1, c) + one_minus_alpha * cond_ok(g2, c)) * (1.0 - eps);
        const double pr = me + mn;
        tab_l[e] = log(pr);                         // (-inf where no such read can be: the pair's W is 0)
        tab_r[e] = pr > 0.0 ? me / pr : 0.0;        // a term whose denominator is 0 is 0; its w is 0 too
    }
    for (int e = tid; e < kQ; e += kT) other_l[e] = log((2.0 / 3.0) * point->err[e]);
    for (int e = tid; e < kErrBinWords; e += kT) bins[e] = 0ull;
    __syncthreads();

    const int ngrp = (in.num_marker + kT - 1) / kT;
    const bool kaf = in.known_af != nullptr;
    for (int grp = bx; grp < ngrp; grp += nbx) {
        const int m = grp * kT + tid;
        double val = 0.0;
        if (m < in.num_marker) {
            const int64_t lo = in.read_off[m], hi = in.read_off[m + 1];
            const double depth = (double)(hi - lo);
            bool walk = hi > lo;                                                    // h:239, 244
            if (walk && !in.sanity_disabled)                                        // h:246-249
                walk = !(depth < in.avg_depth - 3 * in.sd_depth || depth > in.avg_depth + 3 * in.sd_depth);
            if (walk) {
                const unsigned alt = in.alt_base[m];
                const unsigned alt_up = (alt >= 'a' && alt <= 'z') ? alt - 32u : alt;
                // ---- pass one: the nine sums of logarithms ----
                double A[9], c_other = 0.0;
#pragma unroll
                for (int p = 0; p < 9; ++p) A[p] = 0.0;
                for (int64_t j = lo; j < hi; ++j) {
                    const int c = class_of(in.bases[j], alt_up), q = clamp_qual(in.quals[j]);
                    if (c == 2) {
                        c_other += other_l[q];
                    } else {
                        const double* t = tab_l + (c * kQ + q) * 9;
#pragma unroll
                        for (int p = 0; p < 9; ++p) A[p] += t[p];
                    }
                }
                double af1, af2;
                if (kaf) {
                    af1 = af2 = in.known_af[m];
                } else {
                    af1 = 0.0; af2 = 0.0;
                    const double* u = in.ud + (size_t)m * (size_t)k;
#pragma unroll
                    for (int kk = 0; kk < k; ++kk) {
                        af1 = fma(u[kk], point->pc1[kk], af1);
                        af2 = fma(u[kk], point->pc2[kk], af2);
                    }
                    const double mu = in.mu[m];
                    af1 += mu; af1 /= 2.0;
                    af2 += mu; af2 /= 2.0;
                }
                double G1[3], G2[3];
                gf_of(af1, G1);
                gf_of(af2, G2);
                // L as the reference forms it (h:307-309): the marker counts where it is > 0 (h:310)
                double lk = 0.0, amax = -__builtin_inf();
#pragma unroll
                for (int p = 0; p < 9; ++p) {
                    lk += exp(A[p] + c_other) * G1[p / 3] * G2[p % 3];
                    amax = A[p] > amax ? A[p] : amax;
                }
                if (lk > 0) {
                    val = log(lk);
                    double w[9], ls = 0.0;
#pragma unroll
                    for (int p = 0; p < 9; ++p) {
                        w[p] = exp(A[p] - amax) * G1[p / 3] * G2[p % 3];
                        ls += w[p];
                    }
                    const double inv = 1.0 / ls;
#pragma unroll
                    for (int p = 0; p < 9; ++p) w[p] *= inv;
                    // ---- pass two: r per read, binned in fixed point ----
                    for (int64_t j = lo; j < hi; ++j) {
                        const int c = class_of(in.bases[j], alt_up), q = clamp_qual(in.quals[j]);
                        double r = 1.0;
                        if (c != 2) {
                            const double* t = tab_r + (c * kQ + q) * 9;
                            r = 0.0;
#pragma unroll
                            for (int p = 0; p < 9; ++p) r += w[p] * t[p];
                            r = r > 1.0 ? 1.0 : r;
                        }
                        const double scaled = r * kTwo32;                    // exact: a power of two
                        const unsigned long long h32 = (unsigned long long)scaled;
                        const unsigned long long l32 = (unsigned long long)((scaled - (double)h32) * kTwo32);
                        atomicAdd(&bins[q], 1ull);
                        atomicAdd(&bins[kQ + q], h32);
                        atomicAdd(&bins[2 * kQ + q], l32);
                    }
                }
            }
        }
        part[tid] = val;
        tree_sum(part, tid);
        if (tid == 0) partial[grp] = part[0];
        __syncthreads();                                        // part[] is written again in the next round
    }
    __syncthreads();
    for (int e = tid; e < kErrBinWords; e += kT) slab[(size_t)bx * kErrBinWords + e] = bins[e];
}

__global__ void __launch_bounds__(kT)
errstat_reduce_kernel(const unsigned long long* __restrict__ slab, int nslab, const double* __restrict__ partial, int ngrp,
                      unsigned long long* __restrict__ out)
{
    __shared__ double part[kT];
    const int tid = threadIdx.x;
    for (int e = tid; e < kErrBinWords; e += kT) {
        unsigned long long sum = 0ull;
        for (int b = 0; b < nslab; ++b) sum += slab[(size_t)b * kErrBinWords + e];
        out[e] = sum;
    }
    double sum = 0.0;
    for (int i = tid; i < ngrp; i += kT) sum += partial[i];
    part[tid] = sum;
    tree_sum(part, tid);
    if (tid == 0) out[kErrBinWords] = (unsigned long long)__double_as_longlong(part[0]);
}

template <int K>
void launch_marker(const ErrStatInput& in, const ErrStatPoint* d_point, int grid, unsigned long long* d_slab, double* d_partial,
                   hipStream_t stream)
{
    hipLaunchKernelGGL((errstat_marker_kernel<K>), dim3((unsigned)grid), dim3(kT), 0, stream, in, d_point, d_slab, d_partial);
}

}  // namespace

hipError_t launch_errstat(const ErrStatInput& in, const ErrStatPoint* d_point, int grid, unsigned long long* d_slab,
                          double* d_partial, unsigned long long* d_out, hipStream_t stream)
{
    const int ngrp = errstat_groups(in.num_marker);
    if (ngrp <= 0) return hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * kErrOutWords, stream);
    if (grid < 1 || grid > ngrp) return hipErrorInvalidValue;
    const int ksel = in.known_af ? 0 : (in.num_pc == 2 || in.num_pc == 4) ? in.num_pc : 0;
    if (ksel == 2) launch_marker<2>(in, d_point, grid, d_slab, d_partial, stream);
    else if (ksel == 4) launch_marker<4>(in, d_point, grid, d_slab, d_partial, stream);
    else launch_marker<0>(in, d_point, grid, d_slab, d_partial, stream);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(errstat_reduce_kernel, dim3(1), dim3(kT), 0, stream, d_slab, grid, d_partial, ngrp, d_out);
    return hipGetLastError();
}

}  // namespace vb2
