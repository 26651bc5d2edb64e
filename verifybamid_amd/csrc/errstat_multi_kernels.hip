// errstat_multi_kernels.hip -- gfx950 kernels for the batched E-step of the error-rate fit (vb2_abi.h
// section 3h): errstat_kernels.hip's sums for up to 64 samples in one launch pair.
//
// A workgroup works on exactly one sample (its job): the tables in LDS are that sample's alpha and error table.  Within the
// job it walks the sample's groups of 256 markers in stripes, one thread per marker, as the single kernel does.
//
// The bits are the single kernel's.  Pass one adds a marker's reads in file order from the same table; w, r, the clamp and
// the two fixed-point words are the same expressions (this unit is compiled with contraction off, as that one is); the
// log-likelihood is the same tree per group and the same in-order sum over a sample's groups.  Everything past r is integer.
// What differs keeps them:
//   * a group's contiguous read range read_off[m0] .. read_off[m0 + 256] is staged into LDS in chunks of kErrMultiChunk
//     reads with 16-byte loads, instead of every thread chasing its own byte loads.  A group that is one chunk is staged
//     once for both passes; a deeper one is staged again for pass two;
//   * what of the decode does not depend on the marker is done while staging: the quality clamped, the base upper-cased with
//     'a' -- which no upper-cased byte is -- for "." and ",".  The class is then two compares with the marker's allele;
//   * a run of equal (base, quality) within a marker has one r: it is binned as count x word, exact in integers.
#include "errstat_multi_kernels.h"

#include <hip/hip_runtime.h>

namespace vb2 {
namespace {

constexpr int kT = kErrThreads;
constexpr int kQ = kErrNumQual;
constexpr int kChunk = kErrMultiChunk;
constexpr unsigned kRefCode = 'a';
constexpr double kMinAf = 0.00005, kMaxAf = 0.99995;      // h:94-95
constexpr double kTwo32 = 4294967296.0;

static_assert(kChunk % 16 == 0, "a chunk is whole 16-byte loads");

// ---- errstat_kernels.hip's own expressions ----
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

__device__ __forceinline__ void tree_sum(double* part, int tid)
{
    __syncthreads();
    for (int h = kT / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
}

// ---- the staged code of a read: the base's byte below, the clamped quality above ----
__device__ __forceinline__ unsigned code_of(unsigned b, unsigned qc)
{
    unsigned nb = (b >= 'a' && b <= 'z') ? b - 32u : b;
    nb = (b == '.' || b == ',') ? kRefCode : nb;
    int q = (int)qc - 33;
    q = q < 0 ? 0 : q;
    q = q > 93 ? 93 : q;
    return nb | ((unsigned)q << 8);
}

__device__ __forceinline__ unsigned codes_of(unsigned bw, unsigned qw, int i)           // reads i, i + 1 of a word of four
{
    const unsigned lo = code_of((bw >> (8 * i)) & 255u, (qw >> (8 * i)) & 255u);
    const unsigned hi = code_of((bw >> (8 * i + 8)) & 255u, (qw >> (8 * i + 8)) & 255u);
    return lo | (hi << 16);
}

// reads cs .. end of the sample (both multiples of 16, end - cs <= kChunk) into stage[0 .. end - cs)
__device__ __forceinline__ void stage_chunk(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, int64_t cs,
                                            int64_t end, unsigned short* stage, int tid)
{
    const int len = (int)(end - cs);
    for (int o = 16 * tid; o < len; o += 16 * kT) {
        const uint4 b = *reinterpret_cast<const uint4*>(bases + cs + o);
        const uint4 q = *reinterpret_cast<const uint4*>(quals + cs + o);
        uint4 lo4, hi4;
        lo4.x = codes_of(b.x, q.x, 0); lo4.y = codes_of(b.x, q.x, 2);
        lo4.z = codes_of(b.y, q.y, 0); lo4.w = codes_of(b.y, q.y, 2);
        hi4.x = codes_of(b.z, q.z, 0); hi4.y = codes_of(b.z, q.z, 2);
        hi4.z = codes_of(b.w, q.w, 0); hi4.w = codes_of(b.w, q.w, 2);
        uint4* dst = reinterpret_cast<uint4*>(stage + o);
        dst[0] = lo4;
        dst[1] = hi4;
    }
}

__device__ __forceinline__ int class_of_code(unsigned nb, unsigned alt_up) { return nb == kRefCode ? 0 : (nb == alt_up ? 1 : 2); }

__global__ void __launch_bounds__(kT)
errstat_multi_marker_kernel(const ErrMultiJob* __restrict__ jobs, const int* __restrict__ wg_job,
                            unsigned long long* __restrict__ slab, double* __restrict__ partial)
{
    __shared__ double tab_l[2 * kQ * 9];          // log p [class][quality][pair]
    __shared__ double tab_r[2 * kQ * 9];          // M_E eps / p
    __shared__ double other_l[kQ];                // log(2/3 eps)
    __shared__ unsigned long long bins[kErrBinWords];
    __shared__ double part[kT];
    __shared__ __attribute__((aligned(16))) unsigned short stage[kChunk];
    const int tid = threadIdx.x;
    const ErrMultiJob* job = jobs + wg_job[blockIdx.x];
    const int bx = (int)blockIdx.x - job->wg_first, nbx = job->wg_count;
    const ErrStatPoint* __restrict__ point = job->point;
    const int M = job->in.num_marker, k = job->in.num_pc;
    const uint8_t* __restrict__ bases = job->in.bases;
    const uint8_t* __restrict__ quals = job->in.quals;
    const int64_t* __restrict__ read_off = job->in.read_off;
    const uint8_t* __restrict__ alt_base = job->in.alt_base;
    const double* __restrict__ ud = job->in.ud;
    const double* __restrict__ mu_ = job->in.mu;
    const double* __restrict__ known_af = job->in.known_af;
    const double avg_depth = job->in.avg_depth, sd_depth = job->in.sd_depth;
    const bool sanity_disabled = job->in.sanity_disabled != 0;
    const double alpha = point->alpha;

    // ---- the job's tables ----
    for (int e = tid; e < 2 * kQ * 9; e += kT) {
        const int c = e / (kQ * 9), rem = e - c * (kQ * 9), q = rem / 9, p = rem - q * 9;
        const int g1 = p / 3, g2 = p - 3 * g1;
        const double eps = point->err[q];
        const double one_minus_alpha = 1.0 - alpha;
        const double me = (alpha * cond_err(g1, c) + one_minus_alpha * cond_err(g2, c)) * eps;
        const double mn = (alpha * cond_ok(g1, c) + one_minus_alpha * cond_ok(g2, c)) * (1.0 - eps);
        const double pr = me + mn;
        tab_l[e] = log(pr);
        tab_r[e] = pr > 0.0 ? me / pr : 0.0;
    }
    for (int e = tid; e < kQ; e += kT) other_l[e] = log((2.0 / 3.0) * point->err[e]);
    for (int e = tid; e < kErrBinWords; e += kT) bins[e] = 0ull;
    __syncthreads();

    const int ngrp = (M + kT - 1) / kT;
    const bool kaf = known_af != nullptr;
    for (int grp = bx; grp < ngrp; grp += nbx) {
        const int m0 = grp * kT, m = m0 + tid;
        const int mend = m0 + kT < M ? m0 + kT : M;
        // the group's reads, widened to whole 16-byte loads (the arrays end on a multiple of 256 bytes)
        const int64_t g0 = read_off[m0] & ~(int64_t)15, gend = (read_off[mend] + 15) & ~(int64_t)15;
        const bool one_chunk = gend - g0 <= kChunk;
        int64_t lo = 0, hi = 0;
        bool walk = false;
        unsigned alt_up = 0;
        if (m < M) {
            lo = read_off[m];
            hi = read_off[m + 1];
            const double depth = (double)(hi - lo);
            walk = hi > lo;                                                         // h:239, 244
            if (walk && !sanity_disabled)                                           // h:246-249
                walk = !(depth < avg_depth - 3 * sd_depth || depth > avg_depth + 3 * sd_depth);
            const unsigned alt = alt_base[m];
            alt_up = (alt >= 'a' && alt <= 'z') ? alt - 32u : alt;
        }
        // ---- pass one: the nine sums of logarithms, the reads in file order over the chunks ----
        double A[9], c_other = 0.0;
#pragma unroll
        for (int p = 0; p < 9; ++p) A[p] = 0.0;
        for (int64_t cs = g0; cs < gend; cs += kChunk) {
            const int64_t ce = cs + kChunk < gend ? cs + kChunk : gend;
            __syncthreads();                                    // the chunk before is read
            stage_chunk(bases, quals, cs, ce, stage, tid);
            __syncthreads();
            if (walk) {
                // (both within [0, kErrMultiChunk]: the marker's range clipped to the chunk before the offsets are narrowed)
                const int j0 = (int)((lo > cs ? lo : cs) - cs), j1 = (int)((hi < ce ? hi : ce) - cs);
                for (int j = j0; j < j1; ++j) {
                    const unsigned code = stage[j];
                    const int c = class_of_code(code & 255u, alt_up), q = (int)(code >> 8);
                    if (c == 2) {
                        c_other += other_l[q];
                    } else {
                        const double* t = tab_l + (c * kQ + q) * 9;
#pragma unroll
                        for (int p = 0; p < 9; ++p) A[p] += t[p];
                    }
                }
            }
        }
        double val = 0.0, w[9];
        bool counts = false;
        if (walk) {
            double af1, af2;
            if (kaf) {
                af1 = af2 = known_af[m];
            } else {
                af1 = 0.0; af2 = 0.0;
                const double* u = ud + (size_t)m * (size_t)k;
                for (int kk = 0; kk < k; ++kk) {
                    af1 = fma(u[kk], point->pc1[kk], af1);
                    af2 = fma(u[kk], point->pc2[kk], af2);
                }
                const double mu = mu_[m];
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
                counts = true;
                val = log(lk);
                double ls = 0.0;
#pragma unroll
                for (int p = 0; p < 9; ++p) {
                    w[p] = exp(A[p] - amax) * G1[p / 3] * G2[p % 3];
                    ls += w[p];
                }
                const double inv = 1.0 / ls;
#pragma unroll
                for (int p = 0; p < 9; ++p) w[p] *= inv;
            }
        }
        // ---- pass two: r per run of equal reads, binned in fixed point ----
        for (int64_t cs = g0; cs < gend; cs += kChunk) {
            const int64_t ce = cs + kChunk < gend ? cs + kChunk : gend;
            if (!one_chunk) {                                   // (uniform: the chunk of pass one is still there otherwise)
                __syncthreads();
                stage_chunk(bases, quals, cs, ce, stage, tid);
                __syncthreads();
            }
            if (counts) {
                const int j0 = (int)((lo > cs ? lo : cs) - cs), j1 = (int)((hi < ce ? hi : ce) - cs);
                int j = j0;
                while (j < j1) {
                    const unsigned code = stage[j];
                    unsigned long long run = 1ull;
                    for (++j; j < j1 && stage[j] == code; ++j) ++run;
                    const int c = class_of_code(code & 255u, alt_up), q = (int)(code >> 8);
                    double r = 1.0;
                    if (c != 2) {
                        const double* t = tab_r + (c * kQ + q) * 9;
                        r = 0.0;
#pragma unroll
                        for (int p = 0; p < 9; ++p) r += w[p] * t[p];
                        r = r > 1.0 ? 1.0 : r;
                    }
                    const double scaled = r * kTwo32;                        // exact: a power of two
                    const unsigned long long h32 = (unsigned long long)scaled;
                    const unsigned long long l32 = (unsigned long long)((scaled - (double)h32) * kTwo32);
                    atomicAdd(&bins[q], run);
                    atomicAdd(&bins[kQ + q], run * h32);
                    atomicAdd(&bins[2 * kQ + q], run * l32);
                }
            }
        }
        part[tid] = val;
        tree_sum(part, tid);
        if (tid == 0) partial[job->grp_first + grp] = part[0];
        __syncthreads();                                        // part[] and stage[] are written again in the next round
    }
    __syncthreads();
    for (int e = tid; e < kErrBinWords; e += kT) slab[(size_t)blockIdx.x * kErrBinWords + e] = bins[e];
}

// one workgroup per job: its workgroups' bins added, its groups' log-likelihoods in order (errstat_reduce_kernel's sums)
__global__ void __launch_bounds__(kT)
errstat_multi_reduce_kernel(const ErrMultiJob* __restrict__ jobs, const unsigned long long* __restrict__ slab,
                            const double* __restrict__ partial, unsigned long long* __restrict__ out)
{
    __shared__ double part[kT];
    const int tid = threadIdx.x;
    const ErrMultiJob* job = jobs + blockIdx.x;
    const int nslab = job->wg_count, ngrp = (job->in.num_marker + kT - 1) / kT;
    const unsigned long long* s0 = slab + (size_t)job->wg_first * kErrBinWords;
    const double* p0 = partial + job->grp_first;
    unsigned long long* o = out + (size_t)job->sample * kErrOutWords;
    for (int e = tid; e < kErrBinWords; e += kT) {
        unsigned long long sum = 0ull;
        for (int b = 0; b < nslab; ++b) sum += s0[(size_t)b * kErrBinWords + e];
        o[e] = sum;
    }
    double sum = 0.0;
    for (int i = tid; i < ngrp; i += kT) sum += p0[i];
    part[tid] = sum;
    tree_sum(part, tid);
    if (tid == 0) o[kErrBinWords] = (unsigned long long)__double_as_longlong(part[0]);
}

}  // namespace

hipError_t launch_errstat_multi(const ErrMultiJob* d_jobs, int num_job, const int* d_wg_job, int grid, int num_sample,
                                unsigned long long* d_slab, double* d_partial, unsigned long long* d_out, hipStream_t stream)
{
    if (num_sample < 1 || num_sample > kErrMultiMaxSample || num_job < 0 || num_job > num_sample) return hipErrorInvalidValue;
    hipError_t rc = hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * kErrOutWords * (size_t)num_sample, stream);
    if (rc != hipSuccess || num_job == 0) return rc;
    if (grid < num_job) return hipErrorInvalidValue;
    hipLaunchKernelGGL(errstat_multi_marker_kernel, dim3((unsigned)grid), dim3(kT), 0, stream, d_jobs, d_wg_job, d_slab, d_partial);
    rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(errstat_multi_reduce_kernel, dim3((unsigned)num_job), dim3(kT), 0, stream, d_jobs, d_slab, d_partial, d_out);
    return hipGetLastError();
}

}  // namespace vb2
