// refbias_kernels.hip -- gfx950 kernels for the log-likelihood under a reference bias (vb2_abi.h
// section 3g): beta = P(an error-free read of a heterozygous genotype shows REF) in place of the model's constant 0.5,
// one beta per ROW of a set, many points of many rows in one launch.
//
//     class ref:  u(g; e, beta) = (g / 6) e + n_beta(g) (1 - e),        n_beta = {1, beta, 0}[g]
//     class alt:  the ref entry at 1 - beta, read mirrored (g -> 2 - g)
//
// The kernel has the shape of llk_sum_marker_kernel (marker_sum_kernels.hip) and walks the context's layouts through
// marker_walk.h; what differs is the table.  A bias breaks the two facts the other units' tables rest on: class alt is no
// longer class ref mirrored (it is class ref mirrored AT 1 - beta), and the (het, het) entry is no constant of the context
// (L.ediag[2] holds it at beta = 0.5).  So:
//   * probability domain: a table row holds fourteen doubles -- the six off-diagonal pairs and (het, het) at beta, then the
//     same seven at 1 - beta.  A ref step multiplies columns 0..6, an alt step the second half mirrored (pair 5 - p; the het
//     column as it is).  The powers P^2..P^K, the padding row and the window rows are built over all fourteen columns.
//   * run words: seven logarithms per code; a class-alt code's row is built with g -> 2 - g AND beta -> 1 - beta, on its
//     own (it is not the mirror of its twin).
//   * epilogue: W[1][1] = cst acc[6] (run words: exp(c_other + sum)), W[0][0] and W[2][2] from L.ediag as ever.
// One thread per marker, the fixed tree per tile group and llk_bias_reduce_kernel per point: a point's value is the same
// bits whatever else the launch holds.
#include "refbias_kernels.h"

#include "marker_walk.h"

namespace vb2 {
namespace {

using namespace walk;

// section 3g for one class-ref quality and pair, in the reference's expression order (h:223-225); negative (alpha outside
// [0, 1]): NaN, the marker is left out.  At beta = 0.5 these are the bits of entry_of (marker_walk.h).
__device__ __forceinline__ double bias_entry(double alpha, double p_err, int g1, int g2, double beta)
{
    const double p_ok = 1.0 - p_err;
    const double e1 = (double)g1 * (1.0 / 6.0), e2 = (double)g2 * (1.0 / 6.0);
    const double n1 = g1 == 0 ? 1.0 : g1 == 1 ? beta : 0.0, n2 = g2 == 0 ? 1.0 : g2 == 1 ? beta : 0.0;
    const double one_minus_alpha = 1.0 - alpha;
    const double p = (alpha * e1 + one_minus_alpha * e2) * p_err + (alpha * n1 + one_minus_alpha * n2) * p_ok;
    return p >= 0.0 ? p : __builtin_nan("");
}

// column 0..5: the off-diagonal pair; 6: (het, het)
__device__ __forceinline__ void column_g(int p, int& g1, int& g2)
{
    if (p < 6) pair_g(p, g1, g2);
    else g1 = g2 = 1;
}

template <bool PD, int K>
__global__ void __launch_bounds__(kThreads)
llk_bias_marker_kernel(const DeviceLayout L, const double* __restrict__ points, const int32_t* __restrict__ row_of,
                       const double* __restrict__ rows, double* __restrict__ partial)
{
    constexpr int ROW = PD ? kBiasRowDoublesPd : kBiasRowDoublesRun;
    extern __shared__ __attribute__((aligned(16))) double tab[];      // [nrow][ROW], then the tree's [256]
    const int tid = threadIdx.x;
    const int pt = (int)blockIdx.y, bx = (int)blockIdx.x, nbx = (int)gridDim.x;
    const int k = K ? K : L.num_pc, stride = 2 * k + 1;
    const double* prow = points + (size_t)pt * stride;
    const double alpha = prow[2 * k];
    const double beta = rows[row_of[pt]];
    const int nrow = L.num_code + 1;
    const size_t mp = (size_t)L.m_pad;
    double* part = tab + (size_t)nrow * ROW;

    // ---- the point's table ----
    for (int e = tid; e < num_single<PD>(L) * ROW; e += kThreads) {
        const int pi = e / ROW, c = e - pi * ROW;
        const SingleRec rec = single_rec(L, pi);
        int g1, g2;
        if constexpr (PD) {
            const int half = c >= 7 ? 1 : 0;
            column_g(c - 7 * half, g1, g2);
            const double v = bias_entry(alpha, rec.p_err, g1, g2, half ? 1.0 - beta : beta);
            const int kq = rec.kq(), rstep = rec.rstep();
            double r = v;
            for (int n = 1; n <= kq; ++n) {
                const int row = rec.first + (n - 1) * rstep;
                if (row >= 0 && row < nrow) tab[(size_t)row * ROW + c] = r;
                r *= v;
            }
        } else {
            column_g(c, g1, g2);
            const double pe = fabs(rec.p_err);
            const double lref = log(bias_entry(alpha, pe, g1, g2, beta));
            const double lalt = log(bias_entry(alpha, pe, 2 - g1, 2 - g2, 1.0 - beta));
            if (rec.first < nrow) tab[(size_t)rec.first * ROW + c] = rec.alt() ? lalt : lref;
            if (rec.has_twin() && rec.twin < nrow) tab[(size_t)rec.twin * ROW + c] = lalt;
        }
    }
    for (int e = tid; e < ROW; e += kThreads)                   // padding row: P = 1 (log domain: 0)
        tab[(size_t)L.num_code * ROW + e] = PD ? 1.0 : 0.0;
    if constexpr (PD)
        for_each_window<ROW>(L, nrow, tid, [&](uint32_t ra, uint32_t rb, uint32_t dst, int p) {
            tab[(size_t)dst * ROW + p] = tab[(size_t)ra * ROW + p] * tab[(size_t)rb * ROW + p];
        });
    __syncthreads();

    // ---- one thread per marker of the sorted order, one partial sum per tile group ----
    const int m = tid & 15;
    const int ntile_grp = tile_groups(L);
    const bool kaf = L.known_af != nullptr;
    for (int tg = bx; tg < ntile_grp; tg += nbx) {
        const int mt = tg * 16 + (tid >> 4);
        const size_t pos = (size_t)mt * 16 + (size_t)m;
        double val = 0.0;
        if (mt < L.num_mt && pos < (size_t)L.num_active) {
            const uint2 rec = L.mt_rec[mt];
            double acc[7];
            for (int p = 0; p < 7; ++p) acc[p] = PD ? 1.0 : L.ediag[pos];       // log domain: c_other, summed here
            for_each_step<PD, ROW>(L, tab, nrow, rec, m, [&](const double* t, bool alt, double n) {
                if constexpr (PD) {
#pragma unroll
                    for (int p = 0; p < 6; ++p) acc[p] *= t[alt ? 7 + 5 - p : p];
                    acc[6] *= t[alt ? 13 : 6];
                } else {
#pragma unroll
                    for (int p = 0; p < 7; ++p) acc[p] = fma(n, t[p], acc[p]);
                }
            });
            // ---- epilogue: L = G1' W GF2; of W's diagonal only the two homozygous entries are the context's constants ----
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
            const double cst = PD ? L.ediag[pos] : 0.0;
            W[0][0] = L.ediag[mp + pos];
            W[1][1] = PD ? cst * acc[6] : exp(acc[6]);
            W[2][2] = L.ediag[3 * mp + pos];
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
llk_bias_reduce_kernel(const double* __restrict__ partial, int ntile_grp, double* __restrict__ out)
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

template <bool PD, int K>
void launch_marker(const DeviceLayout& L, dim3 grid, size_t shmem, hipStream_t stream, const double* d_points,
                   const int32_t* d_row_of, const double* d_rows, double* d_partial)
{
    hipLaunchKernelGGL((llk_bias_marker_kernel<PD, K>), grid, dim3(kThreads), shmem, stream, L, d_points, d_row_of, d_rows,
                       d_partial);
}

}  // namespace

hipError_t launch_llk_bias(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_row,
                           const double* d_beta, double* d_partial, double* d_out, hipStream_t stream)
{
    if (num_point <= 0) return hipSuccess;
    if (num_point > kMaxPointsPerLaunch) return hipErrorInvalidValue;
    const int nrow = L.num_code + 1;
    const size_t shmem = ((size_t)nrow * (L.pd ? kBiasRowDoublesPd : kBiasRowDoublesRun) + kThreads) * sizeof(double);
    if (shmem > 64 * 1024) return hipErrorInvalidValue;      // (at most 189 rows of 14 doubles and the tree: 23 KiB)
    const int ntile_grp = tile_groups(L);
    if (ntile_grp > 0) {
        const dim3 grid((unsigned)stripe_grid(L, num_point), (unsigned)num_point);
        const int ksel = L.known_af ? 0 : (L.num_pc == 2 || L.num_pc == 4) ? L.num_pc : 0;
        if (L.pd) {
            if (ksel == 2) launch_marker<true, 2>(L, grid, shmem, stream, d_points, d_row, d_beta, d_partial);
            else if (ksel == 4) launch_marker<true, 4>(L, grid, shmem, stream, d_points, d_row, d_beta, d_partial);
            else launch_marker<true, 0>(L, grid, shmem, stream, d_points, d_row, d_beta, d_partial);
        } else {
            if (ksel == 2) launch_marker<false, 2>(L, grid, shmem, stream, d_points, d_row, d_beta, d_partial);
            else if (ksel == 4) launch_marker<false, 4>(L, grid, shmem, stream, d_points, d_row, d_beta, d_partial);
            else launch_marker<false, 0>(L, grid, shmem, stream, d_points, d_row, d_beta, d_partial);
        }
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(llk_bias_reduce_kernel, dim3((unsigned)num_point), dim3(kThreads), 0, stream, d_partial, ntile_grp, d_out);
    return hipGetLastError();
}

}  // namespace vb2
