// marker_sum_kernels.hip -- gfx950 kernels for the two log-likelihoods that are a sum of one term per marker over ONE
// resident sample, at many points at once (DESIGN.md sections 12 and 13):
//     LLK_w(theta)     = sum_i w_i log L_i(theta)                                   integer marker weights ("replicates")
//     LLK(theta | h)   = sum_m log sum_g1 P_h[m][g1] sum_g2 GF2[g2] W[g1][g2]       a hypothesised contaminant's genotypes
// The file walks the layouts the context already holds (llk_kernels.h: DeviceLayout) in both forms through marker_walk.h and
// makes no second copy of the reads.  The two differ in a marker's Term and in nothing else:
//
//   * WeightTerm: a byte of the point's weight row; a marker of weight 0 is not walked at all; the term is w log L -- L^w
//     as ONE logarithm times w, so that a weight of 255 on a marker whose L is 1e-300 neither underflows nor costs 255
//     multiplications.
//   * PriorTerm: three coalesced floats of the point's hypothesis, P_h[m] (the genotype posterior of another sample of the
//     cohort), in flight under the walk; where the triple is not all zero it stands in for the Hardy-Weinberg prior
//     GF1(pc1); the term is log L.
//   * PairTerm: six coalesced floats of the point's hypothesis, pi1_h[m] and pi2_h[m]; a negative
//     pi2_h[m][0] leaves the marker out like a weight of 0; a triple that is not all zero stands in for GF1(pc1) or
//     GF2(pc2); the term is log L.
//   * llk_sum_marker_kernel<Term, PD, K>: one workgroup per (stripe of 16-tile groups, point).  It builds the point's table
//     in LDS -- per table row the six off-diagonal genotype pairs' P^n (probability domain) or log p (run words) -- and
//     one thread per marker walks the marker's steps or runs, forms L = G1' W GF2 in the reference's order (h:307-309)
//     and, where L > 0 (h:310), takes the term.  The 256 values of a tile group are summed by a fixed tree into
//     partial[point][group].  K = 2, 4: the projection loops unrolled for that --NumPC (the evaluation kernels' KSEL);
//     K = 0: any --NumPC.
//   * llk_sum_reduce_kernel: one workgroup per point sums the point's partial sums -- thread t takes groups t, t + 256,
//     ..., then the same tree.  Which workgroup walked a group does not enter: a point's result is the same bits whatever
//     else the launch holds, however many workgroups share the point, and from one call to the next.
//   * weights_permute_kernel, prior_permute_kernel: the caller's rows (panel order) into the context's sorted order, once
//     per set -- bytes [m_pad] per replicate; three planes [3][m_pad] per hypothesis (structure of arrays, so that the
//     marker kernel's thread of sorted position tg * 256 + tid reads three coalesced floats).
//   * pair_permute_kernel, pair_build_kernel: the six planes [6][m_pad] of a pair hypothesis, from the caller's rows
//     [M][6] or, device to device, from the q plane of a source set's row under the rule of section 16.
#include "marker_sum_kernels.h"

#include "marker_walk.h"

namespace vb2 {
namespace {

using namespace walk;

constexpr int kRowDoubles = 6;                    // the six off-diagonal genotype pairs (the diagonal: the context's constants)

// A Term: a marker's share of the sum, a small struct the kernel makes per marker from the point's row of its `rows`
// argument (Row, row_elems) and holds by value.  walks() -- false: the marker is not walked --, then, behind the marker's
// record, load(); prior() may replace G1 and G2, and value() turns L into what the marker adds.  (walks and load are two calls
// because the weight has to be read before the marker's record and the prior's triple behind it, inside the one branch:
// folded into one call the prior term's loads get a branch of their own.)
struct WeightTerm {
    typedef uint8_t Row;                          // a weight row: [mp] counts
    static __device__ __forceinline__ size_t row_elems(size_t mp) { return mp; }
    const uint8_t* row;
    uint32_t w;
    __device__ __forceinline__ explicit WeightTerm(const uint8_t* r) : row(r) {}
    __device__ __forceinline__ bool walks(bool counted, size_t pos, size_t)
    {
        w = counted ? (uint32_t)row[pos] : 0u;
        return w != 0u;
    }
    __device__ __forceinline__ void load(size_t, size_t) {}
    __device__ __forceinline__ void prior(double*, double*) const {}
    __device__ __forceinline__ double value(double lk) const { return (double)w * log(lk); }
};

struct PriorTerm {
    typedef float Row;                            // a hypothesis: three planes [3][mp]
    static __device__ __forceinline__ size_t row_elems(size_t mp) { return 3 * mp; }
    const float* row;
    float h0, h1, h2;
    __device__ __forceinline__ explicit PriorTerm(const float* r) : row(r) {}
    __device__ __forceinline__ bool walks(bool counted, size_t, size_t) const { return counted; }   // no weights
    // the marker's triple: three coalesced floats, in flight under the walk
    __device__ __forceinline__ void load(size_t pos, size_t mp) { h0 = row[pos], h1 = row[mp + pos], h2 = row[2 * mp + pos]; }
    // an all-zero triple carries no information: the anonymous model's term, GF1 at the fixed pc1
    __device__ __forceinline__ void prior(double* G1, double*) const
    {
        const bool given = h0 != 0.0f || h1 != 0.0f || h2 != 0.0f;
        G1[0] = given ? (double)h0 : G1[0];
        G1[1] = given ? (double)h1 : G1[1];
        G1[2] = given ? (double)h2 : G1[2];
    }
    __device__ __forceinline__ double value(double lk) const { return log(lk); }
};

struct PairTerm {
    typedef float Row;                            // a pair hypothesis: six planes [6][mp], pi1[0..2] then pi2[0..2]
    static __device__ __forceinline__ size_t row_elems(size_t mp) { return 6 * mp; }
    const float* row;
    float a0, a1, a2, b0, b1, b2;
    __device__ __forceinline__ explicit PairTerm(const float* r) : row(r) {}
    // a negative pi2[0] leaves the marker out of the hypothesis: read before the marker's record, like a weight
    __device__ __forceinline__ bool walks(bool counted, size_t pos, size_t mp)
    {
        b0 = counted ? row[3 * mp + pos] : -1.0f;
        return !(b0 < 0.0f);
    }
    // the other five floats, coalesced, in flight under the walk
    __device__ __forceinline__ void load(size_t pos, size_t mp)
    {
        a0 = row[pos], a1 = row[mp + pos], a2 = row[2 * mp + pos];
        b1 = row[4 * mp + pos], b2 = row[5 * mp + pos];
    }
    // either side's all-zero triple falls back to its Hardy-Weinberg prior
    __device__ __forceinline__ void prior(double* G1, double* G2) const
    {
        const bool given1 = a0 != 0.0f || a1 != 0.0f || a2 != 0.0f;
        const bool given2 = b0 != 0.0f || b1 != 0.0f || b2 != 0.0f;
        G1[0] = given1 ? (double)a0 : G1[0];
        G1[1] = given1 ? (double)a1 : G1[1];
        G1[2] = given1 ? (double)a2 : G1[2];
        G2[0] = given2 ? (double)b0 : G2[0];
        G2[1] = given2 ? (double)b1 : G2[1];
        G2[2] = given2 ? (double)b2 : G2[2];
    }
    __device__ __forceinline__ double value(double lk) const { return log(lk); }
};

template <class Term, bool PD, int K>
__global__ void __launch_bounds__(kThreads)
llk_sum_marker_kernel(const DeviceLayout L, const double* __restrict__ points, const int32_t* __restrict__ row_of,
                      const typename Term::Row* __restrict__ rows, double* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];      // [nrow][6 pairs], then the tree's [256]
    const int tid = threadIdx.x;
    const int pt = (int)blockIdx.y, bx = (int)blockIdx.x, nbx = (int)gridDim.x;
    const int k = K ? K : L.num_pc, stride = 2 * k + 1;
    const double* prow = points + (size_t)pt * stride;
    const double alpha = prow[2 * k];
    const int nrow = L.num_code + 1;
    const size_t mp = (size_t)L.m_pad;
    const typename Term::Row* row = rows + (size_t)row_of[pt] * Term::row_elems(mp);
    double* part = tab + (size_t)nrow * kRowDoubles;

    // ---- the point's table ----
    for (int e = tid; e < num_single<PD>(L) * 6; e += kThreads) {
        const int pi = e / 6, p = e - pi * 6;
        const SingleRec rec = single_rec(L, pi);
        int g1, g2;
        pair_g(p, g1, g2);
        if constexpr (PD) {
            const double v = entry_of(alpha, rec.p_err, g1, g2);
            const int kq = rec.kq(), rstep = rec.rstep();
            double r = v;
            for (int n = 1; n <= kq; ++n) {
                const int row = rec.first + (n - 1) * rstep;
                if (row >= 0 && row < nrow) tab[(size_t)row * kRowDoubles + p] = r;
                r *= v;
            }
        } else {
            if (rec.alt()) { g1 = 2 - g1; g2 = 2 - g2; }
            const double lv = log(entry_of(alpha, fabs(rec.p_err), g1, g2));
            if (rec.first < nrow) tab[(size_t)rec.first * kRowDoubles + p] = lv;
            if (rec.has_twin() && rec.twin < nrow) tab[(size_t)rec.twin * kRowDoubles + (5 - p)] = lv;
        }
    }
    for (int e = tid; e < kRowDoubles; e += kThreads)           // padding row: P = 1 (log domain: 0)
        tab[(size_t)L.num_code * kRowDoubles + e] = PD ? 1.0 : 0.0;
    if constexpr (PD)
        for_each_window<6>(L, nrow, tid, [&](uint32_t ra, uint32_t rb, uint32_t dst, int p) {
            tab[(size_t)dst * kRowDoubles + p] = tab[(size_t)ra * kRowDoubles + p] * tab[(size_t)rb * kRowDoubles + p];
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
        Term term(row);
        if (term.walks(mt < L.num_mt && pos < (size_t)L.num_active, pos, mp)) {
            const uint2 rec = L.mt_rec[mt];
            term.load(pos, mp);
            double acc[6];
            for (int p = 0; p < 6; ++p) acc[p] = PD ? 1.0 : L.ediag[pos];       // log domain: c_other, summed here
            for_each_step<PD, kRowDoubles>(L, tab, nrow, rec, m, [&](const double* t, bool alt, double n) {
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    if constexpr (PD) acc[p] *= t[alt ? 5 - p : p];
                    else acc[p] = fma(n, t[p], acc[p]);
                }
            });
            // ---- epilogue: L = G1' W GF2, the diagonal of W the context's constants (L as the evaluation kernels define it) ----
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
            term.prior(G1, G2);
            const double cst = PD ? L.ediag[pos] : 0.0;
            for (int g = 0; g < 3; ++g) W[g][g] = L.ediag[(size_t)(1 + g) * mp + pos];
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                int g1, g2;
                pair_g(p, g1, g2);
                W[g1][g2] = PD ? cst * acc[p] : exp(acc[p]);
            }
            // (written out, not mix_of of marker_walk.h: through it the prior term's probability-domain kernels take 76 VGPRs
            // instead of 74)
            double lk = 0.0;
            for (int g1 = 0; g1 < 3; ++g1)
                for (int g2 = 0; g2 < 3; ++g2) lk += W[g1][g2] * G1[g1] * G2[g2];
            if (lk > 0) val = term.value(lk);
        }
        part[tid] = val;
        tree_sum(part, tid);
        if (tid == 0) partial[(size_t)pt * ntile_grp + tg] = part[0];
        __syncthreads();                                        // part[] is written again in the next round
    }
}

__global__ void __launch_bounds__(kThreads)
llk_sum_reduce_kernel(const double* __restrict__ partial, int ntile_grp, double* __restrict__ out)
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

// one thread per (replicate, sorted position)
__global__ void __launch_bounds__(kThreads)
weights_permute_kernel(const uint8_t* __restrict__ panel, const int32_t* __restrict__ pidx, uint8_t* __restrict__ sorted,
                       int num_marker, long long num_active, long long m_pad)
{
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pos >= m_pad) return;
    const size_t r = blockIdx.y;
    uint8_t w = 0;
    if (pos < num_active) {
        const int32_t i = pidx[pos];
        if (i >= 0 && i < num_marker) w = panel[r * (size_t)num_marker + (size_t)i];
    }
    sorted[r * (size_t)m_pad + (size_t)pos] = w;
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

// one thread per (hypothesis, sorted position): rows [M][6] of the panel order into six planes
__global__ void __launch_bounds__(kThreads)
pair_permute_kernel(const float* __restrict__ panel, const int32_t* __restrict__ pidx, float* __restrict__ planes,
                    int num_marker, long long num_active, long long m_pad)
{
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pos >= m_pad) return;
    const size_t h = blockIdx.y;
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (pos < num_active) {
        const int32_t i = pidx[pos];
        if (i >= 0 && i < num_marker) {
            const float* src = panel + (h * (size_t)num_marker + (size_t)i) * 6;
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = src[j];
        }
    }
    float* dst = planes + h * 6 * (size_t)m_pad + (size_t)pos;
#pragma unroll
    for (int j = 0; j < 6; ++j) dst[(size_t)j * (size_t)m_pad] = v[j];
}

// one thread per sorted position of ONE hypothesis: the q plane [M][3] of a source set's row under the paired rule -- pi1
// all zero; pi2 = q where the triple is not all zero and max(q[0], q[2]) >= hom_min; every other marker left out (-1, 0, 0)
__global__ void __launch_bounds__(kThreads)
pair_build_kernel(const float* __restrict__ q, const int32_t* __restrict__ pidx, float* __restrict__ planes, int num_marker,
                  long long num_active, long long m_pad, double hom_min)
{
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pos >= m_pad) return;
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    if (pos < num_active) {
        b0 = -1.0f;
        const int32_t i = pidx[pos];
        if (i >= 0 && i < num_marker) {
            const float* src = q + (size_t)i * 3;
            const float q0 = src[0], q1 = src[1], q2 = src[2];
            const bool counted = q0 != 0.0f || q1 != 0.0f || q2 != 0.0f;
            if (counted && (double)(q0 > q2 ? q0 : q2) >= hom_min) { b0 = q0; b1 = q1; b2 = q2; }
        }
    }
    const size_t mp = (size_t)m_pad;
    float* dst = planes + (size_t)pos;
    dst[0] = 0.0f; dst[mp] = 0.0f; dst[2 * mp] = 0.0f;
    dst[3 * mp] = b0; dst[4 * mp] = b1; dst[5 * mp] = b2;
}

template <class Term, bool PD, int K>
void launch_marker(const DeviceLayout& L, dim3 grid, size_t shmem, hipStream_t stream, const double* d_points,
                   const int32_t* d_row_of, const typename Term::Row* d_rows, double* d_partial)
{
    hipLaunchKernelGGL((llk_sum_marker_kernel<Term, PD, K>), grid, dim3(kThreads), shmem, stream, L, d_points, d_row_of, d_rows,
                       d_partial);
}

// the launch pair of either term: the marker kernel over stripes of tile groups, then a point's fixed-order sum
template <class Term>
hipError_t launch_llk_sum(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_row_of,
                          const typename Term::Row* d_rows, double* d_partial, double* d_out, hipStream_t stream)
{
    if (num_point <= 0) return hipSuccess;
    if (num_point > kMaxPointsPerLaunch) return hipErrorInvalidValue;
    const int nrow = L.num_code + 1;
    const size_t shmem = ((size_t)nrow * kRowDoubles + kThreads) * sizeof(double);
    if (shmem > 64 * 1024) return hipErrorInvalidValue;      // (at most 189 rows of 6 doubles and the tree: 11 KiB)
    const int ntile_grp = tile_groups(L);
    if (ntile_grp > 0) {
        const dim3 grid((unsigned)stripe_grid(L, num_point), (unsigned)num_point);
        const int ksel = L.known_af ? 0 : (L.num_pc == 2 || L.num_pc == 4) ? L.num_pc : 0;
        if (L.pd) {
            if (ksel == 2) launch_marker<Term, true, 2>(L, grid, shmem, stream, d_points, d_row_of, d_rows, d_partial);
            else if (ksel == 4) launch_marker<Term, true, 4>(L, grid, shmem, stream, d_points, d_row_of, d_rows, d_partial);
            else launch_marker<Term, true, 0>(L, grid, shmem, stream, d_points, d_row_of, d_rows, d_partial);
        } else {
            if (ksel == 2) launch_marker<Term, false, 2>(L, grid, shmem, stream, d_points, d_row_of, d_rows, d_partial);
            else if (ksel == 4) launch_marker<Term, false, 4>(L, grid, shmem, stream, d_points, d_row_of, d_rows, d_partial);
            else launch_marker<Term, false, 0>(L, grid, shmem, stream, d_points, d_row_of, d_rows, d_partial);
        }
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(llk_sum_reduce_kernel, dim3((unsigned)num_point), dim3(kThreads), 0, stream, d_partial, ntile_grp, d_out);
    return hipGetLastError();
}

// rows of the panel order into the sorted order: one thread per (row, sorted position)
template <class Kernel, class T>
hipError_t launch_permute(Kernel kernel, const DeviceLayout& L, int num_marker, int num_row, const T* d_panel,
                          const int32_t* d_pidx, T* d_sorted, hipStream_t stream)
{
    if (num_row <= 0 || L.m_pad <= 0) return hipSuccess;
    if (num_row > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((L.m_pad + kThreads - 1) / kThreads), (unsigned)num_row);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, d_panel, d_pidx, d_sorted, num_marker, (long long)L.num_active,
                       (long long)L.m_pad);
    return hipGetLastError();
}

}  // namespace

int marker_sum_tile_groups(const DeviceLayout& L) { return tile_groups(L); }

hipError_t launch_weights_permute(const DeviceLayout& L, int num_marker, int num_rep, const uint8_t* d_panel,
                                  const int32_t* d_pidx, uint8_t* d_sorted, hipStream_t stream)
{
    return launch_permute(weights_permute_kernel, L, num_marker, num_rep, d_panel, d_pidx, d_sorted, stream);
}

hipError_t launch_prior_permute(const DeviceLayout& L, int num_marker, int num_hyp, const float* d_panel, const int32_t* d_pidx,
                                float* d_planes, hipStream_t stream)
{
    return launch_permute(prior_permute_kernel, L, num_marker, num_hyp, d_panel, d_pidx, d_planes, stream);
}

hipError_t launch_llk_weighted(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_row,
                               const uint8_t* d_weights, double* d_partial, double* d_out, hipStream_t stream)
{
    return launch_llk_sum<WeightTerm>(L, num_point, d_points, d_row, d_weights, d_partial, d_out, stream);
}

hipError_t launch_llk_conditioned(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_hyp,
                                  const float* d_planes, double* d_partial, double* d_out, hipStream_t stream)
{
    return launch_llk_sum<PriorTerm>(L, num_point, d_points, d_hyp, d_planes, d_partial, d_out, stream);
}

hipError_t launch_pair_permute(const DeviceLayout& L, int num_marker, int num_hyp, const float* d_panel, const int32_t* d_pidx,
                               float* d_planes, hipStream_t stream)
{
    return launch_permute(pair_permute_kernel, L, num_marker, num_hyp, d_panel, d_pidx, d_planes, stream);
}

hipError_t launch_pair_build(const DeviceLayout& L, int num_marker, const float* d_q, const int32_t* d_pidx, double hom_min,
                             float* d_planes, hipStream_t stream)
{
    if (L.m_pad <= 0) return hipSuccess;
    const dim3 grid((unsigned)((L.m_pad + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(pair_build_kernel, grid, dim3(kThreads), 0, stream, d_q, d_pidx, d_planes, num_marker,
                       (long long)L.num_active, (long long)L.m_pad, hom_min);
    return hipGetLastError();
}

hipError_t launch_llk_paired(const DeviceLayout& L, int num_point, const double* d_points, const int32_t* d_hyp,
                             const float* d_planes, double* d_partial, double* d_out, hipStream_t stream)
{
    return launch_llk_sum<PairTerm>(L, num_point, d_points, d_hyp, d_planes, d_partial, d_out, stream);
}

}  // namespace vb2
