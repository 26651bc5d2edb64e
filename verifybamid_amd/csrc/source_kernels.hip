// source_kernels.hip -- gfx950 kernels behind --FindSource: which sample of a cohort does a
// sample's contamination come from?
//
//   * source_marginal_kernel: at one point (pc1, pc2, alpha) it forms, per marker, the 3x3 matrix W[g1][g2] = prod_reads
//     P(read | g1, g2, alpha) exactly as llk_derivs_marker_kernel does -- the point's table in LDS (values only), one thread
//     per marker walking the context's own run words or steps (llk_kernels.h: DeviceLayout), no second copy of the reads
//     -- and from it, in FP64,
//         L     = sum GF1[g1] GF2[g2] W[g1][g2]
//         c[g1] = (sum_g2 W[g1][g2] GF2[g2]) / L          the contaminant's genotype likelihood, relative to a random one
//         q[g2] = GF2[g2] (sum_g1 GF1[g1] W[g1][g2]) / L  the posterior of the sample's own genotype
//     written in PANEL order through the sort permutation: doubles for vb2_ctx_marginals, float32 rows for a source set.
//     In the log domain W is taken relative to the largest exponent before exp (the derivative kernel's `scale`); in the
//     probability domain the products start at 2^900 (kPdScale).  Markers a thousand reads deep keep their ratios.
//   * source_pair_kernel: S(i, j) = sum_m log max(c_i[m] . q_j[m], 1e-30) over the markers both samples count.  A
//     workgroup takes 16 targets x 16 candidates x one stripe of kPairStripe markers; both sides' triples go through LDS
//     64 markers at a time; one thread per pair forms the three-term dot in FP32, takes its logarithm (v_log_f32 inside
//     __logf) and accumulates in FP64, marker after marker.  source_reduce_kernel adds a pair's stripes in stripe order.
//     No atomics: a pair's score is the same bits from call to call and whatever else the set holds.
#include "source_kernels.h"

#include "marker_walk.h"

namespace vb2 {
namespace {

using namespace walk;

// a table row: the six off-diagonal pairs, then the three diagonal pairs (g, g), whose p = u_g whatever alpha -- P^n in the
// probability domain, log p in the log domain.  The context's own diagonal constants exp(c_other + D[g]) are good enough
// for L itself but are subnormal or 0 on deep markers: no basis for the ratios W / L.
constexpr int kRowDoubles = 9;
// Probability domain: the running products start at 2^900 instead of 1.  A context takes that layout only while no
// marker's (het, het) term can fall below 2^-900 (llk_kernels.h: kPdMaxBound), so the largest of the nine products stays
// >= 1 and a product 2^-1000 of it is still a normal double; started at 1, such entries are subnormal and their few bits
// reach q (measured: 1.2e-4 relative on a marker 400 reads deep).  c_other, common to the nine, cancels in the ratios.
constexpr double kPdScale = 0x1p900, kPdUnscale = 0x1p-900;

// REL (--FindRelated): the epilogue also forms h = q / GF2, the sample's own-genotype likelihood
// relative to a random individual, and t = q T_p, the genotype distribution of a relative who shares one allele identical by
// descent (p: the clamped allele frequency GF2 is formed from); the float32 planes then go where `rel` says, not to `row`.
template <bool PD, bool REL>
__global__ void __launch_bounds__(kThreads)
source_marginal_kernel(const DeviceLayout L, const int num_marker, const double* __restrict__ point,
                       const int32_t* __restrict__ pidx, double* __restrict__ contam_lik, double* __restrict__ geno_post,
                       double* __restrict__ log_l, float* __restrict__ row, const MarginalRelated rel)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];      // [nrow][kRowDoubles]
    const int tid = threadIdx.x;
    const int k = L.num_pc;
    const double alpha = point[2 * k];
    const int nrow = L.num_code + 1;
    const size_t mp = (size_t)L.m_pad;

    // ---- the point's table (deriv_kernels.hip, values only) ----
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
                const int rw = rec.first + (n - 1) * rstep;
                if (rw >= 0 && rw < nrow) tab[(size_t)rw * kRowDoubles + p] = r;
                r *= v;
            }
        } else {
            if (rec.alt()) { g1 = 2 - g1; g2 = 2 - g2; }
            const double lv = log(entry_of(alpha, fabs(rec.p_err), g1, g2));
            if (rec.first < nrow) tab[(size_t)rec.first * kRowDoubles + p] = lv;
            if (rec.has_twin() && rec.twin < nrow) tab[(size_t)rec.twin * kRowDoubles + (5 - p)] = lv;
        }
    }
    // the diagonal pairs: p = u_g whatever alpha; an alt code (log domain) or step (probability domain) reads the genotype mirrored
    for (int e = tid; e < num_single<PD>(L) * 3; e += kThreads) {
        const int pi = e / 3, g = e - pi * 3;
        const SingleRec rec = single_rec(L, pi);
        const double u = diag_entry_of(fabs(rec.p_err), g);
        if constexpr (PD) {
            const int kq = rec.kq(), rstep = rec.rstep();
            double r = u;
            for (int n = 1; n <= kq; ++n) {
                const int rw = rec.first + (n - 1) * rstep;
                if (rw >= 0 && rw < nrow) tab[(size_t)rw * kRowDoubles + 6 + g] = r;
                r *= u;
            }
        } else {
            const double lu = log(u);
            if (rec.first < nrow) tab[(size_t)rec.first * kRowDoubles + 6 + (rec.alt() ? 2 - g : g)] = lu;
            if (rec.has_twin() && rec.twin < nrow) tab[(size_t)rec.twin * kRowDoubles + 6 + (2 - g)] = lu;
        }
    }
    for (int e = tid; e < kRowDoubles; e += kThreads)           // padding row: P = 1 (log domain: 0)
        tab[(size_t)L.num_code * kRowDoubles + e] = PD ? 1.0 : 0.0;
    if constexpr (PD)
        for_each_window<kRowDoubles>(L, nrow, tid, [&](uint32_t ra, uint32_t rb, uint32_t dst, int p) {
            tab[(size_t)dst * kRowDoubles + p] = tab[(size_t)ra * kRowDoubles + p] * tab[(size_t)rb * kRowDoubles + p];
        });
    __syncthreads();

    // ---- one thread per marker of the sorted order ----
    const int m = tid & 15;
    const int ntile_grp = tile_groups(L);
    for (int tg = blockIdx.x; tg < ntile_grp; tg += gridDim.x) {
        const int mt = tg * 16 + (tid >> 4);
        if (mt >= L.num_mt) continue;
        const size_t pos = (size_t)mt * 16 + (size_t)m;
        if (pos >= (size_t)L.num_active) continue;
        const int32_t pm = pidx[pos];
        if (pm < 0 || pm >= num_marker) continue;
        const uint2 rec = L.mt_rec[mt];
        double acc[6], dacc[3];
        for (int p = 0; p < 6; ++p) acc[p] = PD ? kPdScale : L.ediag[pos];
        for (int g = 0; g < 3; ++g) dacc[g] = PD ? kPdScale : L.ediag[pos];     // (log domain: c_other + the sums)
        for_each_step<PD, kRowDoubles>(L, tab, nrow, rec, m, [&](const double* t, bool alt, double n) {
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                if constexpr (PD) acc[p] *= t[alt ? 5 - p : p];
                else acc[p] = fma(n, t[p], acc[p]);
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                if constexpr (PD) dacc[g] *= t[6 + (alt ? 2 - g : g)];
                else dacc[g] = fma(n, t[6 + g], dacc[g]);
            }
        });
        // ---- epilogue ----
        double af1, af2;
        if (L.known_af != nullptr) {
            af1 = af2 = L.known_af[pos];
        } else {
            af1 = 0.0; af2 = 0.0;
            for (int kk = 0; kk < k; ++kk) {
                const double u = L.ud[(size_t)kk * mp + pos];
                af1 = fma(u, point[kk], af1);
                af2 = fma(u, point[k + kk], af2);
            }
            const double mu = L.mu[pos];
            af1 += mu; af1 /= 2.0;
            af2 += mu; af2 /= 2.0;
        }
        double G1[3], G2[3];
        gf_of(af1, G1);
        gf_of(af2, G2);
        double W[3][3], Wu[3][3];       // W: relative to exp(scale); Wu: as the evaluation kernels see it (decides L > 0, gives log L)
        const double cst = PD ? L.ediag[pos] : 0.0;
        for (int g = 0; g < 3; ++g) Wu[g][g] = W[g][g] = L.ediag[(size_t)(1 + g) * mp + pos];
        double scale = 0.0;
        if constexpr (!PD) {
            double amax = -__builtin_huge_val();
            for (int p = 0; p < 6; ++p) amax = acc[p] > amax ? acc[p] : amax;
            for (int g = 0; g < 3; ++g) amax = dacc[g] > amax ? dacc[g] : amax;
            scale = amax > -__builtin_huge_val() && amax < __builtin_huge_val() ? amax : 0.0;
            for (int g = 0; g < 3; ++g) W[g][g] = exp(dacc[g] - scale);
        } else {
            for (int g = 0; g < 3; ++g) W[g][g] = dacc[g];
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            int g1, g2;
            pair_g(p, g1, g2);
            if constexpr (PD) {
                W[g1][g2] = acc[p];
                Wu[g1][g2] = cst * (acc[p] * kPdUnscale);       // (a power of two: the bits of the product started at 1)
            } else {
                Wu[g1][g2] = exp(acc[p]);
                W[g1][g2] = exp(acc[p] - scale);
            }
        }
        const double lk = mix_of(Wu, G1, G2);         // L itself, in the reference's order
        if (!(lk > 0)) continue;
        double r0[3], c0[3], Ls = 0.0;
        for (int a = 0; a < 3; ++a) {
            r0[a] = 0.0;
            c0[a] = 0.0;
            for (int b = 0; b < 3; ++b) {
                r0[a] += W[a][b] * G2[b];
                c0[a] += G1[b] * W[b][a];
            }
        }
        for (int a = 0; a < 3; ++a) Ls += G1[a] * r0[a];
        if (!(Ls > 0)) continue;
        const size_t pm3 = (size_t)pm * 3;
        if constexpr (REL) {
            double qq[3], hh[3], tt[3];
            for (int g = 0; g < 3; ++g) {
                const double c = r0[g] / Ls;
                hh[g] = c0[g] / Ls;
                qq[g] = G2[g] * c0[g] / Ls;                                // (the expression of the other instantiation)
                if (contam_lik) contam_lik[pm3 + g] = c;
                if (geno_post) geno_post[pm3 + g] = qq[g];
                if (rel.c) rel.c[pm3 + g] = (float)c;
                if (rel.q) rel.q[pm3 + g] = (float)qq[g];
            }
            // rows of T_p: (1 - p, p, 0), ((1 - p) / 2, 1 / 2, p / 2), (0, 1 - p, p)
            const double p = clamp_af(af2), np = 1 - p;
            tt[0] = qq[0] * np + qq[1] * (0.5 * np);
            tt[1] = qq[0] * p + qq[1] * 0.5 + qq[2] * np;
            tt[2] = qq[1] * (0.5 * p) + qq[2] * p;
            for (int g = 0; g < 3; ++g) {
                if (rel.own_lik) rel.own_lik[pm3 + g] = hh[g];
                if (rel.kin_post) rel.kin_post[pm3 + g] = tt[g];
                if (rel.h) rel.h[pm3 + g] = (float)hh[g];
                if (rel.t) rel.t[pm3 + g] = (float)tt[g];
            }
        } else {
            for (int g = 0; g < 3; ++g) {
                const double c = r0[g] / Ls, q = G2[g] * c0[g] / Ls;
                if (contam_lik) contam_lik[pm3 + g] = c;
                if (geno_post) geno_post[pm3 + g] = q;
                if (row) {
                    row[pm3 + g] = (float)c;                                   // round to nearest
                    row[(size_t)num_marker * 3 + pm3 + g] = (float)q;
                }
            }
        }
        if (log_l) log_l[pm] = log(lk);
    }
}

// S(i, j) over one stripe of markers for a 16 x 16 tile of pairs
__global__ void __launch_bounds__(kThreads)
source_pair_kernel(const float* const* __restrict__ rows, const int n, const long long num_marker, double* __restrict__ part_s,
                   int32_t* __restrict__ part_n)
{
    // [marker of the chunk][component][sample, padded to 17: the staging writes of one sample's consecutive floats then
    // fall into different banks]; a wave reads 16 consecutive q's (its candidates) and 4 c's (its targets, broadcast)
    constexpr int kPad = kPairTile + 1;
    __shared__ float sc[kPairChunk * 3 * kPad];
    __shared__ float sq[kPairChunk * 3 * kPad];
    const int tid = threadIdx.x;
    const int tj = tid & (kPairTile - 1), ti = tid >> 4;
    const int i0 = blockIdx.y * kPairTile, j0 = blockIdx.x * kPairTile;
    const long long m_begin = (long long)blockIdx.z * kPairStripe;
    const long long m_end = m_begin + kPairStripe < num_marker ? m_begin + kPairStripe : num_marker;
    const size_t qplane = (size_t)num_marker * 3;
    double acc = 0.0;
    int cnt = 0;
    for (long long mc = m_begin; mc < m_end; mc += kPairChunk) {
        const int valid = (int)(m_end - mc < kPairChunk ? m_end - mc : kPairChunk) * 3;     // floats of a sample in this chunk
        __syncthreads();
        for (int e = tid; e < kPairTile * kPairChunk * 3; e += kThreads) {
            const int s = e / (kPairChunk * 3), r = e - s * (kPairChunk * 3);
            float c = 0.0f, q = 0.0f;
            if (r < valid) {
                const float* ri = i0 + s < n ? rows[i0 + s] : nullptr;
                const float* rj = j0 + s < n ? rows[j0 + s] : nullptr;
                if (ri) c = ri[(size_t)mc * 3 + (size_t)r];
                if (rj) q = rj[qplane + (size_t)mc * 3 + (size_t)r];
            }
            sc[r * kPad + s] = c;
            sq[r * kPad + s] = q;
        }
        __syncthreads();
        const int nm = valid / 3;
        for (int mm = 0; mm < nm; ++mm) {
            const float* pc = sc + mm * 3 * kPad + ti;
            const float* pq = sq + mm * 3 * kPad + tj;
            const float c0 = pc[0], c1 = pc[kPad], c2 = pc[2 * kPad];
            const float q0 = pq[0], q1 = pq[kPad], q2 = pq[2 * kPad];
            // a counted marker has a non-zero triple (sum GF1 c = 1, sum q = 1); the triples are non-negative
            const bool both = (c0 + c1 + c2 > 0.0f) && (q0 + q1 + q2 > 0.0f);
            float d = fmaf(c2, q2, fmaf(c1, q1, c0 * q0));
            d = d > kSourceDotFloor ? d : kSourceDotFloor;
            const float lg = __logf(d);
            if (both) {
                acc += (double)lg;
                ++cnt;
            }
        }
    }
    const int i = i0 + ti, j = j0 + tj;
    if (i < n && j < n) {
        const size_t at = ((size_t)blockIdx.z * (size_t)n + (size_t)i) * (size_t)n + (size_t)j;
        part_s[at] = acc;
        part_n[at] = cnt;
    }
}

__global__ void __launch_bounds__(kThreads)
source_reduce_kernel(const float* const* __restrict__ rows, const int n, const int num_stripe, const double* __restrict__ part_s,
                     const int32_t* __restrict__ part_n, double* __restrict__ score, int32_t* __restrict__ shared)
{
    const size_t nn = (size_t)n * (size_t)n;
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= nn) return;
    const int i = (int)(at / (size_t)n), j = (int)(at - (size_t)i * (size_t)n);
    double s = 0.0;
    int c = 0;
    for (int z = 0; z < num_stripe; ++z) {        // stripe order: fixed
        s += part_s[(size_t)z * nn + at];
        c += part_n[(size_t)z * nn + at];
    }
    const bool none = i == j || rows[i] == nullptr || rows[j] == nullptr;
    score[at] = none ? __builtin_nan("") : s;
    shared[at] = none ? 0 : c;
}

}  // namespace

hipError_t launch_source_marginals(const DeviceLayout& L, int num_marker, const double* d_point, const int32_t* pidx,
                                   double* contam_lik, double* geno_post, double* log_l, float* row, hipStream_t stream)
{
    if (L.num_mt <= 0 || L.num_active <= 0) return hipSuccess;
    const int nrow = L.num_code + 1;
    const size_t shmem = (size_t)nrow * kRowDoubles * sizeof(double);
    const dim3 grid((unsigned)stripe_grid(L, 1)), block(kThreads);
    const MarginalRelated none{};
    if (L.pd)
        hipLaunchKernelGGL((source_marginal_kernel<true, false>), grid, block, shmem, stream, L, num_marker, d_point, pidx,
                           contam_lik, geno_post, log_l, row, none);
    else
        hipLaunchKernelGGL((source_marginal_kernel<false, false>), grid, block, shmem, stream, L, num_marker, d_point, pidx,
                           contam_lik, geno_post, log_l, row, none);
    return hipGetLastError();
}

hipError_t launch_related_marginals(const DeviceLayout& L, int num_marker, const double* d_point, const int32_t* pidx,
                                    double* contam_lik, double* geno_post, double* log_l, const MarginalRelated& rel,
                                    hipStream_t stream)
{
    if (L.num_mt <= 0 || L.num_active <= 0) return hipSuccess;
    const int nrow = L.num_code + 1;
    const size_t shmem = (size_t)nrow * kRowDoubles * sizeof(double);
    const dim3 grid((unsigned)stripe_grid(L, 1)), block(kThreads);
    if (L.pd)
        hipLaunchKernelGGL((source_marginal_kernel<true, true>), grid, block, shmem, stream, L, num_marker, d_point, pidx,
                           contam_lik, geno_post, log_l, nullptr, rel);
    else
        hipLaunchKernelGGL((source_marginal_kernel<false, true>), grid, block, shmem, stream, L, num_marker, d_point, pidx,
                           contam_lik, geno_post, log_l, nullptr, rel);
    return hipGetLastError();
}

hipError_t launch_source_pairs(const float* const* d_rows, int n, int64_t num_marker, double* part_s, int32_t* part_n,
                               double* score, int32_t* shared, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int nt = (n + kPairTile - 1) / kPairTile;
    const int ns = source_num_stripe(num_marker);
    if (ns > 65535 || nt > 65535) return hipErrorInvalidValue;
    if (ns > 0) {
        const dim3 grid((unsigned)nt, (unsigned)nt, (unsigned)ns), block(kThreads);
        hipLaunchKernelGGL(source_pair_kernel, grid, block, 0, stream, d_rows, n, (long long)num_marker, part_s, part_n);
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    const size_t nn = (size_t)n * (size_t)n;
    const dim3 rgrid((unsigned)((nn + kThreads - 1) / kThreads)), block(kThreads);
    hipLaunchKernelGGL(source_reduce_kernel, rgrid, block, 0, stream, d_rows, n, ns, part_s, part_n, score, shared);
    return hipGetLastError();
}

}  // namespace vb2
