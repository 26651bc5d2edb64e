// deriv_kernels.hip -- gfx950 kernels for the gradient and Hessian of the genotype-mixture log-likelihood
// (FullLLKFunc::ComputeMixLLKs, ContaminationEstimator.h:194-314) with respect to (pc1[0..k), pc2[0..k), alpha).
// DESIGN.md section 10 has the math; this file walks the layouts the context already holds (llk_kernels.h: DeviceLayout),
// in both forms, and makes no second copy of the reads.
//
//   * llk_derivs_marker_kernel: one workgroup per (stripe of micro-tiles, point).  It builds the point's derivative table
//     in LDS -- per table row and off-diagonal genotype pair {value, d, d^2} with d = dp/dalpha / p -- and one thread per
//     marker walks the marker's runs (log domain: value = log p, a run of n reads adds n x each entry) or steps
//     (probability domain: value = P^n, the row carries n d and n d^2; window rows the sums of their factors').  In the
//     log domain a row also carries log u_g of the three diagonal pairs: the context's diagonal constants are
//     probabilities, exp(c_other + D[g]), which past ~1 000 reads are subnormal doubles with few bits left (or 0) --
//     good enough for L itself, whose value the reference defines that way, but not for the ratios W / L.  The
//     epilogue forms the marker's nine derivatives of L = GF1' W GF2 and writes them with log L to the scratch
//     [point][kDerivVals][m_pad].
//   * llk_derivs_reduce_kernel: one workgroup per (output, point) sums a scalar over the markers with the sorted panel
//     rows (AF = (UD pc + mu) / 2: the chain rule), in a fixed order -- thread t takes positions t, t + 256, ..., then a
//     fixed tree.  A point's results are the same bits whatever else the batch holds and from one call to the next.
//   * llk_derivs_marker_multi_kernel / llk_derivs_reduce_multi_kernel: the same two bodies for the points of SEVERAL samples
//     in one launch pair (Batch::derivs), each workgroup reading its sample's layout through a job table in device memory.
//     A point's results are the single-sample kernels' bits.
//   * llk_pair_derivs_marker_kernel / llk_pair_derivs_marker_multi_kernel: the marker body given a pair hypothesis (DESIGN.md
//     sections 16 and 17), its Prior template parameter a PairPrior: a marker the hypothesis leaves out is not walked, and a
//     side with a prior at a marker is (pi, 0, 0) there.  The anonymous kernels are the body under HardyWeinberg, which
//     compiles to nothing.  The reduction kernels serve both.
#include "deriv_kernels.h"

#include "marker_walk.h"

namespace vb2 {
namespace {

using namespace walk;

constexpr int kEntry = 3;                         // {value, d, d^2} per (row, pair)
constexpr int kPairDoubles = 6 * kEntry;
constexpr int kRowDoublesPd = kPairDoubles;       // probability domain: the six off-diagonal pairs
constexpr int kRowDoublesLog = kPairDoubles + 3;  // log domain: and log u_g of the diagonal pairs (g, g)

// entry_of and d = (u_g1 - u_g2) / p = dp/dalpha / p, 0 where p = 0
__device__ __forceinline__ void entry_d_of(double alpha, double p_err, int g1, int g2, double& p, double& d)
{
    p = entry_of(alpha, p_err, g1, g2);
    d = p != 0.0 ? (diag_entry_of(p_err, g1) - diag_entry_of(p_err, g2)) / p : 0.0;
}

// GF (h:186-192) and its first two derivatives in AF; both 0 where the reference clamps AF (the branch it takes)
__device__ __forceinline__ void gf_derivs(double af, bool fixed, double* gf, double* d1, double* d2)
{
    const bool clamped = af < kMinAf || af > kMaxAf || fixed;
    af = clamp_af(af);
    gf_of(af, gf);
    d1[0] = clamped ? 0.0 : -2.0 * (1.0 - af);
    d1[1] = clamped ? 0.0 : 2.0 - 4.0 * af;
    d1[2] = clamped ? 0.0 : 2.0 * af;
    d2[0] = clamped ? 0.0 : 2.0;
    d2[1] = clamped ? 0.0 : -4.0;
    d2[2] = clamped ? 0.0 : 2.0;
}

// A Prior: what a marker's genotype priors are, a small struct the body makes per marker from the planes of the point's
// hypothesis and holds by value (the Term of marker_sum_kernels.hip, for the derivatives).  walks() -- false: the marker is
// left out, not walked, and contributes ten zeros -- is asked before the marker's record is read; apply(), in the
// epilogue, may replace a side's {GF, GF', GF''}.
struct HardyWeinberg {                            // the anonymous model: GF1(pc1), GF2(pc2) at every marker
    __device__ __forceinline__ explicit HardyWeinberg(const float*) {}
    __device__ __forceinline__ bool walks(size_t, size_t) const { return true; }
    __device__ __forceinline__ void apply(size_t, size_t, double*, double*, double*, double*, double*, double*) const {}
};

// A pair hypothesis (DESIGN.md sections 16 and 17): six planes [6][mp], pi1[0..2] then pi2[0..2], as PairTerm reads them.
struct PairPrior {
    const float* row;
    float b0;
    __device__ __forceinline__ explicit PairPrior(const float* r) : row(r) {}
    // a negative pi2[0] leaves the marker out of the hypothesis: read before the marker's record
    __device__ __forceinline__ bool walks(size_t pos, size_t mp)
    {
        b0 = row[3 * mp + pos];
        return !(b0 < 0.0f);
    }
    // The other five floats are loaded here, behind the walk: only the epilogue needs them, and the probability-domain
    // kernels have no registers to keep them live across it.  A triple that is not all zero stands in for that side's
    // Hardy-Weinberg prior, and nothing at the marker depends on that side's PCs any more: (pi, 0, 0).  The float32 values
    // widened to double, exactly as PairTerm::prior() uses them.
    __device__ __forceinline__ void apply(size_t pos, size_t mp, double* G1, double* G1d, double* G1dd, double* G2, double* G2d,
                                          double* G2dd) const
    {
        const float a0 = row[pos], a1 = row[mp + pos], a2 = row[2 * mp + pos];
        const float b1 = row[4 * mp + pos], b2 = row[5 * mp + pos];
        const bool given1 = a0 != 0.0f || a1 != 0.0f || a2 != 0.0f;
        const bool given2 = b0 != 0.0f || b1 != 0.0f || b2 != 0.0f;
        G1[0] = given1 ? (double)a0 : G1[0];
        G1[1] = given1 ? (double)a1 : G1[1];
        G1[2] = given1 ? (double)a2 : G1[2];
        G2[0] = given2 ? (double)b0 : G2[0];
        G2[1] = given2 ? (double)b1 : G2[1];
        G2[2] = given2 ? (double)b2 : G2[2];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            G1d[g] = given1 ? 0.0 : G1d[g];
            G1dd[g] = given1 ? 0.0 : G1dd[g];
            G2d[g] = given2 ? 0.0 : G2d[g];
            G2dd[g] = given2 ? 0.0 : G2dd[g];
        }
    }
};

// The body of the marker kernels: point pt of `points`, as workgroup bx of the nbx that share the point's 16-tile groups.
// What a marker's ten scalars are does not depend on bx / nbx, nor on where L was read from.  planes: the hypothesis of a
// PairPrior (HardyWeinberg: not read).
template <bool PD, class Prior>
__device__ __forceinline__ void derivs_marker_body(const DeviceLayout& L, const double* __restrict__ points,
                                                   const float* __restrict__ planes, double* __restrict__ out, double* tab,
                                                   int pt, int bx, int nbx)
{
    constexpr int kRowDoubles = PD ? kRowDoublesPd : kRowDoublesLog;
    const int tid = threadIdx.x;
    const int k = L.num_pc, stride = 2 * k + 1;
    const double* prow = points + (size_t)pt * stride;
    const double alpha = prow[2 * k];
    const int nrow = L.num_code + 1;
    const size_t mp = (size_t)L.m_pad;

    // ---- the point's table ----
    for (int e = tid; e < num_single<PD>(L) * 6; e += kThreads) {
        const int pi = e / 6, p = e - pi * 6;
        const SingleRec rec = single_rec(L, pi);
        int g1, g2;
        pair_g(p, g1, g2);
        double v, d;
        if constexpr (PD) {
            entry_d_of(alpha, rec.p_err, g1, g2, v, d);
            const int kq = rec.kq(), rstep = rec.rstep();
            double r = v;
            for (int n = 1; n <= kq; ++n) {
                const int row = rec.first + (n - 1) * rstep;
                if (row >= 0 && row < nrow) {
                    double* c = tab + (size_t)row * kRowDoubles + p * kEntry;
                    c[0] = r;
                    c[1] = (double)n * d;
                    c[2] = (double)n * (d * d);
                }
                r *= v;
            }
        } else {
            if (rec.alt()) { g1 = 2 - g1; g2 = 2 - g2; }
            entry_d_of(alpha, fabs(rec.p_err), g1, g2, v, d);
            const double lv = log(v);
            if (rec.first < nrow) {
                double* c = tab + (size_t)rec.first * kRowDoubles + p * kEntry;
                c[0] = lv; c[1] = d; c[2] = d * d;
            }
            if (rec.has_twin() && rec.twin < nrow) {
                double* c = tab + (size_t)rec.twin * kRowDoubles + (5 - p) * kEntry;
                c[0] = lv; c[1] = d; c[2] = d * d;
            }
        }
    }
    if constexpr (!PD) {
        // the diagonal pairs: p = alpha u_g + (1 - alpha) u_g = u_g whatever alpha; an alt code reads the genotype mirrored
        for (int e = tid; e < num_single<PD>(L) * 3; e += kThreads) {
            const int pi = e / 3, g = e - pi * 3;
            const SingleRec rec = single_rec(L, pi);
            const double lu = log(diag_entry_of(fabs(rec.p_err), g));
            if (rec.first < nrow) tab[(size_t)rec.first * kRowDoubles + kPairDoubles + (rec.alt() ? 2 - g : g)] = lu;
            if (rec.has_twin() && rec.twin < nrow) tab[(size_t)rec.twin * kRowDoubles + kPairDoubles + (2 - g)] = lu;
        }
    }
    for (int e = tid; e < kRowDoubles; e += kThreads)           // padding row: P = 1 (log domain: 0), no derivative
        tab[(size_t)L.num_code * kRowDoubles + e] = (PD && e % kEntry == 0) ? 1.0 : 0.0;
    if constexpr (PD)
        // window rows: the value multiplies, d and d^2 add
        for_each_window<6>(L, nrow, tid, [&](uint32_t ra, uint32_t rb, uint32_t dst, int p) {
            const double* a = tab + (size_t)ra * kRowDoubles + p * kEntry;
            const double* b = tab + (size_t)rb * kRowDoubles + p * kEntry;
            double* c = tab + (size_t)dst * kRowDoubles + p * kEntry;
            c[0] = a[0] * b[0];
            c[1] = a[1] + b[1];
            c[2] = a[2] + b[2];
        });
    __syncthreads();

    // ---- one thread per marker of the sorted order ----
    const int m = tid & 15;
    const int ntile_grp = tile_groups(L);
    for (int tg = bx; tg < ntile_grp; tg += nbx) {
        const int mt = tg * 16 + (tid >> 4);
        if (mt >= L.num_mt) continue;
        const size_t pos = (size_t)mt * 16 + (size_t)m;
        double* o = out + (size_t)pt * kDerivVals * mp + pos;
        if (pos >= (size_t)L.num_active) {
            for (int j = 0; j < kDerivVals; ++j) o[(size_t)j * mp] = 0.0;
            continue;
        }
        Prior prior(planes);
        if (!prior.walks(pos, mp)) {
            for (int j = 0; j < kDerivVals; ++j) o[(size_t)j * mp] = 0.0;
            continue;
        }
        const uint2 rec = L.mt_rec[mt];
        double acc[6], a1[6], a2[6], dacc[3];
        for (int p = 0; p < 6; ++p) { acc[p] = PD ? 1.0 : L.ediag[pos]; a1[p] = 0.0; a2[p] = 0.0; }
        for (int g = 0; g < 3; ++g) dacc[g] = PD ? 0.0 : L.ediag[pos];     // log domain: c_other + D[g], summed here
        // The walk is written out here, not for_each_step of marker_walk.h: through it the scheduler issues a step's 18 LDS
        // reads in fewer groups and the probability-domain kernels take 8 more VGPRs (156 -> 164 and 154 -> 162: the last
        // granule that still gives three waves per SIMD).
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
                for (int p = 0; p < 6; ++p) {
                    const double* c = t + (alt ? 5 - p : p) * kEntry;
                    acc[p] *= c[0];
                    a1[p] += c[1];
                    a2[p] += c[2];
                }
            }
        } else {
            // {first row, rows}; a row = two run words, run = row byte offset | top 16 bits of double(count) << 16
            for (uint32_t r = 0; r < rec.y; ++r) {
                const uint2 w = L.codes[((size_t)rec.x + r) * 16 + (size_t)m];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t rw = j ? w.y : w.x;
                    const double n = __hiloint2double((int)(rw & 0xffff0000u), 0);
                    uint32_t row = (rw & 0xffffu) / (uint32_t)L.row_bytes;
                    row = row < (uint32_t)nrow ? row : (uint32_t)L.num_code;
                    const double* t = tab + (size_t)row * kRowDoubles;
#pragma unroll
                    for (int p = 0; p < 6; ++p) {
                        acc[p] = fma(n, t[p * kEntry], acc[p]);
                        a1[p] = fma(n, t[p * kEntry + 1], a1[p]);
                        a2[p] = fma(n, t[p * kEntry + 2], a2[p]);
                    }
#pragma unroll
                    for (int g = 0; g < 3; ++g) dacc[g] = fma(n, t[kPairDoubles + g], dacc[g]);
                }
            }
        }
        // ---- epilogue: W[g1][g2] (diagonal: the context's constants), A' and A'' + A'^2 off the diagonal ----
        double af1, af2;
        const bool kaf = L.known_af != nullptr;
        if (kaf) {
            af1 = af2 = L.known_af[pos];
        } else {
            af1 = 0.0; af2 = 0.0;
            for (int kk = 0; kk < k; ++kk) {
                const double u = L.ud[(size_t)kk * mp + pos];
                af1 = fma(u, prow[kk], af1);
                af2 = fma(u, prow[k + kk], af2);
            }
            const double mu = L.mu[pos];
            af1 += mu; af1 /= 2.0;
            af2 += mu; af2 /= 2.0;
        }
        double G1[3], G1d[3], G1dd[3], G2[3], G2d[3], G2dd[3];
        gf_derivs(af1, kaf, G1, G1d, G1dd);
        gf_derivs(af2, kaf, G2, G2d, G2dd);
        prior.apply(pos, mp, G1, G1d, G1dd, G2, G2d, G2dd);
        double W[3][3], WA[3][3], WB[3][3];
        const double cst = PD ? L.ediag[pos] : 0.0;
        for (int g = 0; g < 3; ++g) { W[g][g] = L.ediag[(size_t)(1 + g) * mp + pos]; WA[g][g] = 0.0; WB[g][g] = 0.0; }
        double lk;               // L itself, in the reference's order (h:307-309): what decides whether the marker counts
        double scale = 0.0;      // log domain: W relative to exp(scale), so that the ratios survive deep markers
        if constexpr (!PD) {
            double amax = -__builtin_huge_val();
            for (int p = 0; p < 6; ++p) amax = acc[p] > amax ? acc[p] : amax;
            for (int g = 0; g < 3; ++g) amax = dacc[g] > amax ? dacc[g] : amax;
            scale = amax > -__builtin_huge_val() && amax < __builtin_huge_val() ? amax : 0.0;
        }
        double Wu[3][3];
        for (int g = 0; g < 3; ++g) Wu[g][g] = W[g][g];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            int g1, g2;
            pair_g(p, g1, g2);
            double wu, ws;
            if constexpr (PD) {
                wu = ws = cst * acc[p];
            } else {
                wu = exp(acc[p]);
                ws = exp(acc[p] - scale);
            }
            Wu[g1][g2] = wu;
            W[g1][g2] = ws;
            WA[g1][g2] = ws * a1[p];
            WB[g1][g2] = ws * (a1[p] * a1[p] - a2[p]);
        }
        if constexpr (!PD)
            for (int g = 0; g < 3; ++g) W[g][g] = exp(dacc[g] - scale);     // (Wu keeps the context's constant: L as evaluated)
        lk = mix_of(Wu, G1, G2);
        double v[kDerivVals];
        for (int j = 0; j < kDerivVals; ++j) v[j] = 0.0;
        if (lk > 0) {
            // rows weighted by GF2 and its derivatives, then the GF1 side
            double r0[3], r1[3], r2[3], s0[3], s1v[3], t0[3];
            for (int a = 0; a < 3; ++a) {
                r0[a] = r1[a] = r2[a] = s0[a] = s1v[a] = t0[a] = 0.0;
                for (int b = 0; b < 3; ++b) {
                    r0[a] += W[a][b] * G2[b];
                    r1[a] += W[a][b] * G2d[b];
                    r2[a] += W[a][b] * G2dd[b];
                    s0[a] += WA[a][b] * G2[b];
                    s1v[a] += WA[a][b] * G2d[b];
                    t0[a] += WB[a][b] * G2[b];
                }
            }
            double Ls = 0, L1 = 0, L2 = 0, L11 = 0, L22 = 0, L12 = 0, La = 0, L1a = 0, L2a = 0, Laa = 0;
            for (int a = 0; a < 3; ++a) {
                Ls += G1[a] * r0[a];
                L1 += G1d[a] * r0[a];
                L11 += G1dd[a] * r0[a];
                L2 += G1[a] * r1[a];
                L12 += G1d[a] * r1[a];
                L22 += G1[a] * r2[a];
                La += G1[a] * s0[a];
                L1a += G1d[a] * s0[a];
                L2a += G1[a] * s1v[a];
                Laa += G1[a] * t0[a];
            }
            if (Ls > 0) {
                const double inv = 1.0 / Ls;
                const double l1 = L1 * inv, l2 = L2 * inv, la = La * inv;
                v[1] = l1;
                v[2] = l2;
                v[3] = la;
                v[4] = L11 * inv - l1 * l1;
                v[5] = L22 * inv - l2 * l2;
                v[6] = L12 * inv - l1 * l2;
                v[7] = L1a * inv - l1 * la;
                v[8] = L2a * inv - l2 * la;
                v[9] = Laa * inv - la * la;
            }
            v[0] = log(lk);
        }
        for (int j = 0; j < kDerivVals; ++j) o[(size_t)j * mp] = v[j];
    }
}

template <bool PD>
__global__ void __launch_bounds__(kThreads)
llk_derivs_marker_kernel(const DeviceLayout L, const double* __restrict__ points, double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];      // [nrow][6 pairs][kEntry] (+ [3] in the log domain)
    derivs_marker_body<PD, HardyWeinberg>(L, points, nullptr, out, tab, (int)blockIdx.y, (int)blockIdx.x, (int)gridDim.x);
}

// The same given ONE pair hypothesis, `planes` [6][m_pad]
template <bool PD>
__global__ void __launch_bounds__(kThreads)
llk_pair_derivs_marker_kernel(const DeviceLayout L, const double* __restrict__ points, const float* __restrict__ planes,
                              double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];
    derivs_marker_body<PD, PairPrior>(L, points, planes, out, tab, (int)blockIdx.y, (int)blockIdx.x, (int)gridDim.x);
}

// The same for several samples: workgroup (x, y, z) is stripe x of point y of job z.  The job -- its layout included -- is
// read at a workgroup-uniform address (scalar loads); a point the job does not have, or a stripe beyond the job's 16-tile
// groups, leaves before it builds a table.
template <bool PD>
__global__ void __launch_bounds__(kThreads)
llk_derivs_marker_multi_kernel(const DerivJob* __restrict__ jobs)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];      // sized for the widest dictionary of the launch
    const DerivJob& job = jobs[blockIdx.z];
    if ((int)blockIdx.y >= job.num_point) return;
    if ((int)blockIdx.x >= tile_groups(job.L)) return;
    derivs_marker_body<PD, HardyWeinberg>(job.L, job.points, nullptr, job.marker, tab, (int)blockIdx.y, (int)blockIdx.x,
                                          (int)gridDim.x);
}

// ... and given pair hypotheses: job z's is planes[z], [6][m_pad] of its own context's order.  Several hypotheses of one
// context are several jobs with that context's layout, each with marker scratch of its own.
template <bool PD>
__global__ void __launch_bounds__(kThreads)
llk_pair_derivs_marker_multi_kernel(const DerivJob* __restrict__ jobs, const float* const* __restrict__ planes)
{
    extern __shared__ __attribute__((aligned(16))) double tab[];
    const DerivJob& job = jobs[blockIdx.z];
    if ((int)blockIdx.y >= job.num_point) return;
    if ((int)blockIdx.x >= tile_groups(job.L)) return;
    derivs_marker_body<PD, PairPrior>(job.L, job.points, planes[blockIdx.z], job.marker, tab, (int)blockIdx.y, (int)blockIdx.x,
                                      (int)gridDim.x);
}

// Output e of a point (deriv_out_count): 0 = LLK, then the gradient, then the Hessian's upper triangle row by row.
// Returns the marker scalar it sums and the UD columns (-1: none) and power-of-two factor that weight it.
__device__ __forceinline__ void output_terms(int e, int k, int& val, int& ca, int& cb, double& f)
{
    const int n = 2 * k + 1;
    ca = cb = -1;
    f = 1.0;
    if (e == 0) { val = 0; return; }
    e -= 1;
    if (e < n) {                                   // gradient
        if (e < k) { val = 1; ca = e; f = 0.5; }
        else if (e < 2 * k) { val = 2; ca = e - k; f = 0.5; }
        else val = 3;
        return;
    }
    e -= n;
    int r = 0;
    while (e >= n - r) { e -= n - r; ++r; }
    const int c = r + e;                           // r <= c
    const int tr = r < k ? 1 : r < 2 * k ? 2 : 0, tc = c < k ? 1 : c < 2 * k ? 2 : 0;   // 1 pc1, 2 pc2, 0 alpha
    const int ir = tr == 2 ? r - k : r, ic = tc == 2 ? c - k : c;
    if (tr == 1 && tc == 1) { val = 4; ca = ir; cb = ic; f = 0.25; }
    else if (tr == 2 && tc == 2) { val = 5; ca = ir; cb = ic; f = 0.25; }
    else if (tr == 1 && tc == 2) { val = 6; ca = ir; cb = ic; f = 0.25; }
    else if (tr == 1 && tc == 0) { val = 7; ca = ir; f = 0.5; }
    else if (tr == 2 && tc == 0) { val = 8; ca = ir; f = 0.5; }
    else val = 9;
}

// The body of the reduction kernels: output e of point pt.
__device__ __forceinline__ void derivs_reduce_body(const DeviceLayout& L, const double* __restrict__ marker,
                                                   double* __restrict__ out, double* part, int e, int pt)
{
    const int tid = threadIdx.x;
    const int k = L.num_pc;
    int val, ca, cb;
    double f;
    output_terms(e, k, val, ca, cb, f);
    const size_t mp = (size_t)L.m_pad, na = (size_t)L.num_active;
    const double* s = marker + ((size_t)pt * kDerivVals + (size_t)val) * mp;
    // known allele frequencies: no PC dependence (the PC entries are 0 and there are no panel rows to read)
    const bool pc_free = L.known_af == nullptr;
    const double* ua = (ca >= 0 && pc_free) ? L.ud + (size_t)ca * mp : nullptr;
    const double* ub = (cb >= 0 && pc_free) ? L.ud + (size_t)cb * mp : nullptr;
    double sum = 0.0;
    if (ca < 0 || pc_free)
        for (size_t i = (size_t)tid; i < na; i += kThreads) {
            double w = s[i];
            if (ua) w *= ua[i];
            if (ub) w *= ub[i];
            sum += w;
        }
    part[tid] = sum;
    tree_sum(part, tid);
    if (tid == 0) out[(size_t)pt * deriv_out_count(k) + e] = part[0] * f;
}

__global__ void __launch_bounds__(kThreads)
llk_derivs_reduce_kernel(const DeviceLayout L, const double* __restrict__ marker, double* __restrict__ out)
{
    __shared__ double part[kThreads];
    derivs_reduce_body(L, marker, out, part, (int)blockIdx.x, (int)blockIdx.y);
}

// workgroup (x, y, z): output x of point y of job z
__global__ void __launch_bounds__(kThreads)
llk_derivs_reduce_multi_kernel(const DerivJob* __restrict__ jobs)
{
    __shared__ double part[kThreads];
    const DerivJob& job = jobs[blockIdx.z];
    if ((int)blockIdx.y >= job.num_point || (int)blockIdx.x >= deriv_out_count(job.L.num_pc)) return;
    derivs_reduce_body(job.L, job.marker, job.out, part, (int)blockIdx.x, (int)blockIdx.y);
}

}  // namespace

namespace {
hipError_t launch_derivs(const DeviceLayout& L, int num_point, const double* d_points, const float* d_planes, double* d_marker,
                         double* d_out, hipStream_t stream)
{
    if (num_point <= 0) return hipSuccess;
    if (num_point > kDerivChunk) return hipErrorInvalidValue;
    const int nrow = L.num_code + 1;
    const size_t shmem = (size_t)nrow * (L.pd ? kRowDoublesPd : kRowDoublesLog) * sizeof(double);
    const dim3 grid((unsigned)stripe_grid(L, num_point), (unsigned)num_point), block(kThreads);
    if (d_planes) {
        if (L.pd)
            hipLaunchKernelGGL(llk_pair_derivs_marker_kernel<true>, grid, block, shmem, stream, L, d_points, d_planes, d_marker);
        else
            hipLaunchKernelGGL(llk_pair_derivs_marker_kernel<false>, grid, block, shmem, stream, L, d_points, d_planes, d_marker);
    } else if (L.pd)
        hipLaunchKernelGGL(llk_derivs_marker_kernel<true>, grid, block, shmem, stream, L, d_points, d_marker);
    else
        hipLaunchKernelGGL(llk_derivs_marker_kernel<false>, grid, block, shmem, stream, L, d_points, d_marker);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    const dim3 rgrid((unsigned)deriv_out_count(L.num_pc), (unsigned)num_point);
    hipLaunchKernelGGL(llk_derivs_reduce_kernel, rgrid, block, 0, stream, L, d_marker, d_out);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_llk_derivs(const DeviceLayout& L, int num_point, const double* d_points, double* d_marker, double* d_out,
                             hipStream_t stream)
{
    return launch_derivs(L, num_point, d_points, nullptr, d_marker, d_out, stream);
}

hipError_t launch_llk_pair_derivs(const DeviceLayout& L, int num_point, const double* d_points, const float* d_planes,
                                  double* d_marker, double* d_out, hipStream_t stream)
{
    if (!d_planes) return hipErrorInvalidValue;
    return launch_derivs(L, num_point, d_points, d_planes, d_marker, d_out, stream);
}

namespace {
hipError_t launch_derivs_multi(const DerivJob* h_jobs, const DerivJob* d_jobs, const float* const* d_planes, int num_job,
                               hipStream_t stream)
{
    if (num_job <= 0) return hipSuccess;
    // the jobs come sorted: probability domain first.  Per class one launch of the marker kernel.
    int num_pd = 0, total_points = 0, nout = 0, num_cu = 1;
    for (int j = 0; j < num_job; ++j) {
        const DerivJob& job = h_jobs[j];
        if (job.num_point < 1 || job.num_point > kDerivChunk) return hipErrorInvalidValue;
        if (job.L.pd) {
            if (num_pd != j) return hipErrorInvalidValue;
            ++num_pd;
        }
        total_points += job.num_point;
        nout = nout > deriv_out_count(job.L.num_pc) ? nout : deriv_out_count(job.L.num_pc);
        num_cu = job.L.num_cu > num_cu ? job.L.num_cu : num_cu;
    }
    // about four workgroups per CU over the whole launch pair, at least one per (job, point)
    int gx_all = (4 * num_cu + total_points - 1) / total_points;
    gx_all = gx_all > 0 ? gx_all : 1;
    const dim3 block(kThreads);
    for (int cls = 0; cls < 2; ++cls) {
        const int first = cls == 0 ? 0 : num_pd, count = cls == 0 ? num_pd : num_job - num_pd;
        if (count == 0) continue;
        size_t shmem = 0;
        int max_grp = 1;
        for (int j = first; j < first + count; ++j) {
            const DeviceLayout& L = h_jobs[j].L;
            const size_t need = (size_t)(L.num_code + 1) * (L.pd ? kRowDoublesPd : kRowDoublesLog) * sizeof(double);
            shmem = need > shmem ? need : shmem;
            const int grp = tile_groups(L);
            max_grp = grp > max_grp ? grp : max_grp;
        }
        const int gx = gx_all < max_grp ? gx_all : max_grp;
        const dim3 grid((unsigned)gx, (unsigned)kDerivChunk, (unsigned)count);
        if (d_planes) {
            if (cls == 0)
                hipLaunchKernelGGL(llk_pair_derivs_marker_multi_kernel<true>, grid, block, shmem, stream, d_jobs + first,
                                   d_planes + first);
            else
                hipLaunchKernelGGL(llk_pair_derivs_marker_multi_kernel<false>, grid, block, shmem, stream, d_jobs + first,
                                   d_planes + first);
        } else if (cls == 0)
            hipLaunchKernelGGL(llk_derivs_marker_multi_kernel<true>, grid, block, shmem, stream, d_jobs + first);
        else
            hipLaunchKernelGGL(llk_derivs_marker_multi_kernel<false>, grid, block, shmem, stream, d_jobs + first);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    const dim3 rgrid((unsigned)nout, (unsigned)kDerivChunk, (unsigned)num_job);
    hipLaunchKernelGGL(llk_derivs_reduce_multi_kernel, rgrid, block, 0, stream, d_jobs);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_llk_derivs_multi(const DerivJob* h_jobs, const DerivJob* d_jobs, int num_job, hipStream_t stream)
{
    return launch_derivs_multi(h_jobs, d_jobs, nullptr, num_job, stream);
}

hipError_t launch_llk_pair_derivs_multi(const DerivJob* h_jobs, const DerivJob* d_jobs, const float* const* d_planes, int num_job,
                                        hipStream_t stream)
{
    if (!d_planes) return hipErrorInvalidValue;
    return launch_derivs_multi(h_jobs, d_jobs, d_planes, num_job, stream);
}

}  // namespace vb2
