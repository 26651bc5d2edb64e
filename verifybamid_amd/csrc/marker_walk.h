// marker_walk.h -- how a kernel with one thread per marker reads a context's DeviceLayout (llk_kernels.h), once: the table
// records, the genotype pairs and their entry, a marker's steps (probability domain) or runs (run words), the genotype
// frequencies and the launch shape.  Device pieces only, no kernels; included by deriv_kernels.hip, source_kernels.hip and
// marker_sum_kernels.hip and by nothing else (the evaluation kernels keep the walk of eval_body.h).  DESIGN.md section 14.
//
// What stays with each unit: the width of its table rows and what it stores in them, what it accumulates per step, and
// what it makes of a marker's W.  The order of every floating-point operation is the units' own.
#ifndef VB2_MARKER_WALK_H_
#define VB2_MARKER_WALK_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "llk_kernels.h"

namespace vb2 {
namespace walk {

constexpr int kThreads = 256;                     // 16 micro-tiles of 16 markers per tile group
constexpr double kMinAf = 0.00005, kMaxAf = 0.99995;   // h:94-95

// tile groups (256 markers of the sorted order) of a layout
__host__ __device__ __forceinline__ int tile_groups(const DeviceLayout& L) { return (L.num_mt + 15) / 16; }

// About four workgroups per CU over a launch of num_point points; each walks a stripe of tile groups with one table.
inline int stripe_grid(const DeviceLayout& L, int num_point)
{
    const int ntile_grp = tile_groups(L);
    int gx = (4 * (L.num_cu > 0 ? L.num_cu : 1) + num_point - 1) / num_point;
    gx = gx < ntile_grp ? gx : ntile_grp;
    return gx > 0 ? gx : 1;
}

// off-diagonal genotype pairs, in the reference's (g1 outer, g2 inner) order (as llk_kernels.hip numbers them)
__device__ __forceinline__ void pair_g(int p, int& g1, int& g2)
{
    g1 = p >> 1;
    const int lo = p & 1;
    g2 = lo + (lo >= g1 ? 1 : 0);
}

// h:223-224 for one class / quality / pair: p = alpha u_g1 + (1 - alpha) u_g2 in the reference's expression order (prob_entry
// of eval_body.h); a negative p (alpha outside [0, 1]) is NaN, and the marker is left out.  The class is ref; alt reads the
// pair mirrored (g -> 2 - g, h:164-177).
__device__ __forceinline__ double entry_of(double alpha, double p_err, int g1, int g2)
{
    const double p_ok = 1.0 - p_err;
    const double e1 = (double)g1 * (1.0 / 6.0), e2 = (double)g2 * (1.0 / 6.0);
    const double n1 = 1.0 - 0.5 * (double)g1, n2 = 1.0 - 0.5 * (double)g2;
    const double one_minus_alpha = 1.0 - alpha;
    const double p = (alpha * e1 + one_minus_alpha * e2) * p_err + (alpha * n1 + one_minus_alpha * n2) * p_ok;
    return p >= 0.0 ? p : __builtin_nan("");
}

// u_g, the entry of a diagonal pair (g, g) whatever alpha
__device__ __forceinline__ double diag_entry_of(double p_err, int g)
{
    const double p_ok = 1.0 - p_err;
    return (double)g * (1.0 / 6.0) * p_err + (1.0 - 0.5 * (double)g) * p_ok;
}

// ---- table records ----
// A single record of L.prim.  Probability domain: a quality, class ref -- {pErr, first row | K << 16 | rstep << 24}: rows
// first, first + rstep, ... hold P^1 .. P^K (rstep a signed byte).  Run words: a code -- {signed pErr (alt < 0), code |
// twin << 16}: the alt twin's row is this one mirrored (pair 5 - p, genotype 2 - g); twin 0xffff: none.
struct SingleRec {
    double p_err;                                 // run words: signed
    int first, twin;
    __device__ __forceinline__ int kq() const { return twin & 0xff; }
    __device__ __forceinline__ int rstep() const { return (int)(int8_t)(twin >> 8); }
    __device__ __forceinline__ bool alt() const { return p_err < 0.0; }
    __device__ __forceinline__ bool has_twin() const { return twin != 0xffff; }
};
__device__ __forceinline__ SingleRec single_rec(const DeviceLayout& L, int pi)
{
    const double2 rec = L.prim[pi];
    const uint32_t pr = (uint32_t)__double_as_longlong(rec.y);
    return {rec.x, (int)(pr & 0xffffu), (int)(pr >> 16)};
}
template <bool PD>
__device__ __forceinline__ int num_single(const DeviceLayout& L)
{
    return PD ? L.num_prim - L.num_pair : L.num_prim;
}

// The window rows of the probability domain, after the single records in L.prim: {ra | rb << 16, dst}, row dst = row ra x row
// rb, in two levels (level 1 uses rows of level 0).  f(ra, rb, dst, p) for every record with its rows inside the table and
// every p < WIDTH, one barrier before each level; the caller adds the one after the last.
template <int WIDTH, class F>
__device__ __forceinline__ void for_each_window(const DeviceLayout& L, int nrow, int tid, F&& f)
{
    const int first = num_single<true>(L);
    for (int level = 0; level < 2; ++level) {
        const int nrec = level == 0 ? L.num_pair - L.num_pair2 : L.num_pair2;
        const int base = first + (level == 0 ? 0 : L.num_pair - L.num_pair2);
        __syncthreads();
        for (int e = tid; e < nrec * WIDTH; e += kThreads) {
            const int pi = e / WIDTH, p = e - pi * WIDTH;
            const double2 rec = L.prim[base + pi];
            const uint32_t ab = (uint32_t)__double_as_longlong(rec.x), dst = (uint32_t)__double_as_longlong(rec.y);
            const uint32_t ra = ab & 0xffffu, rb = ab >> 16;
            if (ra >= (uint32_t)nrow || rb >= (uint32_t)nrow || dst >= (uint32_t)nrow) continue;
            f(ra, rb, dst, p);
        }
    }
}

// ---- a marker's steps or runs ----
// Marker m (0..15) of a micro-tile with record rec = L.mt_rec[mt]; tab: the table in LDS, ROW doubles per row.
//   PD: rec = {first word row, ref steps | all steps << 16}; a step is the 16-bit byte offset of its row (+ kPdAltOffset for
//       class alt), two per word.  f(t, alt, 1.0) per step: alt reads the row mirrored (pair 5 - p, genotype 2 - g).
//   !PD: rec = {first row, rows}; a row is two run words, a run = row byte offset | top 16 bits of double(count) << 16.
//       f(t, false, n) per run: n reads of the row.
// A row outside the table reads the padding row (L.num_code).
template <bool PD, int ROW, class F>
__device__ __forceinline__ void for_each_step(const DeviceLayout& L, const double* tab, int nrow, uint2 rec, int m, F&& f)
{
    if constexpr (PD) {
        const uint32_t s1 = rec.y & 0xffffu, s2 = rec.y >> 16;
        const uint16_t* c16 = reinterpret_cast<const uint16_t*>(L.codes);
        for (uint32_t s = 0; s < s2; ++s) {
            const bool alt = s >= s1;
            uint32_t off = c16[(((size_t)rec.x + (s >> 1)) * 16 + (size_t)m) * 2 + (s & 1u)];
            if (alt) off -= (uint32_t)kPdAltOffset;
            uint32_t row = off / (uint32_t)L.row_bytes;
            row = row < (uint32_t)nrow ? row : (uint32_t)L.num_code;
            f(tab + (size_t)row * ROW, alt, 1.0);
        }
    } else {
        for (uint32_t r = 0; r < rec.y; ++r) {
            const uint2 rw2 = L.codes[((size_t)rec.x + r) * 16 + (size_t)m];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t rw = j ? rw2.y : rw2.x;
                const double n = __hiloint2double((int)(rw & 0xffff0000u), 0);
                uint32_t row = (rw & 0xffffu) / (uint32_t)L.row_bytes;
                row = row < (uint32_t)nrow ? row : (uint32_t)L.num_code;
                f(tab + (size_t)row * ROW, false, n);
            }
        }
    }
}

// ---- allele frequencies ----
// (The projection AF = (UD pc + mu) / 2 stays in the units: each has its own unrolling of the loop over the PCs, and shared
// it moved the schedule of all three.)
__device__ __forceinline__ double clamp_af(double af)
{
    if (af < kMinAf) af = kMinAf;
    if (af > kMaxAf) af = kMaxAf;
    return af;
}

// GF (h:186-192)
__device__ __forceinline__ void gf_of(double af, double* gf)
{
    af = clamp_af(af);
    gf[0] = (1 - af) * (1 - af);
    gf[1] = 2 * (af) * (1 - af);
    gf[2] = af * af;
}

// L = sum W[g1][g2] G1[g1] G2[g2] in the reference's order (h:307-309)
__device__ __forceinline__ double mix_of(const double (&W)[3][3], const double* G1, const double* G2)
{
    double lk = 0.0;
    for (int g1 = 0; g1 < 3; ++g1)
        for (int g2 = 0; g2 < 3; ++g2) lk += W[g1][g2] * G1[g1] * G2[g2];
    return lk;
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

}  // namespace walk
}  // namespace vb2
#endif
