// eval_body.h -- the device code that every gfx950 evaluation kernel for the genotype-mixture log-likelihood is made of:
// the math helpers, the table entries, the wave shapes and eval_body itself.  No kernel, no launcher and no host-only
// function: each kernel sits next to its launcher in the one unit that instantiates it -- llk_kernels.hip (single sample,
// split launch, resident search: iterative-ILP scheduler) or llk_passes.hip (pass-per-group and cohort kernels: default
// scheduler).
// (reference: FullLLKFunc::ComputeMixLLKs, ContaminationEstimator.h:194-314).
//
// Work decomposition:
//   * a wave = 16 markers x 4 candidate slots: lane (m, g) walks marker m's reads for the BTL
//     candidate points of slot g (MODE 2: 8 points per group); 4-point launches use two
//     16-marker micro-tiles x 2 slots x 2 points instead (MODE 3), 1- and 2-point launches four (MODE 4, 5).  Markers are sorted by depth
//     at context creation and grouped in 16-marker micro-tiles so all lanes of a wave run about
//     the same number of steps;
//   * a marker's reads are run-length coded over the (class x quality) dictionary: one 32-bit run
//     word per distinct code (low half = LDS byte offset of the code's table row, high half = the
//     top 16 bits of double(count), count <= 31), two per uint2, stored [micro-tile][step/2][marker]:
//     a wave load is one contiguous 128-byte row, rows are prefetched 8 deep in cohort steps (HBM), 2-4 deep otherwise;
//   * the per-alpha log-likelihood table (h:213-229) is rebuilt per launch in LDS,
//     restricted to the codes that occur in the data and to the six OFF-diagonal
//     genotype pairs: the diagonal (g1==g2) and the "other base" class do not
//     depend on alpha or the PCs and were summed once at context creation;
//   * each lane keeps 6 FP64 accumulators per candidate point in registers and
//     gathers its table row from LDS with ds_read_b128 (row = 6 values per point);
//   * epilogue per lane: UD*PC projection (h:251-267), HWE priors (h:186-192),
//     9-term exp-sum with the reference's `> 0` test (h:307-311); the marker likelihoods are
//     multiplied as (mantissa, exponent) and the log is taken once per (workgroup, point);
//   * persistent launch: one 1024-thread workgroup per CU (table built once per workgroup);
//     depth-sorted micro-tiles are dealt round-robin across workgroups, so every CU sees the
//     same depth mix, and pulled by the waves of a workgroup through an LDS work queue;
//   * deterministic reduction: 16-lane butterfly -> work-item slots -> per-workgroup partial;
//     the partials cross workgroups inside the launch, either collected by workgroup 0 from
//     tagged, self-validating sets (<= 16 points, cohorts, resident search) or summed by the last
//     workgroup to arrive at an agent-scope ticket (bigger batches), always in the same fixed
//     order (or, two-kernel mode, by llk_finalize_kernel);
//   * llk_resident_kernel keeps the same body on the CUs for a whole Nelder-Mead search and
//     takes its batches from a mailbox in mapped host memory.
//
// Two layouts of a sample (DeviceLayout::pd; Context::create decides):
//   * run words / sums of logarithms, as above: any depth;
//   * probability domain (round 6; template parameter PD): the table holds P(read | genotype pair, alpha)^n per quality,
//     n = 1 .. K, class ref only -- class alt is class ref with the genotypes mirrored (h:164-177) --, a marker's list is one
//     16-bit row offset per STEP (a run of count c = ceil(c / K) steps; ref steps, then alt steps), the six sums are six
//     PRODUCTS of table rows, and the epilogue needs no exponential: (6 exp + 6 log-table rows) per marker and point less,
//     at rounding-level differences.  Taken when every marker's likelihood is bound to stay far from the smallest doubles.
#ifndef VB2_EVAL_BODY_H_
#define VB2_EVAL_BODY_H_

#include "llk_kernels.h"

#include <hip/hip_runtime.h>

#include "kernel_debug.h"

#include <type_traits>
namespace vb2 {

// off-diagonal genotype pairs, in the reference's (g1 outer, g2 inner) order
__device__ __forceinline__ void pair_of(int p, int& g1, int& g2)
{
    // p: 0:(0,1) 1:(0,2) 2:(1,0) 3:(1,2) 4:(2,0) 5:(2,1)
    g1 = p >> 1;
    const int lo = p & 1;
    g2 = lo + (lo >= g1 ? 1 : 0);
}

// v[i] + v[i ^ 32], then ^ 16, 8, 4, 2, 1: the butterfly every final sum of partial LLKs goes through (the order is part of the
// result's bits).  Round 4: without ds_bpermute -- gfx950's v_permlane32_swap / v_permlane16_swap bring the other half / the
// other row next to a lane's own value (x + y = y + x: which of the two registers holds the lane's own does not matter), the
// distances 8 .. 1 are DPP moves inside a row.  The same additions in the same order: the same bits; a search round waits for
// this once (workgroup 0's four sums), a cross-lane LDS round trip per step before.
__device__ __forceinline__ double wave_sum(double v)
{
    {
        const unsigned hi = (unsigned)__double2hiint(v), lo = (unsigned)__double2loint(v);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    }
    {
        const unsigned hi = (unsigned)__double2hiint(v), lo = (unsigned)__double2loint(v);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    }
    auto dpp = [](double x, auto ctrl) -> double {
        constexpr int kCtrl = decltype(ctrl)::value;
        return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(x), kCtrl, 0xf, 0xf, false),
                                __builtin_amdgcn_update_dpp(0, __double2loint(x), kCtrl, 0xf, 0xf, false));
    };
    v += dpp(v, std::integral_constant<int, 0x128>());                       // row_ror:8   -> lane i ^ 8
    {                                                                        // lane i ^ 4: quads 1, 3 <- i - 4, quads 0, 2 <- i + 4
        const int hi = __double2hiint(v), lo = __double2loint(v);
        const int h1 = __builtin_amdgcn_update_dpp(0, hi, 0x124, 0xf, 0xa, false), l1 = __builtin_amdgcn_update_dpp(0, lo, 0x124, 0xf, 0xa, false);
        const int h2 = __builtin_amdgcn_update_dpp(h1, hi, 0x12C, 0xf, 0x5, false), l2 = __builtin_amdgcn_update_dpp(l1, lo, 0x12C, 0xf, 0x5, false);
        v += __hiloint2double(h2, l2);
    }
    v += dpp(v, std::integral_constant<int, 0x4E>());                        // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0xB1>());                        // quad_perm [1,0,3,2]
    return v;
}

// 2^(j/64), j = 0..63, correctly rounded (generated with 60-digit decimal arithmetic).
__device__ const double kExp2Tab[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0};

// exp(x) for x <= 0 (arguments here are sums of log-probabilities), FP64, <= 1.1 ulp:
// x = k*ln2/64 + r, |r| <= ln2/128; exp(x) = 2^(k>>6) * 2^((k&63)/64) * (1 + p(r)), p = r + r^2 q(r), q of degree 3, the
// 2^(j/64) factor from an LDS table.
// `etab_lane` = LDS byte address of this lane's column of the bank-replicated table: entry j sits
// 256*j bytes further, i.e. in LDS banks 2*(lane%32), 2*(lane%32)+1 whatever j is, so the
// 64 lanes' lookups of a wave never conflict (a 512-byte table would: random j's collide).
// v_max_f64 / v_min_f64 as single instructions: the compiler's fmax/fmin lowering first
// canonicalises an operand it cannot prove free of signalling NaNs (one more v_max_f64 x, x);
// the hardware instruction quiets them by itself.
//
// Two forms.  The one every marker x point takes six times applies 2^(k>>6) to the TABLE ENTRY before the last
// multiply-add, by ONE integer add on the entry's high word: the table holds the entries with j << 14 taken off their high
// words (exp_tab_entry), so that adding k << 14 = (k>>6) << 20 + j << 14 leaves exactly (k>>6) in the exponent field -- the
// scaling is exact and the result the same bits as scaling afterwards; the shift and the v_ldexp_f64 of the other form
// are gone, and so is the clamp (three of an exponential's sixteen instructions for one).  It holds as long
// as the scaled entry is a normal number, i.e. for x >= -708 (2^-1022 <= e^-708.39): the caller (marker_lk) takes the
// minimum of a marker's six arguments -- five v_min_f64, integer-rate -- and sends markers with an argument below that
// (deep pileups; -inf: a table entry that is log 0) through the EXACT form: clamp at -800, v_ldexp_f64, gradual underflow,
// 0 exactly where the reference's exp() reaches it (the `markerLK > 0` test, h:310).  Either way the same bits as before.
__device__ __forceinline__ double vmax_f64(double x, double c)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "s"(c));
    return r;
}
__device__ __forceinline__ double vmin_f64(double x, double c)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(x), "s"(c));
    return r;
}
__device__ __forceinline__ double vmin2_f64(double x, double y)      // (both operands in vector registers)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}

typedef __attribute__((address_space(3))) const double lds_cdouble;
typedef double __attribute__((ext_vector_type(2))) vdouble2;      // (a plain vector: loadable through address_space(3))
typedef __attribute__((address_space(3))) const vdouble2 lds_cdouble2;
__device__ __forceinline__ uint32_t lds_byte_addr(const void* p)      // generic pointer into LDS -> LDS address
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}

// what the LDS copy of the table holds for 2^(j/64): the double with j << 14 taken off its high word
__device__ __forceinline__ double exp_tab_entry(double t, int j)
{
    return __hiloint2double(__double2hiint(t) - (j << 14), __double2loint(t));
}

// ESH: log2 of the byte stride between two entries of the table -- 8: 32 copies of every entry, the conflict-free layout
// above (16 KiB); 6: eight copies (4 KiB; lookups of different entries in one column collide) for the one kernel that needs
// the 12 KiB for a third point group's table (llk_eval_passes_kernel).
// EXACT: see above.
template <int ESH = 8, bool EXACT = false>
__device__ __forceinline__ double exp_nonpos(double x, uint32_t& etab_lane)
{
    const double kInvStep = 0x1.71547652b82fep+6;        // 64/ln2
    const double kStepHi = 0x1.62e42fee00000p-7;         // ln2/64, 32 significant bits: k*hi is exact
    const double kStepLo = 0x1.a39ef35793c76p-39;
    const double kMagic = 0x1.8p52;                      // 2^52 + 2^51: x + kMagic rounds x to an integer
    // EXACT: below -800 the result is 0 anyway (2^-1154); the clamp also maps -inf to a finite
    // argument, so no special case is needed after the ldexp.  (The other form is only called with x >= -708.)
    if constexpr (EXACT) x = vmax_f64(x, -800.0);
    // k = rint(x * 64/ln2) by the magic-number addition: the low mantissa word of the sum IS the
    // integer (two's complement), so no v_rndne / v_cvt_i32 pair
    const double tk = fma(x, kInvStep, kMagic);
    const int k = __double2loint(tk);
    const double kd = tk - kMagic;
    double r = fma(-kd, kStepHi, x);
    r = fma(-kd, kStepLo, r);
    double t;
    if constexpr (ESH == 8) {
        // The conflict-free table: entry j of this lane's column sits at LDS address j << 8 | etab_lane, etab_lane < 256 -- the
        // index IS byte 1 of the address.  One SDWA instruction masks k to six bits and drops them into byte 1 of the
        // register that holds etab_lane, the other bytes kept (a shift and an and-or before).  The register is the lane's
        // for the whole kernel: byte 1 is rewritten by every call, byte 0 never.
        asm("v_and_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD"
            : "+v"(etab_lane)
            : "v"(k), "s"(63));
        t = *reinterpret_cast<lds_cdouble*>(etab_lane);
    } else {
        t = *reinterpret_cast<lds_cdouble*>((((uint32_t)k << ESH) & (63u << ESH)) | etab_lane);
    }
    // exp(r) - 1 = r + r^2 q(r), q of degree 3 through the Chebyshev nodes of |r| <= ln2/128 (60-digit arithmetic; relative error
    // of exp 4.4e-18): worst error against expl over [-700, 0] 1.02 ulp
    double p = fma(r, 0x1.11111d8fbe766p-7, 0x1.55556b3304ec0p-5);
    p = fma(p, r, 0x1.5555555555255p-3);
    p = fma(p, r, 0x1.ffffffffff57fp-2);
    p = fma(p, r * r, r);
    if constexpr (EXACT) {
        t = __hiloint2double(__double2hiint(t) + ((k & 63) << 14), __double2loint(t));     // the entry itself again
        return ldexp(fma(t, p, t), k >> 6);
    } else {
        t = __hiloint2double(__double2hiint(t) + (int)((uint32_t)k << 14), __double2loint(t));   // 2^(k>>6) 2^(j/64), exactly
        return fma(t, p, t);
    }
}

// log(x) for x >= 0, FP64 (fdlibm's e_log algorithm with explicit FMAs, ~1 ulp):
// x = 2^e * m, m in [sqrt(1/2), sqrt(2)); f = m-1; s = f/(2+f);
// log(m) = f - hfsq + s*(hfsq + R(s^2)).
// log(0) = -inf (table entries whose probability is exactly 0, e.g. q = 0 / hom-ref).
// The library log() is not used: built without FMA contraction (this file's
// -ffp-contract=off, needed for reference-order rounding elsewhere) it expands to
// ~115 instructions, four times this.
__device__ __forceinline__ double log_nonneg(double x)
{
    const double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    double m = __builtin_amdgcn_frexp_mant(x);           // [0.5, 1), subnormals included
    int e = __builtin_amdgcn_frexp_exp(x);
    const bool lo = m < 0.70710678118654752440;
    m = lo ? m + m : m;
    e = lo ? e - 1 : e;
    const double f = m - 1.0;
    const double d = 2.0 + f;
    double r = __builtin_amdgcn_rcp(d);                  // 1/d, refined twice (Newton)
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    double sq = f * r;
    sq = fma(fma(-d, sq, f), r, sq);                     // s = f/d to ~0.5 ulp
    const double z = sq * sq;
    const double w = z * z;
    const double t1 = w * fma(w, fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * fma(w, fma(w, fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    const double dk = (double)e;
    const double res = fma(dk, kLn2Hi, -((hfsq - fma(sq, hfsq + R, dk * kLn2Lo)) - f));
    return x == 0.0 ? -__builtin_huge_val() : res;
}

// log(x) for 0 <= x <= 1 and normal (the per-alpha table's entries: logarithms of probabilities), table-driven -- round 4,
// second session: the six tables of a 48-point launch were 3.9 us of its 65 (the launch with the table build compiled out),
// nearly all of it the fdlibm-style logarithm above: ~40 dependent instructions, with a reciprocal and two Newton steps.
// Here: x = 2^k z, the interval i of z (seven mantissa bits after an offset that puts 1 INSIDE an interval) gives
// {1 / c_i, log c_i} from a 2 KiB table in LDS; r = fma(z, 1/c, -1) is exact and |r| <= 2^-8;
// log x = k ln2 + log c + (r + r^2 P(r)), P of degree 4.  ~22 instructions, none of them a transcendental.
// The table and the polynomial: log_table.inc, generated with 60-digit arithmetic by tools/gen_log_table.py (the interval
// around 1 has c = 1 exactly: log(1) = 0, and log(1 - p_err) -- most entries of a pileup's table -- keeps full relative
// accuracy; the other reciprocals are chosen so that log c is a double to within 0.001 ulp).  oracle/check_log_table.c is
// this routine statement for statement on the host, held to <= 1.6 ulp against the C library's long-double logarithm
// (tests/test_oracle_golden.py; typical < 0.8, the 1.5 where k ln2 + log c sits a binade above the result).
#include "log_table.inc"
constexpr int kLogTabDoubles = 256;
__device__ const double2 kLogTabRows[128] = {VB2_LOG_TAB_ROWS};
// (the routine proper: x normal and positive, hi its high word, kadj what the caller scaled x by)
__device__ __forceinline__ double log_tab_core(double x, uint32_t hi, int kadj, uint32_t ltab_addr)
{
    const double kLn2Hi = 0x1.62e42fefa3800p-1, kLn2Lo = 0x1.ef35793c76730p-45;
    constexpr double kP[5] = {VB2_LOG_POLY};
    const uint32_t tmp = hi - 0x3FE5F000u;
    const uint32_t i = (tmp >> 13) & 127u;
    const int k = ((int)tmp >> 20) - kadj;
    const double z = __hiloint2double((int)(hi - (tmp & 0xFFF00000u)), __double2loint(x));
    const vdouble2 t = *reinterpret_cast<lds_cdouble2*>(ltab_addr + i * 16u);
    const double r = fma(z, t.x, -1.0);
    const double kd = (double)k;
    const double w = fma(kd, kLn2Hi, t.y);
    const double r2 = r * r;
    // (the polynomial in two halves and k ln2's low part next to r: five dependent steps behind r instead of seven)
    const double q0 = fma(r, kP[1], kP[0]);
    double q1 = fma(r, kP[3], kP[2]);
    q1 = fma(r2, kP[4], q1);
    const double p = fma(r2, q1, q0);
    const double rl = fma(kd, kLn2Lo, r);
    const double y = fma(r2, p, rl);
    return w + y;
}
__device__ __forceinline__ double log_tab(double x, uint32_t ltab_addr /* LDS byte address of the table's copy */)
{
    const uint32_t hi = (uint32_t)__double2hiint(x);
    double res = log_tab_core(x, hi, 0, ltab_addr);
    // Outside the table's domain (one compare on the high word, and a branch no wave of a search ever takes --
    // a real branch: as selects folded into the routine the four cases cost every entry a dozen instructions):
    // zero -> -inf (the reference's log(0): entries whose probability is exactly 0); a positive subnormal (alpha below
    // 2^-1022: a logit under -708) -> scaled into the normal range, 64 ln2 taken off again through k; NaN, a negative
    // "probability" (alpha outside [0, 1]) -> NaN; +inf -> +inf: libm's answers, so that a NaN likelihood reaches the
    // caller as NaN and not as a plausible number.
    if (__builtin_expect(hi - 0x00100000u >= 0x7FE00000u, 0)) {
        if (x == 0.0) res = -__builtin_huge_val();
        else if (!(x > 0.0)) res = __builtin_nan("");
        else if (hi >= 0x7FF00000u) res = x;
        else {
            const double xs = x * 0x1p64;
            res = log_tab_core(xs, (uint32_t)__double2hiint(xs), 64, ltab_addr);
        }
    }
    return res;
}

// A positive value as (mantissa in [0.5,1), binary exponent): products of likelihoods are
// kept in this form so that a marker's log is never taken -- one log per (workgroup, point)
// replaces one per (marker, point).
struct ScaledProd {
    double m;     // mantissa product
    double e;     // exponent sum (exact integer)
};
__device__ __forceinline__ void sp_renorm(ScaledProd& p)
{
    p.e += (double)__builtin_amdgcn_frexp_exp(p.m);
    p.m = __builtin_amdgcn_frexp_mant(p.m);
}
// The per-lane running product of the static deal: integer exponent (one v_add_u32 per marker)
// and a mantissa that is only renormalised every kLazyRenorm factors -- each factor is a
// mantissa in [0.5, 1), so 256 of them cannot underflow.
struct LaneProd {
    double m;
    int e;
};
constexpr int kLazyRenorm = 256;

// One table entry, with the reference's expression order (h:223-225).
// perr_signed = +pErr(q) for class ref, -pErr(q) for class alt (one load per code;
// the alt class is the ref class with genotypes mirrored, g -> 2-g: h:164-177).
__device__ __forceinline__ double table_entry(double alpha, double perr_signed, int g1, int g2, uint32_t ltab_addr)
{
    const bool alt = perr_signed < 0.0;
    const double p_err = fabs(perr_signed);
    const double p_ok = 1.0 - p_err;
    if (alt) { g1 = 2 - g1; g2 = 2 - g2; }
    // class ref: P(ref | g, error) = {0, 1/6, 1/3}[g], P(ref | g, no error) = {1, .5, 0}[g].
    // As arithmetic on g (exact: fl(1/3) = 2*fl(1/6), the same mantissa one binade up; 1 - g/2
    // is exact), which is cheaper than selecting among 64-bit constants:
    const double e1 = (double)g1 * (1.0 / 6.0), e2 = (double)g2 * (1.0 / 6.0);
    const double n1 = 1.0 - 0.5 * (double)g1, n2 = 1.0 - 0.5 * (double)g2;
    const double one_minus_alpha = 1.0 - alpha;
    const double val = (alpha * e1 + one_minus_alpha * e2) * p_err +
                       (alpha * n1 + one_minus_alpha * n2) * p_ok;
    return log_tab(val, ltab_addr);
}

// The same entry BEFORE its logarithm, class ref (probability-domain contexts: llk_kernels.h, kMaxPow): the value the
// reference takes the logarithm of (h:223-225, the same expression order); the table build multiplies it up to P^2 .. P^K.  A
// negative "probability" (alpha outside [0, 1]) or a NaN becomes NaN, like the reference's log() of it: the marker's
// likelihood is then NaN, fails `markerLK > 0` and the marker is left out.
__device__ __forceinline__ double prob_entry(double alpha, double p_err, int g1, int g2)
{
    const double p_ok = 1.0 - p_err;
    const double e1 = (double)g1 * (1.0 / 6.0), e2 = (double)g2 * (1.0 / 6.0);
    const double n1 = 1.0 - 0.5 * (double)g1, n2 = 1.0 - 0.5 * (double)g2;
    const double one_minus_alpha = 1.0 - alpha;
    double val = (alpha * e1 + one_minus_alpha * e2) * p_err +
                 (alpha * n1 + one_minus_alpha * n2) * p_ok;
    return val >= 0.0 ? val : __builtin_nan("");
}

__device__ __forceinline__ void initial_gf(double af, double* gf)   // h:186-192
{
    // (v_max_f64 / v_min_f64 instead of compare + select; a NaN allele frequency -- NaN
    // parameters -- becomes min_af here where the reference keeps the NaN)
    af = vmin_f64(vmax_f64(af, 0.00005), 0.99995);
    gf[0] = (1 - af) * (1 - af);
    gf[1] = 2 * (af) * (1 - af);
    gf[2] = af * af;
}

// Row stride of the LDS table: L.row_bytes (llk_kernels.h: kRowBytesWide = 6 values x 8 points
// + 2 doubles of padding, or kRowBytesNarrow = 6 x 4 + 2), the same for every wave shape of a
// context because the run words of the pileup carry PRE-MULTIPLIED row offsets.  Either stride
// is an odd number of 16-byte slots -> 16 consecutive codes land in 16 distinct 4-dword bank
// slots for ds_read_b128 (bank = (addr/4) % 64).

constexpr int kExpTabDoubles = 64 * 32;    // exp_nonpos's table in LDS (16 KiB)
constexpr int kPrefetch = 8;               // rows of run dwords in flight per lane: cohort steps (lists from HBM)
constexpr int kPrefetchL2 = 2;             // ... a single sample's launches and search rounds (lists in L2 / LDS)

// Lane -> (marker m in the micro-tile, candidate slot g): the 16 lanes that ds_read_b128 services in one LDS pass
// (lanes {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32; MI355X_MICROARCH.md, LDS) share one candidate
// slot, so within a pass the addresses differ only by the code.
__device__ __forceinline__ void lane_map(int lane, int& m, int& g)
{
    const int q = (lane >> 2) & 7;                       // quad within the 32-lane half
    const int nib = (0x76452310u >> (4 * q)) & 7;        // (rank<<1 | group) of quad q
    g = (nib & 1) + 2 * (lane >> 5);
    m = ((nib >> 1) << 2) + (lane & 3);
}
__device__ __forceinline__ int lane_of(int m, int g)
{
    const int idx = ((g & 1) << 2) + (m >> 2);           // group*4 + quad-rank
    const int q = (0x74216530u >> (4 * idx)) & 7;
    return ((g >> 1) << 5) + (q << 2) + (m & 3);
}

// The value of lane `partner` = the lane whose marker index differs in bit `off` (same slot).  The lane map keeps the low
// two marker bits in the low two lane bits, so the exchanges over off = 1 and 2 stay inside a quad: DPP quad permutes -- VALU
// moves, no trip through the LDS crossbar (a ds_bpermute per dword and ~100 cycles before the dependent multiply).  Marker
// bit 2 selects between the quads {0,3}, {1,2} of a 16-lane row (lane_of: ranks 0,1,2,3 of slot-parity 0 sit in quads
// 0,3,5,6, of parity 1 in 1,2,4,7), i.e. quad j <-> 3 - j with the lane in the quad kept: a row rotation by 4 for the
// quads 0 and 2, by 12 for 1 and 3 (tools/ubench/dpp_map.hip: row_ror:n gives lane i the value of lane i - n of its row)
// -- two DPP moves with bank masks.  The exchange over 8 crosses rows and stays a ds_bpermute (as three VALU moves per dword
// -- lane ^ 4, then v_permlane16_swap -- it was measured slower: HISTORY.md, round 4; the split launches, whose LDS pipe is the
// busier one now, take lane_pair8_u32 below instead).  Multiplication commutes: the same bits whatever the route.
__device__ __forceinline__ int lane_xchg_i32(int x, int off, int partner)
{
    if (off == 1) return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true);     // quad_perm [1,0,3,2]
    if (off == 2) return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true);     // quad_perm [2,3,0,1]
    if (off == 4) {
        const int a = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xf, 0x5, false);       // row_ror:4  -> quads 0 and 2 of every row
        return __builtin_amdgcn_update_dpp(a, x, 0x12C, 0xf, 0xa, false);              // row_ror:12 -> quads 1 and 3
    }
    return __shfl(x, partner, 64);
}
__device__ __forceinline__ double lane_xchg_f64(double x, int off, int partner)
{
    if (off == 1 || off == 2 || off == 4)
        return __hiloint2double(lane_xchg_i32(__double2hiint(x), off, partner), lane_xchg_i32(__double2loint(x), off, partner));
    return __shfl(x, partner, 64);
}

// The exchange over marker bit 3 as VALU moves (eval_body, EPI_X8; the 8-point shape, where only the lane of marker 0 -- a
// lane of an EVEN 16-lane row -- stores the tile's product).  Under lane_map a marker's partner over bit 3 sits in the other row
// of its 32-lane half, at quad j ^ 1 of that row (slot parity 0: quads 0, 3 of the even row hold ranks 0, 1, quads 1, 2 of the
// odd row ranks 2, 3; parity 1: quads 1, 2 and 0, 3).  So the ODD rows swap their quads j <-> j ^ 1 -- two DPP moves
// under a row mask, the even rows keep their own --, and v_permlane16_swap puts the two rows' values side by
// side: a lane of an even row holds {its own, its partner's}, in this order.  A lane of an odd row holds the same two values
// as the even row's lane at its position: the odd rows become copies of the even ones, go through the later exchanges (all
// inside a row) as such, and none of their lanes is stored.  The same two factors into the same multiply in every even-row
// lane: the same bits as through ds_bpermute.
__device__ __forceinline__ void lane_pair8_u32(unsigned x, unsigned& own, unsigned& other)
{
    // (row_half_mirror -- lane i <- lane 7 - i of its half row: quad j ^ 1 with its lanes reversed --, then the lanes of every quad
    // reversed again: both moves read only their own result, so they work in place, where two bank-masked rotations of x each
    // needed x itself -- a copy per dword)
    const int a = __builtin_amdgcn_update_dpp((int)x, (int)x, 0x141, 0xa, 0xf, false);             // odd rows: row_half_mirror
    const unsigned z = (unsigned)__builtin_amdgcn_update_dpp(a, a, 0x1B, 0xa, 0xf, false);         // odd rows: quad_perm [3,2,1,0]
    const auto r = __builtin_amdgcn_permlane16_swap(z, z, false, false);      // [0]: the even row's value in both rows, [1]: the odd row's
    own = r[0];
    other = r[1];
}
// The same exchange as a reduce-scatter (eval_body, EPI_SCATTER): a lane holds a dword of TWO points, p0 and p1.  The odd rows
// swap their quads of both in place, as above; v_permlane16_swap then swaps the odd rows of its first operand, p0, with the even
// rows of its second, p1.  An even-row lane ends with {own p0, partner's p0} -- lane_pair8_u32's pair of point 0 --, the odd-row
// lane sixteen above it with {that even lane's p1, its partner's p1} -- the pair of point 1 that lane_pair8_u32 leaves in the
// even-row lane, in the same order.  The odd rows carry point 1 under the even rows' labelling (marker m - 8, slot parity flipped),
// through the later exchanges -- all inside a row -- as copies of the even rows did.  Five moves per dword of two points, not six.
__device__ __forceinline__ void lane_scatter8_u32(unsigned p0, unsigned p1, unsigned& own, unsigned& other)
{
    const int a0 = __builtin_amdgcn_update_dpp((int)p0, (int)p0, 0x141, 0xa, 0xf, false);          // odd rows: row_half_mirror
    const unsigned z0 = (unsigned)__builtin_amdgcn_update_dpp(a0, a0, 0x1B, 0xa, 0xf, false);      // odd rows: quad_perm [3,2,1,0]
    const int a1 = __builtin_amdgcn_update_dpp((int)p1, (int)p1, 0x141, 0xa, 0xf, false);
    const unsigned z1 = (unsigned)__builtin_amdgcn_update_dpp(a1, a1, 0x1B, 0xa, 0xf, false);
    const auto r = __builtin_amdgcn_permlane16_swap(z0, z1, false, false);
    own = r[0];
    other = r[1];
}

// Component KK of the projection with its coefficients from a DPP row's lanes (eval_body, COEF_DPP; the hardware's conditions are
// listed where marker_lk calls this): a1[t] += uu * coefficient [KK][t], a2[t] += uu * coefficient [K + KK][t] of the lane's own slot,
// t = point 0, 1.  ca: lane i of the row holds coefficient i of the slot of the row's quads 0 and 3; cb: the same for the slot of its
// quads 1 and 2, from lane HI on (K = 4: HI = 0, a register pair of its own; K = 2: HI = 8, the upper half of ca's pair).  KK = 0
// opens with the wait states of a vector write of EXEC.
template <int K, int KK>
__device__ __forceinline__ void project_dpp(double& a10, double& a11, double& a20, double& a21, const double ca, const double cb, const double uu)
{
    static_assert((K == 4 || K == 2) && KK >= 0 && KK < K, "sixteen coefficients a slot, or eight");
    constexpr int kHi = K == 2 ? 8 : 0;
    constexpr int j10 = 2 * KK, j11 = 2 * KK + 1, j20 = 2 * (K + KK), j21 = 2 * (K + KK) + 1;
#define VB2_COEF_FMAS \
    "v_fmac_f64_dpp %0, %4, %6 row_newbcast:%7 row_mask:0xf bank_mask:0x9\n\t" \
    "v_fmac_f64_dpp %1, %4, %6 row_newbcast:%8 row_mask:0xf bank_mask:0x9\n\t" \
    "v_fmac_f64_dpp %2, %4, %6 row_newbcast:%9 row_mask:0xf bank_mask:0x9\n\t" \
    "v_fmac_f64_dpp %3, %4, %6 row_newbcast:%10 row_mask:0xf bank_mask:0x9\n\t" \
    "v_fmac_f64_dpp %0, %5, %6 row_newbcast:%11 row_mask:0xf bank_mask:0x6\n\t" \
    "v_fmac_f64_dpp %1, %5, %6 row_newbcast:%12 row_mask:0xf bank_mask:0x6\n\t" \
    "v_fmac_f64_dpp %2, %5, %6 row_newbcast:%13 row_mask:0xf bank_mask:0x6\n\t" \
    "v_fmac_f64_dpp %3, %5, %6 row_newbcast:%14 row_mask:0xf bank_mask:0x6"
#define VB2_COEF_OPERANDS \
    : "+v"(a10), "+v"(a11), "+v"(a20), "+v"(a21) \
    : "v"(ca), "v"(cb), "v"(uu), "n"(j10), "n"(j11), "n"(j20), "n"(j21), "n"(kHi + j10), "n"(kHi + j11), "n"(kHi + j20), "n"(kHi + j21)
    if constexpr (KK == 0) asm volatile("s_nop 4\n\t" VB2_COEF_FMAS VB2_COEF_OPERANDS);
    else asm volatile(VB2_COEF_FMAS VB2_COEF_OPERANDS);
#undef VB2_COEF_FMAS
#undef VB2_COEF_OPERANDS
}

// Occupancy target: one 1024-thread workgroup per CU (4 waves/SIMD, <=128 VGPRs).  Two
// smaller workgroups per CU were measured slower: the per-alpha table is built once per
// workgroup, and that redundant work is 9 % of a launch's transcendentals at one
// workgroup per CU but 18 % at two.
template <int MODE> struct Geom { static constexpr int kMaxWaves = 16, kBlocksPerCU = 1, kWavesPerSimd = 4; };
// points per group of a wave shape
template <int MODE> struct ModeNp { static constexpr int value = MODE == 2 ? 8 : MODE == 4 ? 1 : MODE == 5 ? 2 : 4; };

// MODE picks the wave shape.  BTL = candidate points per lane, SLOTS = candidate slots per wave:
//   MODE 2: 16 markers x 4 slots x 2 points  (NP = 8)
//   MODE 3: 2 x 16 markers x 2 slots x 2 points (NP = 4): the wave takes TWO micro-tiles, so a
//           4-point launch (a Nelder-Mead iteration) amortises the per-run bookkeeping over two
//           points per lane like MODE 2 does, instead of one.
//   MODE 4: 4 x 16 markers x 1 slot x 1 point (NP = 1): a single-point evaluation (a caller's own
//           optimiser, Initialize, LLK0) does a quarter of the work of a 4-point launch instead of
//           evaluating the point four times.
//   MODE 5: 4 x 16 markers x 1 slot x 2 points (NP = 2): cohort steps of a search that speculates on
//           one extra point per iteration (multi-sample kernel only).
// A launch evaluates groups of NP points (num_valid of them real; the rest replicate the last).
// The body is shared by the single-sample kernel (blk = blk, nblk = nblk) and
// the multi-sample kernel (blk/nblk = this workgroup's index among its sample's workgroups).
// Parameter rows passed inside the kernel-argument segment (host-pointer path with few
// points): saves the PCIe round trip of reading them from mapped host memory.
struct InlinePoints {
    int count;                       // doubles valid in v (0 = read from the pointer)
    double v[kInlinePointDoubles];
};

// A wave of the workgroup that spends the tile phase on something else (the resident kernel's control wave:
// resident_kernel.inc).  on_block: this workgroup has such a wave (wave 0); mine: this wave is it.  Only with
// the dynamic work queue (eval_is_dynamic): the other waves then start on items 0..nwave-2 and pull the rest.
struct NoHook {
    __device__ bool on_block() const { return false; }
    __device__ bool mine() const { return false; }
    __device__ void run() {}
    __device__ bool keep_etab() const { return false; }     // (the 2^(j/64) table of an earlier call is still in LDS)
    __device__ bool prim_in_lds() const { return false; }   // the primary-code records live in LDS across calls ...
    __device__ bool keep_prim() const { return false; }     // ... and an earlier call left them there
    __device__ double* sum_stage() const { return nullptr; } // where workgroup 0 stages the partial sums (nullptr: over the dead tables)
    __device__ uint32_t cache_rec() const { return 0u; }    // LCACHE: LDS byte address of this workgroup's tile records
    __device__ unsigned int* sync_word() const { return nullptr; }   // a zeroed LDS word: the hook wave skips the prologue (see eval_body)
    __device__ bool collect_only() const { return false; }  // this workgroup owns no tiles: it collects the other workgroups' sums (and hosts the hook wave)
    __device__ bool no_collect() const { return false; }    // the tagged sets are collected by such a workgroup, not by workgroup 0
};
// The waves of a workgroup pull (tile, group) items through the LDS queue (per-item result slots) when there
// are at most dyn_limit of them per wave; else the static deal (cohort launches).
__host__ __device__ __forceinline__ bool eval_is_dynamic(const DeviceLayout& L, uint32_t nblk, int nwave, int ngrp)
{
    const uint32_t max_tiles_blk = owned_most(L.pd ? 1 : 0, (uint32_t)L.num_mt, nblk);
    return max_tiles_blk * (uint32_t)ngrp <= (uint32_t)(L.dyn_limit * nwave);
}

// STREAM: the launch reads its samples' run lists from HBM (cohort steps) rather than from L2: the prefetch never
// runs past a tile's own rows then (see the read loop).
// QUEUE: 1 = the launch is known (on the host, by eval_is_dynamic) to take its work items through the LDS queue, 0 = the
// static deal, -1 = decided in the kernel.  The single-sample kernels are compiled for both: with the other way's code
// gone a 48-point launch is 1.8 % shorter and a search round 5 % (fewer scalar registers spilled to vector lanes).
// KSEL: --NumPC when it is 2 (the reference's default) or 4 (its usual setting) AND the context has no known-allele-
// frequency column (the usual case: AF from UD x PC), else 0 = both read from the layout: the guards and address
// multiples of the projection and the known-AF tests go at compile time (+2.6 % on the 48-point launch).
// LCACHE (the resident search kernel): this workgroup's run lists and tile records were copied to LDS when the kernel
// started (a workgroup owns the same micro-tiles in every round), so a round's read loops begin without the two dependent
// trips to L2 (tile record, then its first rows) and never wait for a row again.
// ESH: log2 of the byte stride between the entries of exp_nonpos's table (8: conflict-free; 6: the compact copy).
// (Measured and dropped over the rounds, all bit-identical: a software-pipelined item loop, the next item drawn a whole item
// early, two half-sized workgroups per CU; of table reads that run ahead of their multiplies: a ring that carries reads ACROSS
// the steps of the run-word kernel -- rounds 3 and 4: 128 registers and spills, slower -- and eight to ten reads in flight in
// the search round's single item per wave -- round 5: equal, that regime is bound by the deepest wave's latency.  Kept: the
// probability-domain walk requests a row word's twelve reads before it multiplies, READS_AHEAD below -- HISTORY.md.
// Variants of the switches below that were built, measured and retired, each one bit-identical to what is kept:
//   * reads ahead a STEP at a time (six reads, then their multiplies): 45.22 us per 48-point step against 45.03 a row at a
//     time (profiles/r09/ab_reads_ahead.txt);
//   * the tile's last row also requesting the epilogue's projection coefficients: all 2 k quads spill at --NumPC 4 (128
//     registers, 120 B of scratch: never timed), those of the first two components 44.40 us against 43.75 without them
//     (profiles/r10/ab_item_head.txt);
//   * the next item's rows fetched under the epilogue WITHOUT fixed ring registers: 43.97 us against 43.75 with them
//     (profiles/r10/ab_item_head.txt);
//   * the queue's draw riding the last row's reads, behind them or in front: SLOWER by 0.41 and 0.36 us -- the tile's last row
//     on its own costs more than the draw's trip --, and the coefficients requested behind the last row's multiplies: 0.05 us,
//     no effect, the waves fill each other's epilogue holes (profiles/r11/ab_epi_trips.txt);
//   * the split launch's short head and short tail each without the other: both are kept (profiles/r07/ab_split_head_tail.txt);
//   * wave w of a search round taking item w (no SIMD-balanced first deal) and the resident kernel's control wave starting
//     behind the table build: see the first deal and the prologue below;
//   * the host's flag as a relaxed store behind acknowledged result stores: the release store costs nothing measurable and is
//     the code (profiles/r06/ab_flag_release.txt).)
// ITEM_AHEAD (the 8-point probability-domain shape on the queue; the split launch takes it): where a wave gets its NEXT item
// from.  false: at the item's head -- the draw, the tile's record, the list's first rows: three dependent trips before the first
// table read.  true: the draw and the record's request behind the present item's last row, the rows 0, 1, 2 of the list behind
// its epilogue; the next iteration starts from those registers (see the item loop), and the ring of row words has FIXED
// registers: a row's two table addresses are taken from its word before the refill is loaded into the same register, so no loop
// of the walk begins or ends with a copy of a register that is being loaded.  -2.6 % on the 48-point launch; on the plain
// 8-point launch faster too, but not by three times the spread (HISTORY.md).
// (The item drawn a WHOLE item early -- round 4, above -- cost balance; this draw is one epilogue early.)
// EPI_X8 (the same shape; the split launch takes it): the tile butterfly's exchange over marker bit 3 as DPP moves and
// v_permlane16_swap (lane_pair8_u32) instead of ds_bpermute -- six instructions per item off the LDS pipe, which the other
// fifteen waves' row reads fill: -1.2 % on the 48-point launch, no effect on the plain 8-point launch (HISTORY.md).
// EPI_SCATTER (needs EPI_X8; the split launches take it): the tile butterfly as a reduce-scatter, ONE point per lane.  Marker bit 3
// is the lane's row parity, so after the exchange over it an even 16-lane row only ever needs point 0 and an odd row point 1:
// the odd rows swap their quads in place as for EPI_X8, both points' dwords, and v_permlane16_swap takes point 0's dword and
// point 1's as its two operands (lane_scatter8_u32) -- an even-row lane then holds {its own point 0, its partner's}, the odd-row
// lane sixteen above it {that even lane's point 1, its partner's}: one multiply and one add per lane where there were two, the
// steps over bits 2, 1, 0 on one value, and the lanes of marker 0 AND the lanes sixteen above them store, each one point, in one
// ds_write_b128.  The same two factors into every multiply: the same bits.  With it marker_lk's `lk > 0 ? lk : 1.0` moves into
// the branch of the tiny values (a value of at least 2^-960 is positive; a NaN takes the branch): HISTORY.md, profiles/r13.
// ADDR_SCALAR (needs ITEM_AHEAD; the split launches take it): what the item loop computes per lane although it is the same in every
// lane, or a scalar plus a constant of the lane, goes to the scalar unit.  The nine per-marker constants are loaded through buffer
// descriptors, one per column, built by scalar instructions from the layout's pointers (the opaque-scalar base of the other
// kernels compiles to a 64-bit vector add in front of every load); the list words through one descriptor with the lane's word in
// the vector offset and the row -- the tile's first row, one v_readfirstlane per item, plus the row in the tile -- in the scalar
// offset; the tile's record is decoded by scalar shifts and selects; and the queue is drawn by lane 0 alone under an exec mask of
// one bit, where the compiler's wave-aggregated atomic counts lanes for an add that only ever has one.  The same addresses, no
// arithmetic on a likelihood: the same bits.  44 vector instructions fewer in the item loop of llk_eval_split6_kernel<4>
// (tools/item_census.py: 511 -> 467; HISTORY.md, profiles/r14).
// COEF_DPP (the split launch six ways at --NumPC 4 and 2): a workgroup of such a launch has ONE point group, so a lane's slot and
// its two points never change, and the epilogue's 2 k ds_read_b128 of projection coefficients fetched the same bytes into the same
// lane for every item.  The coefficients are loaded once, behind the prologue's last barrier, into the lanes of the 16-lane DPP rows
// -- lane i of a row holds coefficient i of a slot, ptq's own order [2 k][2 points] --, and each FMA of the projection takes its
// coefficient from its lane of the reader's row: v_fmac_f64_dpp with row_newbcast, the one DPP control FP64 instructions take.  A
// row holds the lanes of TWO slots (see the load in front of the item loop), so each FMA exists twice, under complementary bank
// masks.  The same two factors into the same addend in the same order: the same bits.  Four resident registers (two at --NumPC 2)
// for the 32 that the reads landed in; 2 k LDS instructions fewer and 4 k vector instructions more per item (HISTORY.md, profiles/r15).
// PD: a probability-domain context (DeviceLayout::pd; llk_kernels.h, kMaxPow): the table holds P^n rows of class ref only,
// a marker's list is one 16-bit row offset per step, ref steps first and alt steps behind them; the six sums are PRODUCTS,
// class alt multiplies them with the row read the other way round (g -> 2 - g, h:164-177: T[alt][q][g1][g2] is T[ref][q][2-g1][2-g2]),
// and the epilogue needs no exponential.  Only for contexts whose markers cannot underflow that way (Context::create).
// READS_AHEAD: how a row word of the probability-domain walk orders its table reads and its multiplies (walk_pd).  false: as the
// scheduler likes it -- four landing quads, a step's six reads in three dependent round trips.  true: a row at a time -- both
// steps' twelve reads, then their multiplies.  The split, plain and narrow launches take it; the resident search kernel,
// which spills already, spills more with it and keeps the old order (HISTORY.md), and so do the cohort kernels and the
// pass-per-group kernel, some of which spill with it.
// SPLIT (a probability-domain launch of more points than a workgroup's LDS holds tables for -- a dictionary of ~100 rows and 48
// points): the workgroups come in PAIRS that share their tiles and split the point groups -- workgroup 2v takes the first
// half of the groups, 2v + 1 the second, both over the tiles of the VIRTUAL blocks v and v + grid / 2, i.e. over exactly the
// tiles two workgroups of a plain launch own.  A tile's product still has its own slot, a virtual block's slots are
// multiplied in the same order and its sum goes to the same word of the partial sums as in a plain launch of this grid:
// the same bits, and no second pass over the tiles (llk_eval_passes_kernel: +4 us per pass at C3).  In general SPLIT = S
// workgroups make a set: workgroup S v + j takes share j of the groups over the tiles of the virtual blocks v + i * grid / S.
// S = kMaxGroups (a launch of six groups on a grid that is a multiple of six): every workgroup has exactly ONE group -- half the
// table entries per workgroup of S = 3, no group arithmetic per item (ONEGRP), the same items, slots and sums.
//
// A kernel's configuration of the body: a type that derives from EvalConfig, names its MODE and sets what differs (the members
// are explained above; W16: the cohort steps' 16-bit run lists / 8-bit step lists).
struct EvalConfig {
    static constexpr bool W16 = false, STREAM = false, LCACHE = false, PD = false;
    static constexpr int QUEUE = -1, KSEL = 0, ESH = 8, SPLIT = 0;
    static constexpr bool READS_AHEAD = false, ITEM_AHEAD = false, EPI_X8 = false, EPI_SCATTER = false, ADDR_SCALAR = false;
    static constexpr bool COEF_DPP = false;
};
template <class Config, class Hook = NoHook>
__device__ __forceinline__ void
eval_body(const DeviceLayout& L, const double* ip_v, const int ip_count, const double* __restrict__ points, int num_valid,
          double* __restrict__ partials, double* __restrict__ llk_out,
          unsigned int* __restrict__ ticket, unsigned long long* __restrict__ done_flag,
          unsigned long long done_seq, const uint32_t blk, const uint32_t nblk,
          unsigned int* __restrict__ batch_done, unsigned int batch_active, const int ngrp_in,
          const unsigned long long tag, const Schedule sch, const bool coherent_points = false,
          const int tid_in = -1, const double* lds_rows = nullptr /* the parameter rows, already in LDS */,
          Hook hook = Hook())
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int MODE = Config::MODE, QUEUE = Config::QUEUE, KSEL = Config::KSEL, ESH = Config::ESH, SPLIT = Config::SPLIT;
    constexpr bool W16 = Config::W16, STREAM = Config::STREAM, LCACHE = Config::LCACHE, PD = Config::PD;
    static_assert(MODE >= 2 && MODE <= 5, "wave shapes 2..5");
    static_assert(!PD || ESH == 8, "probability-domain contexts have no exp table");
    static_assert(!(PD && W16) || ((MODE == 4 || MODE == 5) && STREAM), "8-bit step lists: cohort steps of one and two points");
    static_assert(!SPLIT || (PD && MODE == 2 && QUEUE == 1 && !STREAM && !LCACHE), "split launches: the 8-point shape on the queue");
    static_assert(SPLIT == 0 || SPLIT == 2 || SPLIT == 3 || SPLIT == kMaxGroups, "sets of two, three or kMaxGroups workgroups");
    static_assert(SPLIT + 1 <= kTicketScratchWord, "a ticket per share and one word to count the shares");
    constexpr int OSH = PD ? 1 : 0;             // a workgroup owns pairs of neighbouring micro-tiles (owned_tile)
    // the launch is known to carry ONE group of points (every shape but the 8-point one always does; cohort steps too):
    // the group loops and the item -> (group, unit) division go at compile time
    // (SPLIT == 6: the launcher takes sets of six only for launches of six groups -- a workgroup has exactly one)
    constexpr bool ONEGRP = MODE != 2 || STREAM || SPLIT == kMaxGroups;
    constexpr int KAF = KSEL > 0 ? 0 : -1;      // 0: no known-AF column, known at compile time
    constexpr int BTL = MODE == 4 ? 1 : 2;
    constexpr int TPW = MODE == 3 ? 2 : (MODE == 4 || MODE == 5) ? 4 : 1;   // micro-tiles per wave
    constexpr int SLOTS = 4 / TPW;                           // candidate slots per wave
    constexpr int NP = SLOTS * BTL;
    constexpr bool kReadsAhead = PD && Config::READS_AHEAD;    // walk_pd requests a row's table reads before it multiplies
    static_assert(!Config::EPI_SCATTER || Config::EPI_X8, "the reduce-scatter is the exchange over marker bit 3 of EPI_X8, two operands");
    static_assert(!(Config::ITEM_AHEAD || Config::EPI_X8) ||
                      (PD && MODE == 2 && QUEUE == 1 && !STREAM && !LCACHE && !W16 && std::is_same<Hook, NoHook>::value),
                  "items requested ahead, the exchange over marker bit 3: the 8-point probability-domain shape on the queue");
    constexpr bool kAhead = Config::ITEM_AHEAD && (kAblate & (kAblNoReads | kAblNoRowLoads)) == 0;      // (see the item loop)
    constexpr bool kEpiX8 = Config::EPI_X8 && (kAblate & (kAblNoReads | kAblNoMul | kAblNoEpi)) == 0;
    constexpr bool kEpiScatter = Config::EPI_SCATTER && kEpiX8;      // (one point per lane behind the exchange over marker bit 3)
    static_assert(!Config::ADDR_SCALAR || Config::ITEM_AHEAD, "scalar row offsets: the record's words are taken where the rows ahead are requested");
    constexpr bool kAddrScalar = Config::ADDR_SCALAR && kAhead;      // (the item loop's uniform address arithmetic on the scalar unit)
    // (the projection's coefficients resident in a DPP row's lanes: one group for the whole launch, two points per lane, --NumPC 4 or 2)
    constexpr bool kCoefDpp = Config::COEF_DPP && ONEGRP && PD && MODE == 2 && BTL == 2 && (KSEL == 4 || KSEL == 2) && (kAblate & kAblNoEpi) == 0;
    // (items ahead: every row but a tile's first is walked from its two table ADDRESSES, taken from the ring's word before that
    // register is refilled -- row_step and walk_pd, kAt)
    constexpr bool kFixedRing = kAhead && kReadsAhead && (kAblate & kAblNoMul) == 0;
    // (the run-word kernels of the static deal in the paired shapes: the layout's four sizes in scalar registers of their own.
    // Under those kernels' scalar pressure the register allocator gave up the {num_code, row_bytes, num_prim, num_mt} quad of the
    // kernel arguments, loaded it again at each of six uses and left the quad's spill slot behind: scratch memory set up for
    // every launch that no instruction touches)
    constexpr bool kOwnSizes = QUEUE == 0 && KSEL == 0 && !PD && !STREAM && (MODE == 3 || MODE == 4) && std::is_same<Hook, NoHook>::value;    // llk_eval_kernel<3, 0, 0, false>, <4, 0, 0, false>: no others
    int own_num_code = 0, own_row_bytes = 0, own_num_prim = 0, own_num_mt = 0;
    if constexpr (kOwnSizes) {
        own_num_code = L.num_code; own_row_bytes = L.row_bytes; own_num_prim = L.num_prim; own_num_mt = L.num_mt;
        asm volatile("" : "+s"(own_num_code), "+s"(own_row_bytes), "+s"(own_num_prim), "+s"(own_num_mt));
    }
    const auto l_num_code = [&] { if constexpr (kOwnSizes) return own_num_code; else return L.num_code; };
    const auto l_row_bytes = [&] { if constexpr (kOwnSizes) return own_row_bytes; else return L.row_bytes; };
    const auto l_num_prim = [&] { if constexpr (kOwnSizes) return own_num_prim; else return L.num_prim; };
    const auto l_num_mt = [&] { if constexpr (kOwnSizes) return own_num_mt; else return L.num_mt; };
    const int row_bytes = MODE == 2 ? kRowBytesWide : l_row_bytes();      // (the 8-point shape needs the wide rows: the launcher sees to it)
    const int RS = row_bytes >> 3;              // doubles per table row (>= 6 * NP + 2)
    const int nrow = l_num_code() + 1;
    const int nthread = blockDim.x;
    const int nwave = nthread >> 6;
    const int k = KSEL > 0 ? KSEL : L.num_pc;
    const int stride = 2 * k + 1;
    // A launch carries ngrp groups of NP points; each group has its own table and the
    // (tile, group) pairs are the work items, so a bigger batch re-reads the pileup from
    // L2 per group but pays launch, prologue and reduction once.
    // (SPLIT = S workgroups share their tiles: this workgroup's share of the launch's groups, the points before them, and its S
    // virtual blocks vb0 + j * vstep)
    constexpr int NVS = SPLIT ? SPLIT : 1;      // virtual blocks per workgroup
    const int g_per = SPLIT ? (ngrp_in + NVS - 1) / NVS : ngrp_in;
    const int g_lo = SPLIT ? (int)(blk % (uint32_t)NVS) * g_per : 0;
    const int ngrp = ONEGRP ? 1 : SPLIT ? (ngrp_in - g_lo < g_per ? ngrp_in - g_lo : g_per) : ngrp_in;      // (the launcher sees to it that none is empty)
    const int p_off = g_lo * NP;
    const uint32_t vstep = SPLIT ? nblk / (uint32_t)NVS : 0u, vb0 = SPLIT ? blk / (uint32_t)NVS : blk;
    const double* const known_af_p = KAF == 0 ? nullptr : L.known_af;
    const int NPT = NP * ngrp;                  // points of this launch
    constexpr int kEtabCopies = (1 << ESH) / 8, kEtabDoubles = PD ? 0 : 64 * kEtabCopies;
    constexpr int kLtabDoubles = PD ? 0 : kLogTabDoubles;
    double* etab = lds;                         // [64][32] exp_nonpos's 2^(j/64), bank-replicated; at LDS address 0
    double* ltab = lds + kEtabDoubles;          // [128] {1 / c, log c} of log_tab
    double* tab = ltab + kLtabDoubles;          // [ngrp][nrow][RS]  (PD: neither table above: this one is at address 0)
    double* red = tab + ngrp * nrow * RS;       // [virtual blocks][NPT] block sums; then the work-queue counter
    unsigned int* queue = reinterpret_cast<unsigned int*>(red + NVS * NPT);
    double* pts = red + NVS * NPT + 2;          // [NPT][2k+1] this launch's parameter rows
    // the PCs again, as the epilogue reads them: [group][slot][2k][BTL] -- a lane's BTL points side by
    // side, so one ds_read_b128 (4 LDS cycles) brings a coefficient of both points where two
    // strided 8-byte reads (ds_read2_b64: 8 cycles) did
    double* ptq = pts + (size_t)NPT * stride + ((NPT * stride) & 1);
    const size_t prim_off = (size_t)(ptq - lds) + (size_t)NPT * 2 * k;
    double2* prim_lds = reinterpret_cast<double2*>(lds + prim_off + (prim_off & 1));   // [num_prim], 16-B aligned
    double* tile_llk = reinterpret_cast<double*>(prim_lds + l_num_prim());   // [work items or waves][NP] {mantissa, exponent}

    // (tid_in: the resident kernel passes its thread index through an opaque register each round,
    // so that nothing derived from it is hoisted out of the round loop and kept alive across it)
    const int tid = tid_in >= 0 ? tid_in : (int)threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform, and the compiler knows it)
    int m, g4;
    lane_map(lane, m, g4);
    const int g = g4 & (SLOTS - 1);              // candidate slot
    const int half = TPW == 1 ? 0 : g4 / SLOTS;  // which of the item's TPW micro-tiles
    // profiling aid: 100 MHz wall-clock stamps per workgroup (stamps pointer null normally)
    // (kernel_debug.h: VB2_STAMP_ROUND; the accumulated figures cover every round either way)
    const bool stamp_this = VB2_STAMP_ROUND == 0 || (unsigned)(tag & 0xffffffffull) == (unsigned)VB2_STAMP_ROUND;
    unsigned long long* stamps = (VB2_STAMPS_OF(L) && stamp_this) ? VB2_STAMPS_OF(L) + (size_t)blk * 8 : nullptr;
    if (stamps && tid == 0) { stamps[0] = wall_clock64(); stamps[4] = 0; }
    if constexpr (SPLIT != 0) {
        // (word 7 = 1 + the id of the XCD this workgroup runs on, for the finishing spread by XCD -- tools/stamps.py; not in the
        // workgroups 0, 20 and 21, whose word 7 the search rounds' accumulated figures use)
        if (stamps && tid == 0 && blk != 0u && blk != 20u && blk != 21u) {
            unsigned int xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            stamps[7] = 1ull + (xcc & 15u);
        }
    }

    // A workgroup that owns no tiles (the resident kernel's extra workgroup for the control wave: Hook::collect_only): nothing of
    // the evaluation -- its hook wave does its work, then all of it collects the tile workgroups' sums below.
    const bool collect_only = hook.collect_only();
    if (collect_only && hook.mine()) hook.run();
    if (!collect_only) {
    const bool hook_blk = hook.on_block(), hook_mine = hook.mine();
    // A workgroup with a hook wave (the resident kernel's control wave: wave 0 of workgroup 0) in a probability-domain search
    // round: that wave starts on its own work AT ONCE -- it builds no table entries and does not come to the prologue's barriers,
    // which the other waves replace by a counter in LDS (hook.sync_word(), zero at the round's start).  Its work is the round's
    // longest dependent chain (resident_kernel.inc: control_tile_phase, ~6 us): begun behind the table build it ended 1.5 us
    // after every other workgroup had its sums in.
    unsigned int* const soft_word = PD ? hook.sync_word() : nullptr;
    const bool soft = hook_blk && soft_word != nullptr;
    if (soft && hook_mine) hook.run();
    const int ptid = !soft ? tid : hook_mine ? 0x3fffffff : tid - 64, pnthread = soft ? nthread - 64 : nthread;
    unsigned int soft_gen = 0;
    auto prologue_sync = [&]() {
        if (!soft) { __syncthreads(); return; }
        if (hook_mine) return;
        soft_gen += (unsigned int)(nwave - 1);
        // (a wave's LDS operations are performed in order: its table entries are in place when its arrival is counted)
        if (lane == 0) __hip_atomic_fetch_add(soft_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(soft_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < soft_gen) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    };
    // SPLIT: a thread's table entries need its record and the alphas of its groups, nothing else -- requested straight from
    // global memory here, in one burst with the staging loads below, so that the table is built from registers and does not
    // wait at a barrier for the staged rows and records to be read back (the resident kernel's early_table, for launches of
    // many groups).  The same numbers into the same expressions.
    constexpr int kTabSide = 3;                       // groups whose entries a thread builds side by side (see the table loop)
    constexpr int kTabN = ONEGRP ? 1 : kTabSide;      // ... of which a workgroup with one group has one
    const int ntab_split = (kAblate & kAblNoTable) ? 0 : (PD ? l_num_prim() - L.num_pair : l_num_prim()) * 6 * NP;
    auto table_inputs = [&](int e, int g0, double2& rec_o, double* al_o) {
        const int pi = e / (6 * NP);
        const int bb = (e - pi * (6 * NP)) / 6;
        rec_o = L.prim[pi];
#pragma unroll
        for (int u = 0; u < kTabN; ++u) {
            const int ge = g0 + u < ngrp ? g0 + u : ngrp - 1;
            const int b = ge * NP + bb;
            const int idx = (p_off + b < num_valid ? p_off + b : num_valid - 1) * stride + 2 * k;
            al_o[u] = (kAblate & kAblNoMap) ? 0.01 * (double)(1 + idx % 7) : points[idx];
        }
    };
    double2 tin_rec = make_double2(0.0, 0.0);
    double tin_al[kTabSide] = {0.0, 0.0, 0.0};
    if constexpr (SPLIT != 0)
        if (ptid < ntab_split) table_inputs(ptid, 0, tin_rec, tin_al);
    if (ptid == 0) *queue = (unsigned int)(nwave - (hook_blk ? 1 : 0));      // waves start on tiles 0..nwave-1
    // parameter rows -> LDS with one coalesced load (they may live in mapped host memory)
    for (int e = ptid; e < NPT * stride; e += pnthread) {
        const int b = e / stride;
        const int src = p_off + b < num_valid ? p_off + b : num_valid - 1;
        const int idx = src * stride + (e - b * stride);
        // resident mode: the rows were just written by another workgroup -> L1-bypassing loads
        const double v = (kAblate & kAblNoMap) ? 0.01 * (double)(1 + idx % 7)
                         : lds_rows ? lds_rows[idx]
                         : ip_count > 0 ? ip_v[idx]
                         : coherent_points ? __hip_atomic_load(&points[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                           : points[idx];
        pts[e] = v;
        const int c = e - b * stride;                       // 0..2k-1: a PC coordinate, 2k: alpha
        if (c < 2 * k) ptq[((b / BTL) * 2 * k + c) * BTL + (b % BTL)] = v;
    }
    // 2^(j/64) table of exp_nonpos, one copy per pair of LDS banks (see there)
    // (entry j = e / 32 is the same for a half-wave: two SCALAR loads per step, no vector-memory
    // round trip before the first barrier)
    if (!PD && !hook.keep_etab() && tid < kLogTabDoubles / 2)
        reinterpret_cast<double2*>(ltab)[tid] = kLogTabRows[tid];
    if (!PD && !hook.keep_etab())
        for (int jb = 2 * wave; jb < 64; jb += 2 * nwave) {
            const double t0 = kExp2Tab[jb], t1 = kExp2Tab[jb + 1];
            const double tv = lane < 32 ? exp_tab_entry(t0, jb) : exp_tab_entry(t1, jb + 1);
            if constexpr (ESH == 8) etab[jb * 32 + lane] = tv;
            else if ((lane & 31) < kEtabCopies) etab[(jb + (lane >> 5)) * kEtabCopies + (lane & 31)] = tv;
        }
    // With several groups a thread builds several table entries: the primary-code records (a
    // few dozen) go to LDS first so that the loop below does not wait on a global load per
    // entry.  With one group each thread builds about one entry and loads its record directly.
    // (the resident kernel keeps them in LDS from its first round on: a round's table then starts without a trip to L2)
    const bool prim_kept = hook.prim_in_lds() && hook.keep_prim();
    const bool staged = ngrp > 1 || (hook.prim_in_lds() && !prim_kept) || (PD && L.num_pair > 0 && !prim_kept);      // (pair rows: their records from LDS)
    if (staged)
        for (int e = ptid; e < l_num_prim(); e += pnthread) prim_lds[e] = L.prim[e];
    // A search round (its rows are in LDS since the round's staging barrier) builds its one table without waiting
    // for the copies above: the table needs the alphas only, and takes them from the staged rows (-0.6 us per
    // round; the same for launches whose rows come with the kernel arguments: no gain, not kept).
    const bool early_table = lds_rows != nullptr && !staged;
    if (!early_table && SPLIT == 0) prologue_sync();
    if (stamps && (soft ? ptid : tid) == 0) stamps[1] = wall_clock64();      // (SPLIT: the staging stores are issued, nothing waited for)

    // ---- per-alpha table, off-diagonal pairs only (h:213-229) ----
    // Class alt is class ref with the genotypes mirrored (g -> 2-g, h:164-177): the entry of
    // (alt, q) for pair p IS the entry of (ref, q) for pair 5-p, the same expression on the same
    // numbers.  So only the "primary" codes are computed -- every ref code, and alt codes whose
    // quality has no ref code in the data -- and the thread that computes a ref entry also stores
    // it into the alt twin's row: half the logarithms, and no barrier in between.
    // (a thread's entries for the different groups are independent: computed side by side so
    // that their long dependent logarithm chains overlap)
    const uint32_t ltab_addr = lds_byte_addr(ltab);
    const int num_single = PD ? l_num_prim() - L.num_pair : l_num_prim();
    if constexpr (SPLIT != 0) {
        // (the loop below on inputs that are in registers: the next step's are requested before this step's entries are computed)
        int e = ptid, g0 = 0;
        while (e < ntab_split) {
            int e_n = e, g0_n = g0 + kTabN;
            if (g0_n >= ngrp) {
                g0_n = 0;
                e_n = e + pnthread;
            }
            double2 rec_n = tin_rec;
            double al_n[kTabSide] = {tin_al[0], tin_al[1], tin_al[2]};
            if (e_n < ntab_split) table_inputs(e_n, g0_n, rec_n, al_n);
            const int pi = e / (6 * NP);
            const int bp = e - pi * (6 * NP);
            const int bb = bp / 6, p = bp - bb * 6;
            (void)bb;
            const uint32_t pr = (uint32_t)__double_as_longlong(tin_rec.y);
            const int dc = (int)(pr & 0xffffu), twin = (int)(pr >> 16);
            int g1, g2;
            pair_of(p, g1, g2);
            double v3[kTabSide], r3[kTabSide];
            double* cell3[kTabSide];
#pragma unroll
            for (int u = 0; u < kTabN; ++u) {
                const int ge = g0 + u < ngrp ? g0 + u : ngrp - 1;      // (past the last group: the last one again, the same values)
                v3[u] = prob_entry(tin_al[u], tin_rec.x, g1, g2);
                r3[u] = v3[u];
                cell3[u] = tab + (size_t)ge * nrow * RS + dc * RS + bp;
                *cell3[u] = r3[u];
            }
            const int kq = twin & 0xff, pstride = RS * (int)(int8_t)(twin >> 8);
            for (int n = 1; n < kq; ++n) {
#pragma unroll
                for (int u = 0; u < kTabN; ++u) {
                    r3[u] *= v3[u];
                    cell3[u] += pstride;
                    *cell3[u] = r3[u];
                }
            }
            tin_rec = rec_n;
#pragma unroll
            for (int u = 0; u < kTabN; ++u) tin_al[u] = al_n[u];
            e = e_n;
            g0 = g0_n;
        }
    } else
    for (int e = ptid; e < ((kAblate & kAblNoTable) ? 0 : num_single * 6 * NP); e += pnthread) {
        const int pi = e / (6 * NP);
        const int bp = e - pi * (6 * NP);
        const int bb = bp / 6, p = bp - bb * 6;
        const double2 rec = (staged || prim_kept) ? prim_lds[pi] : L.prim[pi];       // {signed pErr, code | twin << 16}
        const uint32_t pr = (uint32_t)__double_as_longlong(rec.y);
        const int dc = (int)(pr & 0xffffu), twin = (int)(pr >> 16);
        int g1, g2;
        pair_of(p, g1, g2);
        // W16 (cohort steps on the 16-bit run lists): the run word's count field decodes to the double 2 * n with ONE
        // byte permute (see the read loop), so the table holds T / 2 -- both scalings are exact (powers of two), and
        // fma(2n, T/2, acc) rounds the same real number as fma(n, T, acc): bit-identical to the 32-bit lists.
        // (the groups one after the other in a rolled loop: side by side -- six logarithms' chains interleaved -- the
        // unrolled body held every group's temporaries and constants at once and spilled scalar registers to vector lanes;
        // it cost 430 vector instructions per thread of a 48-point launch where this costs 285: headline +0.8 %, 118 codes +2.2 %)
        if constexpr (PD && !ONEGRP) {
            // (probability domain, several groups: an entry is a dozen dependent FP64 operations and K dependent multiplies -- no
            // logarithm's forty --, so THREE groups' entries side by side cost few registers and hide each other's latencies:
            // the tables of a split launch's workgroup 1.8 -> 1.6 us (127 KB of LDS stores: ~0.75 us at the LDS's store rate),
            // the 48-point launch 51.35 -> 50.6 us on one box)
            constexpr int kSide = 3;
            for (int g0 = 0; g0 < ngrp; g0 += kSide) {
                double v3[kSide], r3[kSide];
                double* cell3[kSide];
#pragma unroll
                for (int u = 0; u < kSide; ++u) {
                    const int ge = g0 + u < ngrp ? g0 + u : ngrp - 1;      // (past the last group: the last one again, the same values)
                    v3[u] = prob_entry(pts[(ge * NP + bb) * stride + 2 * k], rec.x, g1, g2);
                    r3[u] = v3[u];
                    cell3[u] = tab + (size_t)ge * nrow * RS + dc * RS + bp;
                    *cell3[u] = r3[u];
                }
                const int kq = twin & 0xff, pstride = RS * (int)(int8_t)(twin >> 8);      // (record: first row | K << 16 | rows from P^n to P^(n+1), a signed byte, << 24)
                for (int n = 1; n < kq; ++n) {
#pragma unroll
                    for (int u = 0; u < kSide; ++u) {
                        r3[u] *= v3[u];
                        cell3[u] += pstride;
                        *cell3[u] = r3[u];
                    }
                }
            }
        } else
#pragma clang loop unroll(disable)
        for (int grp_e = 0; grp_e < ngrp; ++grp_e) {
            const double alpha_e = early_table ? lds_rows[(bb < num_valid ? bb : num_valid - 1) * stride + 2 * k]
                                               : pts[(grp_e * NP + bb) * stride + 2 * k];
            double* gtab = tab + (size_t)grp_e * nrow * RS;
            if constexpr (PD) {
                // record pi = a QUALITY: {pErr, first row | K << 16}: its rows P^1 .. P^K follow each other, one multiply
                // apiece (class alt reads the same rows mirrored)
                const double v = prob_entry(alpha_e, rec.x, g1, g2);
                double r = v;
                double* cell = gtab + dc * RS + bp;
                // (shapes of at most four points: the row's second half holds its mirror image, pair p <-> 5 - p, where the
                // alt steps' offsets point -- kPdAltOffset)
                constexpr int kMir = kPdAltOffset / 8;
                const int mir = kMir + bb * 6 + (5 - p) - bp;
                *cell = r;
                if constexpr (NP <= 4 && STREAM) cell[mir] = r;
                const int kq = twin & 0xff, pstride = RS * (int)(int8_t)(twin >> 8);      // (record: first row | K << 16 | rows from P^n to P^(n+1), a signed byte, << 24)
                for (int n = 1; n < kq; ++n) {
                    r *= v;
                    cell += pstride;
                    *cell = r;
                    if constexpr (NP <= 4 && STREAM) cell[mir] = r;
                }
            } else {
                const double v = table_entry(alpha_e, rec.x, g1, g2, ltab_addr);
                const double tv = W16 ? 0.5 * v : v;
                gtab[dc * RS + bp] = tv;
                if (twin != 0xffff) gtab[twin * RS + bb * 6 + (5 - p)] = tv;
            }
        }
    }
    for (int e = ptid; e < ngrp * RS; e += pnthread) {                // padding code: zero rows (PD: ones)
        const int grp_e = e / RS;
        tab[((size_t)grp_e * nrow + l_num_code()) * RS + (e - grp_e * RS)] = PD ? 1.0 : 0.0;
    }
    if constexpr (PD) {
        // ---- pair rows (PdDict): the product of two of the rows above, entry by entry -- one record per row
        // {bits: row a | row b << 16, bits: the row}, from LDS ----
        for (int level = 0; level < 2 && L.num_pair > 0 && !(kAblate & kAblNoTable); ++level) {
            // (level 1: products of two rows the records of this kind made -- windows of three and four qualities)
            const int nrec = level == 0 ? L.num_pair - L.num_pair2 : L.num_pair2;
            if (nrec == 0) break;
            prologue_sync();
            const double2* const prec = prim_lds + num_single + (level == 0 ? 0 : L.num_pair - L.num_pair2);
            for (int e = ptid; e < nrec * 6 * NP; e += pnthread) {
                const int pi = e / (6 * NP);
                const int bp = e - pi * (6 * NP);
                const double2 rec = prec[pi];
                const uint32_t ab = (uint32_t)__double_as_longlong(rec.x), dst = (uint32_t)__double_as_longlong(rec.y);
                const int ra = (int)(ab & 0xffffu) * RS + bp, rb = (int)(ab >> 16) * RS + bp, rd = (int)dst * RS + bp;
                constexpr int kMir = kPdAltOffset / 8;
                const int bb = bp / 6, p = bp - bb * 6;
                const int mir = kMir + bb * 6 + (5 - p) - bp;
#pragma clang loop unroll(disable)
                for (int grp_e = 0; grp_e < ngrp; ++grp_e) {
                    double* gtab = tab + (size_t)grp_e * nrow * RS;
                    const double v = gtab[ra] * gtab[rb];
                    gtab[rd] = v;
                    if constexpr (NP <= 4 && STREAM) gtab[rd + mir] = v;
                }
            }
        }
    }
    prologue_sync();
    if (stamps && (soft ? ptid : tid) == 0) stamps[2] = wall_clock64();

    // Work distribution.  Workgroup b owns micro-tiles b, b+grid, b+2*grid, ... (the tiles are
    // depth-sorted, so every workgroup -- hence every CU, and every XCD's L2 at every launch --
    // gets the same depth mix of the same data).  The (tile, group) work items of the workgroup
    // are dealt to its waves in snake order (static: a lane then keeps ONE running product per
    // group in registers and a work item costs no cross-lane traffic at all), or -- L.dyn_limit,
    // an A/B knob -- pulled longest-first through an LDS counter, each item's product going to its
    // own LDS slot.  Either way the multiplication order is fixed, so the schedule does not
    // change a single bit of the result.
    const uint32_t nt_v0 = owned_count(OSH, (uint32_t)l_num_mt(), vb0, nblk);
    const uint32_t nt_v1 = SPLIT ? owned_count(OSH, (uint32_t)l_num_mt(), vb0 + vstep, nblk) : 0u;
    const uint32_t nt_v2 = SPLIT > 2 ? owned_count(OSH, (uint32_t)l_num_mt(), vb0 + 2u * vstep, nblk) : 0u;
    // (more than three virtual blocks: owned_count does not grow with the block index and takes two neighbouring values over a
    // grid, so the counts are nt_v0 for the first nv_full virtual blocks and the last one's for the rest -- two scalars and a
    // compare, where an array of NVS counts indexed by the item's virtual block went to scratch memory)
    uint32_t nv_full = 0u, nt_last = nt_v0;
    if constexpr (NVS > 3) {
#pragma unroll
        for (int j = 0; j < NVS; ++j) {
            nt_last = owned_count(OSH, (uint32_t)l_num_mt(), vb0 + (uint32_t)j * vstep, nblk);
            nv_full += nt_last == nt_v0 ? 1u : 0u;
        }
    }
    auto nt_of = [&](uint32_t vs) {
        if constexpr (NVS > 3) return vs < nv_full ? nt_v0 : nt_last;
        else return vs == 0u ? nt_v0 : vs == 1u ? nt_v1 : nt_v2;
    };
    // (SPLIT: per virtual block, the largest -- virtual block vb0 has it: owned_count does not grow with the block index)
    const uint32_t ntile_blk = nt_v0;
    const size_t mp = L.m_pad;
    // work items: (tile, group), or (TPW consecutive owned tiles, group)
    const uint32_t nunit = SPLIT ? (uint32_t)NVS * ntile_blk : (ntile_blk + TPW - 1) / TPW;
    const uint32_t nitem = (kAblate & kAblNoItems) ? 0u : nunit * (uint32_t)ngrp;
    const float inv_nunit = 1.0f / (float)(nunit ? nunit : 1u);
    const uint32_t ngrp_magic = ngrp > 1 ? 0xFFFFFFFFu / (uint32_t)ngrp + 1u : 0u;      // ceil(2^32 / ngrp) for ngrp >= 2
    // Decided on ceil(tiles / workgroups), the same for every workgroup and exactly what
    // eval_shmem_np sized the result slots for (a workgroup with one tile fewer must not choose
    // differently: the queue needs a slot per item, the static deal only one per wave).
    const bool dyn = QUEUE < 0 ? eval_is_dynamic(L, nblk, nwave, ngrp) : QUEUE != 0;
    // The pileup arrays through GLOBAL-address-space pointers: the resident kernel passes its layout through
    // opaque registers every round, after which the compiler no longer knows where the pointers came from
    // and would use flat loads -- whose waits also cover the LDS counter, i.e. every per-marker load would
    // be waited for together with the table reads.
    typedef unsigned int __attribute__((ext_vector_type(2))) vuint2;          // (a plain vector: loadable through address_space(1))
    typedef __attribute__((address_space(1))) const vuint2 g_cuint2;
    typedef __attribute__((address_space(1))) const double g_cdouble;
    typedef __attribute__((address_space(1))) const char g_cchar;
    g_cuint2* const g_rec = (g_cuint2*)(W16 ? L.mt_rec16 : L.mt_rec);
    g_cuint2* const g_codes = (g_cuint2*)(W16 ? L.codes16 : L.codes);
    // (PD: a row of the list is 16 x 4 bytes -- two 16-bit steps per marker -- where the run words' rows are 16 x 8)
    typedef __attribute__((address_space(1))) const uint32_t g_cuint;
    typedef __attribute__((address_space(3))) const uint32_t lds_cuint;
    typedef typename std::conditional<PD, uint32_t, vuint2>::type RowWord;
    constexpr uint32_t kRowBytes = PD ? kMtMarkers * 4u : kMtMarkers * 8u, kLaneBytes = PD ? 4u : 8u;
    g_cdouble* const g_ediag = (g_cdouble*)L.ediag;
    g_cdouble* const g_ud = (g_cdouble*)L.ud;
    g_cdouble* const g_mu = (g_cdouble*)L.mu;
    g_cdouble* const g_kaf = (g_cdouble*)known_af_p;
    // ADDR_SCALAR: the same arrays through buffer descriptors -- kernel arguments, so wave-uniform and built by the scalar unit.
    // A column of the per-marker constants has a descriptor of its OWN: base + column x m_pad x 8 in 64-bit scalar arithmetic
    // (m_pad < 2^29: a 32-bit scalar offset would wrap at the third column of the largest contexts), m_pad x 8 bytes long, the lane's
    // part -- its marker's byte offset -- in the 32-bit vector offset.  The run lists: one descriptor without a length of its own
    // (the layout does not carry the list's; the array's padding rows bound the reads past a tile as before), the lane's word of a
    // row in the vector offset, the row in the scalar one (a sample's list stays below 4 GiB: Context::create).
    constexpr int kRsrcFlags = 0x00020000;                // (raw buffer, 32-bit data format: untyped loads)
    const uint32_t col_bytes = (uint32_t)(mp * 8);
    auto col_rsrc = [&](const double* base_) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base_), 0, (int)col_bytes, kRsrcFlags);
    };
    const uint32_t lane_word = (uint32_t)m * kLaneBytes;  // this lane's word of a row of the list
    auto codes_rsrc = [&] {
        if constexpr (Config::ADDR_SCALAR && KSEL == 0) {       // (kItemScalars, below: the quad's registers free between the loads)
            unsigned long long b_ = (unsigned long long)(W16 ? L.codes16 : L.codes);
            asm volatile("" : "+s"(b_));
            return __builtin_amdgcn_make_buffer_rsrc((void*)b_, 0, -1, kRsrcFlags);
        }
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint2*>(W16 ? L.codes16 : L.codes), 0, -1, kRsrcFlags);
    };
    auto list_word = [&](const uint32_t row_, const uint32_t ahead_) -> uint32_t {      // row row_ + ahead_ (a constant: the instruction's offset)
        return __builtin_amdgcn_raw_buffer_load_b32(codes_rsrc(), lane_word + ahead_ * kRowBytes, row_ * kRowBytes, 0);
    };
    // The per-marker likelihoods of a work item are MULTIPLIED (mantissa x 2^exponent): over
    // the 16 markers of the tile by a butterfly, then slot by slot in the block reduction.
    auto tile_product = [&](ScaledProd* p, bool cross) {  // over the 16 lanes sharing slot g (+ the item's other tiles)
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const int partner = lane_of(m ^ off, g4);
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                p[t].m *= lane_xchg_f64(p[t].m, off, partner);    // 16 factors in [0.5,1): no underflow
                p[t].e += lane_xchg_f64(p[t].e, off, partner);
            }
        }
        if (!cross) return;
#pragma unroll
        for (int off = SLOTS; off < 4; off <<= 1) {       // the item's other micro-tiles
            const int partner = lane_of(m, g4 ^ off);
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                p[t].m *= __shfl(p[t].m, partner, 64);    // factors >= 2^-16 each: no underflow
                p[t].e += __shfl(p[t].e, partner, 64);
            }
        }
    };
    LaneProd wave_prod[BTL];                              // static mode: this lane's running product
#pragma unroll
    for (int t = 0; t < BTL; ++t) wave_prod[t] = LaneProd{1.0, 0};
    int nfactor = 0;                                      // factors in wave_prod.m since its last renormalisation
    auto renorm_wave = [&]() {
#pragma unroll
        for (int t = 0; t < BTL; ++t) {
            wave_prod[t].e += __builtin_amdgcn_frexp_exp(wave_prod[t].m);
            wave_prod[t].m = __builtin_amdgcn_frexp_mant(wave_prod[t].m);
        }
        nfactor = 0;
    };
    uint32_t grp_wave = 0;                                // static mode: group wave_prod belongs to
    auto flush_wave = [&](uint32_t grp) {                 // static mode: one slot per (wave, group)
        renorm_wave();
        ScaledProd sp[BTL];
#pragma unroll
        for (int t = 0; t < BTL; ++t) sp[t] = ScaledProd{wave_prod[t].m, (double)wave_prod[t].e};
        tile_product(sp, true);
        if (m == 0 && half == 0) {
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                const size_t o = (((size_t)grp * nwave + wave) * NP + g * BTL + t) * 2;
                tile_llk[o] = sp[t].m;
                tile_llk[o + 1] = sp[t].e;
            }
        }
#pragma unroll
        for (int t = 0; t < BTL; ++t) wave_prod[t] = LaneProd{1.0, 0};
    };
    uint32_t etab_lane = (uint32_t)(lane & (kEtabCopies - 1)) * 8u;     // etab is at LDS address 0 (no static LDS in this file)
    const uint32_t tab_addr = lds_byte_addr(tab);
    const uint32_t ptq_addr = lds_byte_addr(ptq);
    // COEF_DPP: the projection's coefficients, resident in the lanes of the DPP rows for the whole launch -- loaded here, behind the
    // barrier after which ptq is complete, and never written again (no vector write of them anywhere near a DPP read: there is none
    // in the item loop).  Which slots a 16-lane row r = lane >> 4 holds, from lane_map: the quads of the rows 0 and 2 have slot
    // parity 0, 1, 1, 0, those of the rows 1 and 3 parity 1, 0, 0, 1 (nib & 1 of the quads 0..3 and 4..7), and the slot is the
    // parity + 2 * (lane >> 5) -- the row's quads {0, 3} belong to slot r, its quads {1, 2} to slot r ^ 1: the LDS pass groups
    // straddle the rows.  --NumPC 4 (sixteen coefficients a slot, ptq's order [2 k][2 points]): lane i of the row holds ptq[slot r][i]
    // in coef_a and ptq[slot r ^ 1][i] in coef_b.  --NumPC 2 (eight a slot): one pair is enough -- the lanes 0..7 hold slot r's,
    // the lanes 8..15 slot r ^ 1's, in coef_a.  The values the epilogue's reads brought, the copies of a padded group's last
    // valid point among them: they come from the same ptq.
    double coef_a = 0.0, coef_b = 0.0;
    if constexpr (kCoefDpp) {
        static_assert(SLOTS == 4 && 2 * KSEL * BTL <= 16, "a row's sixteen lanes hold a slot's coefficients, or two slots'");
        const uint32_t row_ = (uint32_t)lane >> 4, i_ = (uint32_t)lane & 15u;
        // (kept as they are loaded: opaque, so that nothing reads them again from LDS inside the loop)
        if constexpr (KSEL == 4) {
            coef_a = *reinterpret_cast<lds_cdouble*>(ptq_addr + (row_ * 16u + i_) * 8u);
            coef_b = *reinterpret_cast<lds_cdouble*>(ptq_addr + ((row_ ^ 1u) * 16u + i_) * 8u);
            asm volatile("" : "+v"(coef_a), "+v"(coef_b));
        } else {
            coef_a = *reinterpret_cast<lds_cdouble*>(ptq_addr + ((i_ < 8u ? row_ : row_ ^ 1u) * 8u + (i_ & 7u)) * 8u);
            asm volatile("" : "+v"(coef_a));
        }
    }
    if (L.stagger > 0 && wave >= (nwave >> 1))
        for (int i = 0; i < L.stagger; ++i) __builtin_amdgcn_s_sleep(1);
    // static mode: the host-built schedule (LPT over the waves), or items dealt in snake order
    const bool have_sched = !dyn && sch.off != nullptr;
    uint32_t s_i = 0, s_end = 0;
    if (have_sched) {
        s_i = sch.off[blk * (uint32_t)nwave + (uint32_t)wave];
        s_end = sch.off[blk * (uint32_t)nwave + (uint32_t)wave + 1];
    }
    uint32_t round = 0;
    if (hook_mine && !soft) hook.run();                   // (this wave takes no work items; the others cover for it)
#ifdef VB2_STAMP_CTRL     // (profiling build: workgroup 0's slot 3 = the control wave is back from its tile-phase work)
    if (stamps && hook_mine && lane == 0) stamps[3] = wall_clock64();
#endif
    typedef __attribute__((address_space(3))) const vuint2 lds_cuint2v;
    // (PD, the 8-point shape: its window of rows moves up a row at a time -- kept short)
    constexpr int kPf = (STREAM && !(PD && MODE == 2)) ? kPrefetch : kPrefetchL2;
    RowWord w[kPf];                                       // this lane's run words, kPf rows in flight
    // PIPE (a cohort step under the static deal: every sample's lists come from HBM, one item = ~8 KB per wave, and a
    // wave that requests an item's bytes, waits ~2 us for ALL of them -- the compiler's vmcnt(0) at the head of the row
    // loop --, computes for ~2 us and only then requests the next item's spends half its time waiting, and four waves
    // per SIMD do not cover that).  So the next item's run words are requested BEFORE this item's epilogue and its tile
    // record an item earlier still; this item's per-marker constants are requested at its top and awaited at its epilogue;
    // the first kPf rows of an item are walked in straight-line code, where the compiler counts the loads in flight
    // instead of draining them.
    // (compiled for the static deal only -- QUEUE == 0 --: with the way of dealing decided at run time the carried
    // registers of the two ways meet in copies after every item, and a copy of a register that is being loaded drains the
    // loads: the 4-point cohort step, whose kernel decides at run time, went 199 -> 228 us that way.  The same for the
    // 8-point shape on the work queue was measured and dropped twice: HISTORY.md.)
    constexpr bool PIPE = STREAM && ONEGRP && !LCACHE && QUEUE == 0;
    // the item after position (s_pos, rnd) of this wave's static deal
    auto static_item = [&](uint32_t s_pos, uint32_t rnd) -> uint32_t {
        if (have_sched) return s_pos < s_end ? (uint32_t)sch.item[s_pos] : nitem;
        return rnd * (uint32_t)nwave + ((rnd & 1u) ? (uint32_t)(nwave - 1 - wave) : (uint32_t)wave);
    };
    // (one group) item -> this lane's micro-tile
    auto tile_of = [&](uint32_t idx_, bool& have_) -> uint32_t {
        const uint32_t it_ = TPW * idx_ + (uint32_t)half;
        have_ = idx_ < nitem && (TPW == 1 || it_ < ntile_blk);
        return have_ ? owned_tile(OSH, blk, nblk, it_) : owned_tile(OSH, blk, nblk, 0u);
    };
    auto draw_item = [&]() -> uint32_t {                             // the workgroup's next item, whichever wave asks first
        if constexpr (kAddrScalar) {
            // (every wave draws one item, and all its lanes are here: lane 0 alone, under an exec mask of one bit, adds 1 -- the
            // compiler's wave-aggregated form counts the lanes and finds the first for an atomic that only ever has one.  The
            // wait is the one the compiler placed: the record's request below needs the item.  Written out because the counter
            // of LDS returns is not the compiler's to track inside a statement; exec is put back before the statement ends.)
            uint32_t nxt_, one_;
            unsigned long long exec_;
            asm volatile("s_mov_b64 %2, exec\n\t"
                         "s_mov_b64 exec, 1\n\t"
                         "v_mov_b32 %1, 1\n\t"
                         "ds_add_rtn_u32 %1, %3, %1\n\t"
                         "s_waitcnt lgkmcnt(0)\n\t"
                         "v_readfirstlane_b32 %0, %1\n\t"
                         "s_mov_b64 exec, %2"
                         : "=&s"(nxt_), "=&v"(one_), "=&s"(exec_)
                         : "v"(lds_byte_addr(queue))
                         : "memory");
            return nxt_;
        }
        uint32_t nxt = 0;
        if (lane == 0) nxt = atomicAdd(queue, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane(nxt);
    };
    auto issue_rows = [&](const vuint2 rec_, bool have_) {           // the first kPf rows of a tile (clamped to its own)
        const uint32_t cb_ = rec_.x * kRowBytes + (uint32_t)m * kLaneBytes;       // (32-bit byte offsets: see load_row)
        const int rows_ = have_ ? (PD ? (int)(((rec_.y >> 16) + (W16 ? 3u : 1u)) >> (W16 ? 2 : 1)) : (int)rec_.y) : 0;
        const int last_ = rows_ > 0 ? rows_ - 1 : 0;
#pragma unroll
        for (int j = 0; j < kPf; ++j) {
            g_cchar* a_ = reinterpret_cast<g_cchar*>(g_codes) + (cb_ + (uint32_t)(j < last_ ? j : last_) * kRowBytes);
            if constexpr (PD) w[j] = *reinterpret_cast<g_cuint*>(a_);
            else w[j] = *reinterpret_cast<g_cuint2*>(a_);
        }
    };
    // ---- one uint2 of run words (2 runs, or 4 of the 16-bit lists) into the accumulators ----
    // (first_tag: the tile's first row under PEEL -- its first run starts the sums from `init`, the marker's "other base"
    // constant, instead of adding to accumulators that were set to it: the same FMAs, twelve register moves fewer per item)
    auto walk_word = [&](const vuint2 w_cur, double* acc, const uint32_t my_tab, const uint32_t my_tab_w16, auto first_tag,
                         const double init) {
        constexpr bool kFirst = decltype(first_tag)::value;
        if constexpr ((kAblate & kAblNoReads) != 0) {        // (ablation build: the run words are consumed, the table is not read)
            acc[0] += __hiloint2double((int)((w_cur.x ^ w_cur.y) & 0x000f0000u) | 0x3ff00000, 0);
            return;
        }
#pragma unroll
        for (int j = 0; j < (W16 ? 4 : 2); ++j) {
            // one run: `n` reads of the same (class, quality) -> n * table row.  The run
            // word is {low half: byte offset of the row, high half: the top 16 bits of the
            // double n} -- one add and one and, no multiply, no int -> double conversion.
            // W16 (cohort steps): {low byte: dictionary index, next byte: n} -- two field
            // extractions, a multiply-add and a conversion, for half the bytes from HBM
            double n;
            uint32_t row_addr;
            if constexpr (W16) {
                // 16-bit run word = dictionary index | count code << 8, count code = (top 16 bits of double(n)) -
                // 0x3ff0 = exponent offset << 4 | top four mantissa bits (n <= 31: that IS the double).  The
                // high dword of 2 * n is 0x40 | code | 00 | 00: ONE byte permute (every VALU instruction costs
                // the same issue slot on gfx950 -- tools/ubench/int_rates.hip -- so what counts is their number:
                // round 3 spent five per run on the decode, and - 1 point per lane - six on the arithmetic);
                // the row address is one 24-bit multiply of the index byte, the table's base rides in the
                // ds_read's immediate offset.
                const uint32_t w2 = (j & 2) ? w_cur.y : w_cur.x;
                const uint32_t idx = (j & 1) ? ((w2 >> 16) & 0xffu) : (w2 & 0xffu);
                const uint32_t hi = __builtin_amdgcn_perm(0x40000000u, w2, (j & 1) ? 0x07030c0cu : 0x07010c0cu);
                n = __hiloint2double((int)hi, 0);
                row_addr = my_tab_w16 + __umul24(idx, (uint32_t)row_bytes);
            } else {
                const uint32_t rw = j ? w_cur.y : w_cur.x;
                n = __hiloint2double((int)(rw & 0xffff0000u), 0);
                row_addr = my_tab + (rw & 0xffffu);
            }
            lds_cdouble2* row = reinterpret_cast<lds_cdouble2*>(row_addr);
#pragma unroll
            for (int i = 0; i < 3 * BTL; ++i) {
                const vdouble2 t = row[i];
                acc[2 * i] = fma(n, t.x, (kFirst && j == 0) ? init : acc[2 * i]);
                acc[2 * i + 1] = fma(n, t.y, (kFirst && j == 0) ? init : acc[2 * i + 1]);
            }
        }
    };
    // ---- PD: one word of the list = two steps.  A step multiplies the six products of every point by ONE table row; class alt
    // (the rows behind the tile's ref rows: alt_tag) by the same row read the other way round, pair p <-> 5 - p.  No count, no
    // conversion: one SDWA add per step and the multiplies ----
    // (kFixedRing, every row but the first: the caller has taken the word's two row addresses from it and passes THEM as w_cur and my_tab)
    auto walk_pd = [&](const uint32_t w_cur, double* acc, const uint32_t my_tab, auto alt0_tag, auto alt1_tag, auto first_tag) {
        constexpr bool kAlt0 = decltype(alt0_tag)::value, kAlt1 = decltype(alt1_tag)::value, kFirst = decltype(first_tag)::value;
        constexpr bool kAt = kFixedRing && !kFirst;
        if constexpr ((kAblate & kAblNoReads) != 0) {        // (ablation build: the steps are consumed, the table is not read)
            acc[0] = (kFirst ? 1.0 : acc[0]) * __hiloint2double((int)((w_cur ^ (w_cur >> 16)) & 0x000fu) | 0x3ff00000, 0);
            return;
        }
        // (kReadsAhead: the word's rows are REQUESTED before they are multiplied -- both steps' 6 * BTL reads, then the
        // 12 * BTL multiplies -- and the order is pinned behind them.  Left to itself the scheduler takes the low-pressure
        // order: four landing quads, three dependent LDS round trips per step, every step drained.  The same multiplies in the
        // same order on the same products: no bit moves.  The first row already has all its reads in flight -- its first step
        // has nothing to multiply.)
        if constexpr (kReadsAhead && !kFirst && (kAblate & kAblNoMul) == 0) {
            vdouble2 t[6 * BTL];
            auto request = [&](const int j) {
                const bool kAlt = j ? kAlt1 : kAlt0;
                uint32_t row_addr;
                if constexpr (kAt) row_addr = j ? my_tab : w_cur;
                else row_addr = (kAlt ? my_tab - (uint32_t)kPdAltOffset : my_tab) + (j ? (w_cur >> 16) : (w_cur & 0xffffu));
                lds_cdouble2* row = reinterpret_cast<lds_cdouble2*>(row_addr);
#pragma unroll
                for (int i = 0; i < 3 * BTL; ++i) t[j * 3 * BTL + i] = row[i];
            };
            auto multiply = [&](const int j) {
                const bool kAlt = j ? kAlt1 : kAlt0;
#pragma unroll
                for (int i = 0; i < 3 * BTL; ++i) {
                    const int pt = i / 3, q2 = 2 * (i - 3 * pt);
                    const int a0 = pt * 6 + (kAlt ? 5 - q2 : q2), a1 = pt * 6 + (kAlt ? 4 - q2 : q2 + 1);
                    acc[a0] = acc[a0] * t[j * 3 * BTL + i].x;
                    acc[a1] = acc[a1] * t[j * 3 * BTL + i].y;
                }
            };
            // (0x100: LDS reads, 0x002: vector ALU; the groups of one id follow each other in this order)
            request(0); request(1);
            multiply(0); multiply(1);
            __builtin_amdgcn_sched_group_barrier(0x100, 6 * BTL, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 12 * BTL, 0);
            return;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool kAlt = j ? kAlt1 : kAlt0;        // (a compile-time value after unrolling)
            // (an alt step's offset points at the mirror image the narrow shapes keep in the row's second half: this shape
            // has eight points there -- it takes the offset off and names its products the other way round)
            const uint32_t row_addr = (kAlt ? my_tab - (uint32_t)kPdAltOffset : my_tab) + (j ? (w_cur >> 16) : (w_cur & 0xffffu));
            lds_cdouble2* row = reinterpret_cast<lds_cdouble2*>(row_addr);
#pragma unroll
            for (int i = 0; i < 3 * BTL; ++i) {
                const vdouble2 t = row[i];
                const int pt = i / 3, q2 = 2 * (i - 3 * pt);
                const int a0 = pt * 6 + (kAlt ? 5 - q2 : q2), a1 = pt * 6 + (kAlt ? 4 - q2 : q2 + 1);
                // (a tile's first step: the products START as the row -- the marker's constant is multiplied in once, at the end)
                if constexpr ((kAblate & kAblNoMul) != 0) {      // (ablation build: the rows are read and consumed, not multiplied)
                    asm volatile("" ::"v"(t.x), "v"(t.y));
                    if (kFirst && j == 0) { acc[a0] = t.x; acc[a1] = t.y; }
                    continue;
                }
                acc[a0] = (kFirst && j == 0) ? t.x : acc[a0] * t.x;
                acc[a1] = (kFirst && j == 0) ? t.y : acc[a1] * t.y;
            }
        }
    };
    // ---- PD, shapes of at most four points per row: ONE kind of step -- an alt step's offset points at the row's mirror image ----
    auto walk_pd1 = [&](const uint32_t w_cur, double* acc, const uint32_t my_tab, auto first_tag) {
        constexpr bool kFirst = decltype(first_tag)::value;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t row_addr = my_tab + (j ? (w_cur >> 16) : (w_cur & 0xffffu));
            lds_cdouble2* row = reinterpret_cast<lds_cdouble2*>(row_addr);
#pragma unroll
            for (int i = 0; i < 3 * BTL; ++i) {
                const vdouble2 t = row[i];
                acc[2 * i] = (kFirst && j == 0) ? t.x : acc[2 * i] * t.x;
                acc[2 * i + 1] = (kFirst && j == 0) ? t.y : acc[2 * i + 1] * t.y;
            }
        }
    };
    // ---- PD, the cohort steps' 8-BIT lists (W16; DeviceLayout::codes16 of a probability-domain context): a word = FOUR steps, a
    // byte = the row's index; whether a step is an alt step -- its row's mirror image, kPdAltOffset into the row -- follows from
    // its position in the tile (the ref steps come first: step >= s1).  Half the list bytes of a step that is bound by what it
    // streams; three vector instructions more per step (index x row stride, the comparison, the choice of the base) ----
    auto walk_pd8 = [&](const uint32_t w_cur, double* acc, const uint32_t my_tab, auto first_tag, const int step0, const int s1) {
        constexpr bool kFirst = decltype(first_tag)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t idx = (w_cur >> (8 * j)) & 0xffu;
            const uint32_t base = (step0 + j >= s1) ? my_tab + (uint32_t)kPdAltOffset : my_tab;
            const uint32_t row_addr = base + __umul24(idx, (uint32_t)row_bytes);
            lds_cdouble2* row = reinterpret_cast<lds_cdouble2*>(row_addr);
#pragma unroll
            for (int i = 0; i < 3 * BTL; ++i) {
                const vdouble2 t = row[i];
                acc[2 * i] = (kFirst && j == 0) ? t.x : acc[2 * i] * t.x;
                acc[2 * i + 1] = (kFirst && j == 0) ? t.y : acc[2 * i + 1] * t.y;
            }
        }
    };
    // (the number of components, the columns' length and the known-AF pointer AS AN ITEM SEES THEM.  The same values in every
    // kernel; the ADDR_SCALAR kernels of KSEL 0, where they are run-time values, pass them through opaque scalar registers once per
    // item -- kItemScalars, in the item loop --, so that what is derived from them is computed by a scalar instruction or two where
    // it is used.  Hoisted out of the item loop, the tests `kk < k` and `known_af == nullptr` were six 64-bit masks, the columns'
    // bases eighteen registers and the tail of the projection's loop four more, kept across the whole loop: 28 to 30 scalar
    // registers of those three kernels went to vector lanes, 14 to 31 before ADDR_SCALAR.  With the hand-off's arguments read again
    // behind the item loop -- see there -- none does.)
    constexpr bool kItemScalars = kAddrScalar && KSEL == 0;
    int k_item = k;
    size_t mp_item = mp;
    unsigned long long kaf_item = (unsigned long long)known_af_p;
    // ---- per-marker epilogue: a marker's likelihood as (mantissa, exponent) per point, from its six sums per point ----
    auto marker_lk = [&](const bool live, const uint32_t pos, const double* acc, const double e0, const double e1, const double e2,
                         const double* udr, const double mur, const uint32_t my_ptq, double* lk_m, int* lk_e, const double cst_pd) {
#pragma unroll
        for (int t = 0; t < BTL; ++t) { lk_m[t] = 1.0; lk_e[t] = 0; }
        if constexpr ((kAblate & kAblNoEpi) != 0) {          // (ablation build: the sums and the constants are consumed, nothing is computed from them)
            double z = e0 + e1 + e2 + mur + udr[0] + udr[1] + udr[2] + udr[3];
            for (int i = 0; i < BTL * 6; ++i) z += acc[i];
            if (z == 12345.678) lk_m[0] = 0.75;
            return;
        }
        // COEF_DPP: the projection with its coefficients from the resident registers coef_a / coef_b, lane j of the reader's own
        // 16-lane row -- v_fmac_f64_dpp under row_newbcast:j, written as assembly: the compiler does not fold a 64-bit DPP move into
        // the FMA.  Per FMA of the old projection TWO: from coef_a under bank mask 0x9 (the row's quads 0 and 3: slot r) and from coef_b
        // -- --NumPC 2: the same pair's upper eight lanes -- under 0x6 (quads 1 and 2: slot r ^ 1); under a bank mask the other quads
        // keep their accumulator, so every lane ends with its own slot's sum.  Per accumulator the components come in the old order
        // kk = 0, 1, ..., each a fused multiply-add of the same two factors into the same addend: the same bits.  One statement per
        // component, the four accumulators interleaved: a chain's dependent FMAs are four instructions apart.
        // What the compiler does not check for inline assembly:
        //   * EXEC must be all ones here -- a source lane that is switched off leaves its readers with their old value (bound_ctrl
        //     is 0), silently.  So the projection stands IN FRONT of the branch on `live`, which diverges in a partly filled last
        //     tile, and runs for all 64 lanes: the branches around the epilogue are wave-uniform, every workgroup is whole waves.
        //     A dead lane's udr was loaded from position 0 and is finite; its sums are not used.
        //   * no vector instruction writes coef_a / coef_b in the item loop (a VALU write of a DPP source needs two wait states);
        //   * a vector instruction that writes EXEC needs five wait states before a DPP instruction: the s_nop 4 at the head of the
        //     first statement covers them (the statements are volatile and keep their order).
        double afd1[2] = {0., 0.}, afd2[2] = {0., 0.};
        if constexpr (kCoefDpp) {
            const double cb_ = KSEL == 2 ? coef_a : coef_b;
            project_dpp<KSEL, 0>(afd1[0], afd1[1], afd2[0], afd2[1], coef_a, cb_, udr[0]);
            project_dpp<KSEL, 1>(afd1[0], afd1[1], afd2[0], afd2[1], coef_a, cb_, udr[1]);
            if constexpr (KSEL == 4) {
                project_dpp<KSEL, 2>(afd1[0], afd1[1], afd2[0], afd2[1], coef_a, cb_, udr[2]);
                project_dpp<KSEL, 3>(afd1[0], afd1[1], afd2[0], afd2[1], coef_a, cb_, udr[3]);
            }
        }
        if (live) {
            double af1[BTL], af2[BTL];
            if constexpr (kCoefDpp) {
#pragma unroll
                for (int t = 0; t < BTL; ++t) {
                    af1[t] = afd1[t] + mur; af1[t] /= 2.0;
                    af2[t] = afd2[t] + mur; af2[t] /= 2.0;
                }
            } else
            if (kaf_item) {
                const double a = g_kaf[pos];
#pragma unroll
                for (int t = 0; t < BTL; ++t) af1[t] = af2[t] = a;
            } else {
                // h:251-267: AF = (sum_k UD[i][k]*pc[k] + mean) / 2, same order of the k terms; each
                // term enters with one rounding (FMA) where the reference's x86-64 build rounds the
                // product first: AF differs by <= k/2 ulp, far inside the 1e-12 the tests hold the LLK to
#pragma unroll
                for (int t = 0; t < BTL; ++t) af1[t] = af2[t] = 0.;
                auto project = [&](int kk, double uu) {
                    if constexpr (BTL == 2) {              // both points' coefficient in one ds_read_b128
                        const vdouble2 c1 = *reinterpret_cast<lds_cdouble2*>(my_ptq + (uint32_t)kk * 16u);
                        const vdouble2 c2 = *reinterpret_cast<lds_cdouble2*>(my_ptq + (uint32_t)(k_item + kk) * 16u);
                        af1[0] = fma(uu, c1.x, af1[0]); af1[1] = fma(uu, c1.y, af1[1]);
                        af2[0] = fma(uu, c2.x, af2[0]); af2[1] = fma(uu, c2.y, af2[1]);
                    } else {
                        af1[0] = fma(uu, *reinterpret_cast<lds_cdouble*>(my_ptq + (uint32_t)kk * 8u), af1[0]);
                        af2[0] = fma(uu, *reinterpret_cast<lds_cdouble*>(my_ptq + (uint32_t)(k_item + kk) * 8u), af2[0]);
                    }
                };
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    if (kk < k_item) project(kk, udr[kk]);                       // rows loaded before the read loop
                for (int kk = 4; kk < k_item; ++kk) project(kk, g_ud[(size_t)kk * mp_item + pos]);
                const double mu = mur;
#pragma unroll
                for (int t = 0; t < BTL; ++t) {
                    af1[t] += mu; af1[t] /= 2.0;
                    af2[t] += mu; af2[t] /= 2.0;
                }
            }
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                double gf[3], gf2[3];
                initial_gf(af1[t], gf);
                initial_gf(af2[t], gf2);
                const double* a = acc + t * 6;
                // h:307-311: lk = sum_{g1,g2} exp(A[g1][g2]) GF[g1] GF2[g2], factored as
                // sum_g1 GF[g1] * (sum_g2 exp(A[g1][g2]) GF2[g2]) with FMAs (12 operations instead
                // of 27; the rounding differs from the reference's term-by-term sum at the 1e-16
                // level, like the marker summation order does).  The three g1==g2 exponentials do
                // not depend on (alpha, PC) and were taken at context creation.
                double x01, x02, x10, x12, x20, x21;
                const double a_min = PD ? 0.0 : vmin2_f64(vmin2_f64(vmin2_f64(a[0], a[1]), vmin2_f64(a[2], a[3])), vmin2_f64(a[4], a[5]));
                if constexpr (PD) {
                    // the products ARE the six likelihoods: no exponential (probability domain)
                    x01 = a[0]; x02 = a[1]; x10 = a[2]; x12 = a[3]; x20 = a[4]; x21 = a[5];
                } else
                if (__builtin_expect(a_min < -708.0, 0)) {      // (wave-divergent, and never taken on whole-genome depths: exp_nonpos)
                    x01 = exp_nonpos<ESH, true>(a[0], etab_lane); x02 = exp_nonpos<ESH, true>(a[1], etab_lane);
                    x10 = exp_nonpos<ESH, true>(a[2], etab_lane); x12 = exp_nonpos<ESH, true>(a[3], etab_lane);
                    x20 = exp_nonpos<ESH, true>(a[4], etab_lane); x21 = exp_nonpos<ESH, true>(a[5], etab_lane);
                } else {
                    x01 = exp_nonpos<ESH>(a[0], etab_lane); x02 = exp_nonpos<ESH>(a[1], etab_lane);
                    x10 = exp_nonpos<ESH>(a[2], etab_lane); x12 = exp_nonpos<ESH>(a[3], etab_lane);
                    x20 = exp_nonpos<ESH>(a[4], etab_lane); x21 = exp_nonpos<ESH>(a[5], etab_lane);
                }
                double lk;
                if constexpr (PD) {
                    // the six products lack the marker's constant exp(c_other) (`cst`): it multiplies their part of the sum
                    // once; the three g1 == g2 terms hold it since context creation
                    const double o0 = fma(x02, gf2[2], x01 * gf2[1]);
                    const double o1 = fma(x12, gf2[2], x10 * gf2[0]);
                    const double o2 = fma(x21, gf2[1], x20 * gf2[0]);
                    const double off = fma(o2, gf[2], fma(o1, gf[1], o0 * gf[0]));
                    const double dg = fma(e2 * gf2[2], gf[2], fma(e1 * gf2[1], gf[1], (e0 * gf2[0]) * gf[0]));
                    lk = fma(cst_pd, off, dg);
                    if constexpr (!kEpiScatter) {              // (EPI_SCATTER: in the one branch of the tiny values, below)
                    if (__builtin_expect(lk < 0x1p-960, 0)) {
                        x01 *= cst_pd; x02 *= cst_pd; x10 *= cst_pd; x12 *= cst_pd; x20 *= cst_pd; x21 *= cst_pd;
                    }
                    }
                } else {
                const double s0 = fma(x02, gf2[2], fma(x01, gf2[1], e0 * gf2[0]));
                const double s1 = fma(x12, gf2[2], fma(e1, gf2[1], x10 * gf2[0]));
                const double s2 = fma(e2, gf2[2], fma(x21, gf2[1], x20 * gf2[0]));
                lk = fma(s2, gf[2], fma(s1, gf[1], s0 * gf[0]));
                }
                // Near the bottom of the double range the factoring is no longer harmless: products with
                // the priors underflow at different places, and the reference's rule below (h:310-311,
                // "add log(lk) only if lk > 0") turns that into a marker counted or dropped, 745 units
                // of LLK apart (markers with ~1000 reads).  There the sum is redone term by term in the
                // reference's own order (g1 outer, g2 inner, h:307-309), as round 1 did everywhere;
                // wave-divergent, and never taken on whole-genome depths.
                // (EPI_SCATTER: the select of the reference's rule below sits in this branch -- a value of at least 2^-960 is
                // positive --, and the condition is written so that a NaN takes the branch, is not re-summed and becomes 1.0)
                if (__builtin_expect(kEpiScatter ? !(lk >= 0x1p-960) : lk < 0x1p-960, 0)) {
                    if (!kEpiScatter || lk < 0x1p-960) {
                    if constexpr (PD && kEpiScatter) {
                        x01 *= cst_pd; x02 *= cst_pd; x10 *= cst_pd; x12 *= cst_pd; x20 *= cst_pd; x21 *= cst_pd;
                    }
                    double r = 0;
                    r += e0 * gf[0] * gf2[0];
                    r += x01 * gf[0] * gf2[1];
                    r += x02 * gf[0] * gf2[2];
                    r += x10 * gf[1] * gf2[0];
                    r += e1 * gf[1] * gf2[1];
                    r += x12 * gf[1] * gf2[2];
                    r += x20 * gf[2] * gf2[0];
                    r += x21 * gf[2] * gf2[1];
                    r += e2 * gf[2] * gf2[2];
                    lk = r;
                    }
                    if constexpr (kEpiScatter) lk = lk > 0 ? lk : 1.0;
                }
                // the reference adds log(lk) only if lk > 0 (h:310-311): a dropped marker is
                // the factor 1
                if constexpr (!kEpiScatter) lk = lk > 0 ? lk : 1.0;
                lk_m[t] = __builtin_amdgcn_frexp_mant(lk);
                lk_e[t] = __builtin_amdgcn_frexp_exp(lk);
            }
        }
    };
    vuint2 rec_nx;                                        // PIPE: the record of the item about to be processed ...
    rec_nx.x = rec_nx.y = 0u;
    double cst_nx = 0.0;                                  // ... and its markers' "other base" constants (the accumulators start from them)
    auto other_const = [&](uint32_t mt_, bool have_) -> double {
        const uint32_t pos_ = mt_ * (uint32_t)kMtMarkers + (uint32_t)m;
        const uint32_t boff_ = ((have_ && pos_ < (uint32_t)L.num_active) ? pos_ : 0u) * 8u;
        return *reinterpret_cast<g_cdouble*>(reinterpret_cast<__attribute__((address_space(1))) const char*>(g_ediag) + boff_);
    };
    // The workgroup of the resident kernel's control wave (wave 0, busy with the simplex during the tile phase): the waves w, w + 4,
    // w + 8, ... of a workgroup run on one SIMD (tools/ubench/wave_simd.hip), so the waves 4, 8, 12 share the control wave's.
    // They come LAST in the order in which the waves take their first items: a search round has fewer items than waves (13 for
    // 15 at C3), and the idle waves are then the control wave's neighbours instead of the last two.  Same items, same slots: the
    // same bits.  OptimizeLLK 6.09 -> 6.04 ms on the same box.
    const int spare_rank = (wave & 3) ? (wave >> 2) * 3 + (wave & 3) - 1 : (nwave - (nwave >> 2)) + (wave >> 2) - 1;
    // FEWER ITEMS THAN WAVES (a search round, the launches of one to four points): which wave takes which item decides how
    // the rows are spread over the CU's four SIMDs (waves w, w + 4, w + 8, w + 12 share one).  The items are depth-sorted, so
    // "wave w takes item w" gives SIMD 0 the deepest item of every four -- and a fourth item when there are thirteen -- and the
    // round ends with that SIMD's last wave.  Instead: one SIMD takes the ceil(n / 4) SHALLOWEST items (in the control wave's
    // workgroup: its SIMD, and one item fewer), the others share the rest in snake order; up to eight items: a snake over all
    // four.  On the queue a tile's product has its own slot whichever wave computes it: the same bits.  OptimizeLLK at C3
    // 5.86 -> 5.60 ms on one box (three alternating rounds; either workgroup kind alone: no gain -- the round ends with the
    // other kind), the control wave's SIMD with ONE item as before: no gain; tables for 13 items built by hand: the same 5.59-5.61.
    int deal_rank = hook_blk ? spare_rank : wave;
    if (dyn && nwave == 16 && ONEGRP && SPLIT == 0 && nitem <= (uint32_t)(hook_blk ? 15 : 16)) {
        const int n = (int)nitem, sd = wave & 3, sj = wave >> 2;
        int r;
        if (!hook_blk && n <= 8) r = sj == 0 ? sd : sj == 1 ? 7 - sd : n;
        else {
            const int c0 = ((n + 3) >> 2) - (hook_blk ? 1 : 0), nrest = n - c0;
            if (sd == 0) {
                const int j0 = sj - (hook_blk ? 1 : 0);
                r = (j0 >= 0 && j0 < c0) ? nrest + j0 : n;
            } else {
                r = 3 * sj + ((sj & 1) ? 3 - sd : sd - 1);
                if (r >= nrest) r = n;
            }
        }
        deal_rank = r < n ? r : n;
    }
    const uint32_t idx_first = hook_mine ? nitem
                               : have_sched ? (s_i < s_end ? (uint32_t)sch.item[s_i] : nitem)
                                            : (uint32_t)deal_rank;
    if (PIPE && idx_first < nitem) {
        bool h0;
        const uint32_t mt0 = tile_of(idx_first, h0);
        rec_nx = g_rec[mt0];
        cst_nx = other_const(mt0, h0);
        issue_rows(rec_nx, h0);
    }
    // ITEM_AHEAD (the 8-point probability-domain shape on the queue: several items per wave, lists in L2): an item used
    // to begin with three DEPENDENT trips -- the draw from the queue, the tile's record from L2, the list's first rows from L2 --
    // during which the wave feeds neither the LDS nor the VALU, and the depth-sorted items keep a workgroup's waves so close to
    // lock-step that these holes coincide.  Now a wave draws its next item when its last row's multiplies are issued, requests that
    // item's record at once and -- behind marker_lk, when the record is there -- the rows 0, 1 and 2 of its list: they land under
    // the epilogue, the 16-lane exchange and the slot write, and the next iteration starts from these registers.  The item's nine
    // per-marker constants stay where they were: requested at its top, awaited behind its read loop.  Each word is consumed in the
    // register it was loaded into -- row 0 and row 1 ARE the ring's two slots, row 2 is the first row's refill, so the three kinds
    // of first row request nothing and meet without a copy of a register that is being loaded (such a copy drains every load).
    // A tile's product still goes to its own slot: the same bits whichever wave drew it, and when.
    vuint2 rec_ah;                                        // the record of the item about to be processed ...
    rec_ah.x = rec_ah.y = 0u;
    uint32_t w_ah[3] = {0u, 0u, 0u};                      // ... and this lane's words of its rows 0, 1, 2
    auto request_rec_ahead = [&](const uint32_t idx_) {
        // (item -> tile as the loop's head does it; an item past the queue's end: tile 0's record, never used)
        const uint32_t unit_ = ngrp > 1 ? __umulhi(idx_, ngrp_magic) : idx_;
        const uint32_t vs_ = SPLIT ? unit_ % (uint32_t)NVS : 0u;
        const uint32_t it_ = SPLIT ? unit_ / (uint32_t)NVS : unit_;
        const bool have_ = idx_ < nitem && (SPLIT ? it_ < nt_of(vs_) : true);
        const uint32_t mt_ = have_ ? owned_tile(OSH, vb0 + vs_ * vstep, nblk, it_) : 0u;
        rec_ah = g_rec[mt_];
    };
    uint32_t rec_ah_x = 0u, rec_ah_y = 0u;                // ADDR_SCALAR: the record's two words in scalar registers -- one v_readfirstlane each per item
    auto request_rows_ahead = [&]() {
        // (a tile shorter than three rows: the rows behind it, never consumed -- the array ends in padding rows)
        if constexpr (kAddrScalar) {
            rec_ah_x = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec_ah.x);
            rec_ah_y = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec_ah.y);
#pragma unroll
            for (int j = 0; j < 3; ++j) w_ah[j] = list_word(rec_ah_x, (uint32_t)j);
            return;
        }
        const uint32_t cb_ = rec_ah.x * kRowBytes + (uint32_t)m * kLaneBytes;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            w_ah[j] = *reinterpret_cast<g_cuint*>(reinterpret_cast<g_cchar*>(g_codes) + (cb_ + (uint32_t)j * kRowBytes));
    };
    if constexpr (kAhead) {
        if (idx_first < nitem) {
            request_rec_ahead(idx_first);
            request_rows_ahead();
        }
    }
    for (uint32_t idx = idx_first; idx < nitem;) {
        // grp = idx / nunit without the ~25-instruction integer division: float estimate (exact for
        // these magnitudes up to one) and a correction step
        uint32_t grp, unit;
        if (MODE == 2 && QUEUE == 1 && !ONEGRP) {
            // The queue walks the tiles deepest first and every tile's point groups side by side: the waves that hold a tile's items at
            // the same time read the same run words and per-marker constants (one trip to L2 instead of up to six), and the order is
            // still longest-first.  The slots and their order are those of a group-by-group walk: the same bits.
            // (idx is uniform and so is the reciprocal: a scalar multiply-high -- exact for idx < 2^32 / ngrp -- where the float
            // division of the uniform pair cost fifteen vector instructions per item)
            unit = ngrp > 1 ? __umulhi(idx, ngrp_magic) : idx;
            grp = idx - unit * (uint32_t)ngrp;
        } else {
            grp = ngrp == 1 ? 0u : (uint32_t)(((float)idx + 0.5f) * inv_nunit);
            if (ngrp != 1) {
                if (grp * nunit > idx) --grp;
                else if ((grp + 1) * nunit <= idx) ++grp;
            }
            unit = idx - grp * nunit;
        }
        // index in this workgroup's tile list (SPLIT: the units alternate between the two virtual blocks -- both lists are
        // in descending order of rows, so the queue still walks longest first)
        const uint32_t vs = SPLIT ? unit % (uint32_t)NVS : 0u;
        const uint32_t it = SPLIT ? unit / (uint32_t)NVS : TPW * unit + (uint32_t)half;
        const bool have_tile = SPLIT ? it < nt_of(vs) : (TPW == 1 || it < ntile_blk);   // TPW > 1: the list's end may leave lanes idle
        const uint32_t mt = owned_tile(OSH, vb0 + vs * vstep, nblk, have_tile ? it : 0u);
        const uint32_t my_tab = tab_addr + (grp * (uint32_t)nrow * (uint32_t)row_bytes + (uint32_t)g * (6 * BTL * 8));
        const uint32_t my_ptq = ptq_addr + (grp * SLOTS + (uint32_t)g) * (uint32_t)(2 * k * BTL * 8);
        // (one slot, one group: the table's address is the constant behind the exp table -- this file has no static LDS --
        // and the compiler folds it into the reads' immediate offsets)
        const uint32_t my_tab_w16 = (SLOTS == 1 && ONEGRP) ? (uint32_t)((kEtabDoubles + kLogTabDoubles) * sizeof(double)) : my_tab;
        while (!dyn && grp_wave < grp) {                     // wave-uniform
            flush_wave(grp_wave);
            ++grp_wave;
        }
        // {first row, rows}; one scalar load when TPW == 1.  LCACHE: {LDS byte address of the tile's first row, rows}
        vuint2 rec;
        if constexpr (LCACHE) rec = *reinterpret_cast<lds_cuint2v*>(hook.cache_rec() + (have_tile ? it : 0u) * 8u);
        else if (PIPE) rec = rec_nx;
        else if (kAhead) rec = rec_ah;
        else rec = g_rec[mt];
        // PIPE: the next item's record, requested now, needed when this item's rows have been walked
        uint32_t idx_next = nitem;
        bool have_next = false;
        uint32_t mt_next = blk;
        vuint2 rec_n2;
        rec_n2.x = rec_n2.y = 0u;
        if (PIPE) {
            idx_next = static_item(s_i + 1, round + 1);
            mt_next = tile_of(idx_next, have_next);
            rec_n2 = g_rec[mt_next];
        }
        // per-marker constants: issued now, consumed after the read loop
        const uint32_t pos = mt * (uint32_t)kMtMarkers + (uint32_t)m;      // position in sorted order
        const bool live = have_tile && pos < (uint32_t)L.num_active;
        // One 32-bit byte offset for all of a marker's constants, each array's base a scalar: the loads take the
        // base-plus-offset form and cost no 64-bit vector address arithmetic (nine add pairs per item before).
        const uint32_t boff = (live ? pos : 0u) * 8u;        // (m_pad < 2^29: vb2_ctx_create refuses more markers)
        auto at = [&](g_cdouble* base_) -> double {
            // (the base through an opaque scalar register: else the compiler re-associates base + offset + column stride
            // and adds the uniform stride in 64-bit vector arithmetic)
            // (ADDR_SCALAR: the column's descriptor, this offset in the vector offset -- no vector instruction but the load;
            // a dead lane reads position 0 as before, and the descriptor's length is the column's)
            if constexpr (kAddrScalar) {
                // (the base through an opaque scalar register here too: nine descriptors kept across the loop are 36 scalar
                // registers, and the kernels of three workgroups to a set then spill some; a descriptor is two scalar moves)
                unsigned long long b_ = (unsigned long long)base_;
                asm volatile("" : "+s"(b_));
                const auto v_ = __builtin_amdgcn_raw_buffer_load_b64(col_rsrc((const double*)b_), boff, 0, 0);
                return __hiloint2double((int)v_[1], (int)v_[0]);
            }
            unsigned long long b_ = (unsigned long long)base_;
            asm volatile("" : "+s"(b_));
            return *reinterpret_cast<g_cdouble*>(reinterpret_cast<__attribute__((address_space(1))) const char*>(b_) + boff);
        };
        // (column c_ of an array.  kItemScalars: its base from the item's own copy of the columns' length -- two scalar adds a load,
        // nothing kept across the loop but the arrays' pointers)
        if constexpr (kItemScalars) asm volatile("" : "+s"(mp_item));
        const unsigned long long cs_ = (unsigned long long)mp_item * 8ull;
        auto at_col = [&](g_cdouble* arr_, const int c_) -> double {
            if constexpr (kItemScalars) {
                unsigned long long b_ = (unsigned long long)arr_ + (unsigned long long)c_ * cs_;
                asm volatile("" : "+s"(b_));
                const auto v_ = __builtin_amdgcn_raw_buffer_load_b64(col_rsrc((const double*)b_), boff, 0, 0);
                return __hiloint2double((int)v_[1], (int)v_[0]);
            }
            return at(arr_ + (size_t)c_ * mp);
        };
        const double cst = PIPE ? cst_nx : at_col(g_ediag, 0);
        const double e0 = at_col(g_ediag, 1), e1 = at_col(g_ediag, 2), e2 = at_col(g_ediag, 3);

        // (the panel row of the marker too: up to four UD columns and the mean)
        double udr[4], mur = 0.0;
        if constexpr (kItemScalars) { asm volatile("" : "+s"(k_item)); asm volatile("" : "+s"(kaf_item)); }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) udr[kk] = (!kaf_item && kk < k_item) ? at_col(g_ud, kk) : 0.0;
        if (!kaf_item) mur = at_col(g_mu, 0);

        // the six off-diagonal sums start from the marker's "other base" constant (it is part of
        // every genotype pair's sum, h:299-303), so the epilogue needs no separate addition
        // PEEL (one tile per wave, lists from L2: the launches of many points): a tile's row count is uniform, and its
        // first row is walked outside the row loop
        constexpr bool PEEL = TPW == 1 && !W16 && !PIPE && !LCACHE && QUEUE == 1 && (kAblate & kAblNoReads) == 0;
        double acc[BTL * 6];
        if constexpr (!PEEL && !PD) {
#pragma unroll
            for (int i = 0; i < BTL * 6; ++i) acc[i] = cst;
        }

        // ---- per-read accumulate (h:288-303), one step per run ----
        // Rows are prefetched kPrefetch deep: with one sample its pileup sits in L2, but a cohort
        // launch streams every sample's rows from HBM once, and two rows ahead (~0.6 us of work)
        // does not cover that latency.  The loads are unconditional: a prefetch past the tile's
        // last row reads the next tile's rows (never consumed), and the array ends in
        // 2 * kPrefetch padding rows (context.cpp).
        // The read loop is bound by the LDS pipe, the epilogue by the FP64 VALU, and the waves of a CU
        // are spread over both phases at any time: waves in the read loop get issue priority, so that
        // their ds_reads go out as soon as they can and the LDS pipe stays busy, while the epilogue
        // waves fill the VALU slots in between (-0.8 % per launch measured; the other way round: +0.8 %)
        // A search round (the four-point shape on the work queue) has at most one item per wave, and the round ends with the
        // wave that holds the deepest tiles (17 rows at C3 against a median of 9: the first items of the low-numbered
        // workgroups): the deeper a wave's item -- the lower its index -- the higher its priority on its SIMD (the three
        // deepest items of a workgroup are on three different SIMDs: the first deal above).  OptimizeLLK 5.98 -> 5.90 ms on the same box.
        if (MODE == 3 && ONEGRP && dyn) {
            if (idx < 4u) __builtin_amdgcn_s_setprio(3);
            else if (idx < 8u) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(1);
        } else
            __builtin_amdgcn_s_setprio(1);
        // the run words by 32-bit byte offsets from the array's (scalar) base: the list of one sample stays below 4 GiB
        // (Context::create refuses more rows), and a row's address costs no 64-bit vector arithmetic
        const uint32_t cbase = LCACHE ? 0u : rec.x * kRowBytes + (uint32_t)m * kLaneBytes;
        const uint32_t crow = rec.x + (uint32_t)m * kLaneBytes;      // (LCACHE: this lane's word of the tile's first row, LDS)
        // a scalar when TPW == 1.  PD: {ref steps | all steps << 16}: the tile's markers have their ref steps at [0, s1) and
        // their alt steps at [s1, s2), two steps to a row (walk_pd)
        // (one tile per wave: both are the same in every lane, and the compiler is told so -- the branches on them are scalar)
        // (ADDR_SCALAR: from the record's words as request_rows_ahead left them in scalar registers -- shifts and selects of the
        // scalar unit; the tile's first row for load_row too)
        const uint32_t rec_sx = rec_ah_x, rec_sy = kAddrScalar ? rec_ah_y : rec.y;
        const int steps_ref_v = PD ? (have_tile ? (int)(rec_sy & 0xffffu) : 0) : 0;
        const int rows_v = have_tile ? (PD ? (int)(((rec_sy >> 16) + (W16 ? 3u : 1u)) >> (W16 ? 2 : 1)) : (int)rec_sy) : 0;
        const int steps_ref = (PD && TPW == 1 && !kAddrScalar) ? __builtin_amdgcn_readfirstlane(steps_ref_v) : steps_ref_v;
        const int rows = (PD && TPW == 1 && !kAddrScalar) ? __builtin_amdgcn_readfirstlane(rows_v) : rows_v;
        // (ONE sample's pileup sits in L2, and a deep prefetch costs more than it hides there: the loads run past the
        // tile's last row -- up to kPf useless row loads per item of 6..16 rows -- and every block of kPf rows begins
        // by waiting for all of them.  Measured on one box, depth 8 / 4 / 2: 48-point launch 74.9 / 74.4 / 76.6 us;
        // OptimizeLLK at C3 (one 4-point item per wave and round) 7.8 / 7.55 / 7.35 ms, at 10 000 markers 2.39 /
        // 2.31 / 2.43 ms.)
        // (STREAM: rows past the tile's last are the NEXT tiles' -- another workgroup's, at another time: fetched here
        // they came from HBM twice, 573 MB instead of 356 MB per one-point step of 32 C3 samples (FETCH_SIZE, round 3).
        // The row index is clamped to the tile's last row instead: the same cache line again, no new bytes.)
        const int last_row = rows > 0 ? rows - 1 : 0;
        auto load_row = [&](int j) -> RowWord {              // row j of this lane's run words
            if constexpr (PD && (kAblate & kAblNoRowLoads) != 0) {      // (ablation build: no trip to memory for the steps -- made-up rows)
                const uint32_t r0 = ((uint32_t)m * 7u + (uint32_t)j * 2u) % (uint32_t)nrow, r1 = ((uint32_t)m * 7u + (uint32_t)j * 2u + 1u) % (uint32_t)nrow;
                return (r0 * (uint32_t)row_bytes) | ((r1 * (uint32_t)row_bytes) << 16);
            }
            // (ADDR_SCALAR: every caller asks for row r + kPf of the ring -- the kPf rides in the instruction's offset)
            if constexpr (kAddrScalar) return list_word(rec_sx + (uint32_t)(j - kPf), (uint32_t)kPf);
            if constexpr (LCACHE && PD) return *reinterpret_cast<lds_cuint*>(crow + (uint32_t)j * kRowBytes);
            else if constexpr (LCACHE) return *reinterpret_cast<lds_cuint2v*>(crow + (uint32_t)j * kRowBytes);
            else {
                g_cchar* a_ = reinterpret_cast<g_cchar*>(g_codes) + (cbase + (uint32_t)(STREAM ? (j < last_row ? j : last_row) : j) * kRowBytes);
                if constexpr (PD) return *reinterpret_cast<g_cuint*>(a_);
                else return *reinterpret_cast<g_cuint2*>(a_);
            }
        };
        if constexpr (kAhead) {
            if constexpr (PD) { w[0] = w_ah[0]; w[1] = w_ah[1]; }
        } else if (!PIPE) {
#pragma unroll
            for (int j = 0; j < kPf; ++j) w[j] = load_row(j);
        }
        auto walk_block = [&](const int s0, const bool refill, auto first_tag) {     // rows s0 .. s0 + kPf - 1 of the tile
            constexpr bool kFirstBlock = decltype(first_tag)::value;
#pragma unroll
            for (int u = 0; u < kPf; ++u) {
                if (s0 + u >= rows) break;
                const RowWord w_cur = w[u];
                if (refill) w[u] = load_row(s0 + u + kPf);
                if constexpr (PD) {
                    if constexpr (W16) {
                        if (kFirstBlock && u == 0) walk_pd8(w_cur, acc, my_tab, std::true_type(), (s0 + u) * 4, steps_ref);
                        else walk_pd8(w_cur, acc, my_tab, std::false_type(), (s0 + u) * 4, steps_ref);
                    } else {
                        if (kFirstBlock && u == 0) walk_pd1(w_cur, acc, my_tab, std::true_type());
                        else walk_pd1(w_cur, acc, my_tab, std::false_type());
                    }
                } else {
                    if (kFirstBlock && u == 0) walk_word(w_cur, acc, my_tab, my_tab_w16, std::true_type(), cst);
                    else walk_word(w_cur, acc, my_tab, my_tab_w16, std::false_type(), cst);
                }
            }
        };
        if constexpr (PD && TPW > 1 && STREAM) {
            // (cohort steps of the narrow shapes: one kind of step -- walk_pd1 --, so the run words' loops serve, with their rows
            // requested an item ahead; a lane's first step IS its products, a lane without rows has none.  A single sample's
            // launches and search rounds -- lists in L2 / LDS -- take the two loops below: OptimizeLLK 5.41 against 5.58 ms)
            if (__any(rows == 0)) {
                if (rows == 0) {
#pragma unroll
                    for (int i = 0; i < BTL * 6; ++i) acc[i] = 1.0;
                }
            }
            if constexpr (PIPE) {
                const bool more = __any(rows > kPf);
                walk_block(0, more, std::true_type());
                if (more)
                    for (int s0 = kPf; s0 < rows; s0 += kPf) walk_block(s0, true, std::false_type());
                issue_rows(rec_n2, have_next);
                cst_nx = other_const(mt_next, have_next);
                rec_nx = rec_n2;
            } else {
                walk_block(0, true, std::true_type());
                for (int s0 = kPf; s0 < rows; s0 += kPf) walk_block(s0, true, std::false_type());
            }
        } else if constexpr (PD) {
            // The tile's ref rows, then its alt rows: TWO loops of one body each (as one loop with a test per row the
            // compiler kept the twelve products in different registers on the two paths and moved them all where the paths
            // meet).  The rows in flight are a window of kPf words that moves up one row per iteration.  In the paired shapes
            // the bounds are per half of the wave: the two tiles are neighbours of the sorted order and nearly always agree.
            int r = 0;
            // The rows in flight are a RING of kPf words with fixed slots -- row r in slot r % kPf -- and every step names its
            // slot at compile time.  (Before, the window MOVED up a register per row: the move of the newest word is a use of
            // it, so every row began by waiting for the load issued one row earlier.  Worth 0.6 % of a 48-point launch: the
            // lists' loads hide behind the table reads either way -- with made-up steps and no loads at all, VB2_ABLATE = 128,
            // the launch is no shorter; profiles/r06/ab_ablations.txt.)
            static_assert(kPf == 2, "the ring below has two slots");
            auto row_step = [&](auto slot_tag, auto alt0_tag, auto alt1_tag, auto first_tag) {
                constexpr int kSlot = decltype(slot_tag)::value;
                const uint32_t cur = w[kSlot];
                // (kFixedRing: the ring's slots are FIXED registers -- the row's two table addresses are taken from the word first, and
                // the refill is loaded into the register that held it: no copy of a loading register at the loops' heads and exits)
                constexpr bool kAt = kFixedRing && !decltype(first_tag)::value;
                uint32_t row_a0 = cur, row_a1 = my_tab;
                if constexpr (kAt) {
                    row_a0 = (decltype(alt0_tag)::value ? my_tab - (uint32_t)kPdAltOffset : my_tab) + (cur & 0xffffu);
                    row_a1 = (decltype(alt1_tag)::value ? my_tab - (uint32_t)kPdAltOffset : my_tab) + (cur >> 16);
                    asm volatile("" : "+v"(row_a0), "+v"(row_a1));
                }
                if constexpr (kAhead && decltype(first_tag)::value) w[kSlot] = w_ah[2];      // (row 2: requested with rows 0 and 1)
                else w[kSlot] = load_row(r + kPf);
                walk_pd(row_a0, acc, row_a1, alt0_tag, alt1_tag, first_tag);      // (not kAt: the word and the table's address)
                ++r;
            };
            const std::integral_constant<int, 0> kS0;
            const std::integral_constant<int, 1> kS1;
            // (the first row's first step IS the products: no initial values, no multiplies).  Rows [0, s1 / 2) hold two ref
            // steps, the rows behind two alt steps; if s1 is odd, row s1 / 2 holds the last ref and the first alt step.
            const int rows_ra = steps_ref >> 1;
            const std::false_type kRef;
            const std::true_type kAltT, kFirstT;
            const std::false_type kNotFirst;
            if (rows > 0) {
                if (steps_ref >= 2) row_step(kS0, kRef, kRef, kFirstT);
                else if (steps_ref == 1) row_step(kS0, kRef, kAltT, kFirstT);
                else row_step(kS0, kAltT, kAltT, kFirstT);
            } else {
#pragma unroll
                for (int i = 0; i < BTL * 6; ++i) acc[i] = 1.0;
            }
            // rows [r, end) of one kind: an odd row first, then pairs, then an even one
            auto rows_of_kind = [&](const int end, auto alt_tag) {
                if (r < end && (r & 1)) row_step(kS1, alt_tag, alt_tag, kNotFirst);
                while (r + 1 < end) {
                    row_step(kS0, alt_tag, alt_tag, kNotFirst);
                    row_step(kS1, alt_tag, alt_tag, kNotFirst);
                }
                if (r < end) row_step(kS0, alt_tag, alt_tag, kNotFirst);
            };
            rows_of_kind(rows_ra, kRef);
            if ((steps_ref & 1) && r == rows_ra && r < rows) {
                if (r & 1) row_step(kS1, kRef, kAltT, kNotFirst);
                else row_step(kS0, kRef, kAltT, kNotFirst);
            }
            rows_of_kind(rows, kAltT);
            if constexpr (PIPE) {
                issue_rows(rec_n2, have_next);
                cst_nx = other_const(mt_next, have_next);
                rec_nx = rec_n2;
            }
        } else if constexpr (PIPE) {
            // the first kPf rows outside any loop (loads in flight are counted, not drained); an item with more
            // rows -- wide quality alphabets -- refills the ring as before
            const bool more = __any(rows > kPf);
            walk_block(0, more, std::false_type());
            if (more)
                for (int s0 = kPf; s0 < rows; s0 += kPf) walk_block(s0, true, std::false_type());
            // this item's rows are walked: the next item's go out now, under the epilogue
            issue_rows(rec_n2, have_next);
            cst_nx = other_const(mt_next, have_next);
            rec_nx = rec_n2;
        } else if constexpr (PEEL) {
            if (rows > 0) {
                walk_block(0, true, std::true_type());
                for (int s0 = kPf; s0 < rows; s0 += kPf) walk_block(s0, true, std::false_type());
            } else {
#pragma unroll
                for (int i = 0; i < BTL * 6; ++i) acc[i] = cst;
            }
        } else {
            for (int s0 = 0; s0 < rows; s0 += kPf) walk_block(s0, true, std::false_type());
        }

        // ITEM_AHEAD: the last row's multiplies are issued -- the next item is drawn and its record requested
        uint32_t idx_ah = nitem;
        if constexpr (kAhead) {
            idx_ah = draw_item();
            request_rec_ahead(idx_ah);
        }
        __builtin_amdgcn_s_setprio(0);
#ifdef VB2_STAMP_CTRL
        if (stamps && lane == 0 && wave == 1 && !hook_blk) stamps[3] = wall_clock64();
#else
        if (stamps && lane == 0 && wave == 1) stamps[3] = wall_clock64();      // wave 1: out of its (first) read loop
#endif
        // ---- per-marker epilogue: this marker's likelihood as (mantissa, exponent) per point ----
        double lk_m[BTL];
        int lk_e[BTL];
        marker_lk(live, pos, acc, e0, e1, e2, udr, mur, my_ptq, lk_m, lk_e, cst);
        if constexpr (kAhead) request_rows_ahead();           // (the record has had the epilogue to arrive)
        if (!dyn) {
#pragma unroll
            for (int t = 0; t < BTL; ++t) {               // running product, renormalised lazily
                wave_prod[t].m *= lk_m[t];
                wave_prod[t].e += lk_e[t];
            }
            if (++nfactor == kLazyRenorm) renorm_wave();
            if (have_sched) {
                ++s_i;
                idx = PIPE ? idx_next : (s_i < s_end ? (uint32_t)sch.item[s_i] : nitem);
                continue;
            }
            // next round, direction reversed: the items are depth-sorted, and a plain deal would
            // hand wave 0 the deepest tile of every round
            ++round;
            idx = round * (uint32_t)nwave + ((round & 1u) ? (uint32_t)(nwave - 1 - wave) : (uint32_t)wave);
            continue;
        }
        // every MICRO-TILE's product goes to its own slot (not the item's): the slots and the
        // order they are multiplied in are then the same for every wave shape, so a point's value
        // does not depend on whether it was evaluated alone, among four, or in a group of eight.
        // Butterfly over the 16 lanes that share slot g: mantissas multiply (16 factors in
        // [0.5, 1): no underflow), exponents add as integers (three dwords per exchange, not four)
        if constexpr (kEpiScatter) {
            // (EPI_SCATTER: the step over marker bit 3 as a reduce-scatter -- lane_scatter8_u32: the even rows go on with point 0,
            // the odd rows with point 1 of the even-row lane sixteen below; all 64 lanes, the idle ones carry (1.0, 0))
            static_assert(BTL == 2, "two points per lane to scatter");
            unsigned h0, h1, l0, l1, x0, x1;
            lane_scatter8_u32((unsigned)__double2hiint(lk_m[0]), (unsigned)__double2hiint(lk_m[1]), h0, h1);
            lane_scatter8_u32((unsigned)__double2loint(lk_m[0]), (unsigned)__double2loint(lk_m[1]), l0, l1);
            lane_scatter8_u32((unsigned)lk_e[0], (unsigned)lk_e[1], x0, x1);
            double pm = __hiloint2double((int)h0, (int)l0) * __hiloint2double((int)h1, (int)l1);
            int pe = (int)x0 + (int)x1;
            // (the row steps written out: of a loop over `off` the compiler kept a run-time loop with a switch over the exchanges)
            auto row_step = [&](auto off) {                  // (an exchange inside a row: DPP moves, lane_xchg_i32)
                pm *= lane_xchg_f64(pm, decltype(off)::value, 0);
                pe += lane_xchg_i32(pe, decltype(off)::value, 0);
            };
            row_step(std::integral_constant<int, 4>());
            row_step(std::integral_constant<int, 2>());
            row_step(std::integral_constant<int, 1>());
            // the lanes of marker 0 store point 0 of their slot, the lanes sixteen above them (marker 8 of the slot of the other
            // parity) point 1 of THAT slot: {mantissa, exponent} in one 16-byte store, the slots' addresses as ever
            if ((m & 7) == 0 && have_tile) {
                const int t = m >> 3;
                const size_t o = ((((size_t)grp * NVS + vs) * ntile_blk + it) * NP + (g ^ t) * BTL + t) * 2;
                *reinterpret_cast<double2*>(tile_llk + o) = make_double2(pm, (double)pe);
            }
        } else {
        if constexpr (kEpiX8) {
            // (EPI_X8: the step over marker bit 3 without the LDS crossbar -- lane_pair8_u32; the steps over 4, 2, 1 follow below)
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                unsigned h0, h1, l0, l1, x0, x1;
                lane_pair8_u32((unsigned)__double2hiint(lk_m[t]), h0, h1);
                lane_pair8_u32((unsigned)__double2loint(lk_m[t]), l0, l1);
                lane_pair8_u32((unsigned)lk_e[t], x0, x1);
                lk_m[t] = __hiloint2double((int)h0, (int)l0) * __hiloint2double((int)h1, (int)l1);
                lk_e[t] = (int)x0 + (int)x1;
            }
        }
#pragma unroll
        for (int off = kEpiX8 ? 4 : 8; off >= 1; off >>= 1) {
            const int partner = lane_of(m ^ off, g4);
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                lk_m[t] *= lane_xchg_f64(lk_m[t], off, partner);
                lk_e[t] += lane_xchg_i32(lk_e[t], off, partner);
            }
        }
        if (m == 0 && have_tile) {
#pragma unroll
            for (int t = 0; t < BTL; ++t) {
                const size_t o = ((((size_t)grp * NVS + vs) * ntile_blk + it) * NP + g * BTL + t) * 2;
                tile_llk[o] = lk_m[t];
                tile_llk[o + 1] = (double)lk_e[t];
            }
        }
        }      // (!kEpiScatter)
        // next work item of this workgroup, whichever wave gets there first
        if constexpr (kAhead) idx = idx_ah;
        else idx = draw_item();
    }
    if (!dyn) {                                           // slots (wave, group): factor 1 if idle
        for (uint32_t grp = grp_wave; grp < (uint32_t)ngrp; ++grp) flush_wave(grp);
    }

    if constexpr (Config::ADDR_SCALAR && KSEL == 0) {
        // (kItemScalars: what only the code from here on needs of the kernel's arguments -- where the sums go -- is read again from the
        // kernel-argument segment instead of being kept in ten scalar registers across the item loop.  SplitKernArgs restates the
        // split kernels' parameter list, llk_kernels.hip: a by-value argument sits at its natural alignment, as a member does.)
        struct SplitKernArgs {
            DeviceLayout L;
            const double* points;
            int num_valid;
            double* partials;
            double* llk_out;
            unsigned int* ticket;
            unsigned long long* done_flag;
            unsigned long long done_seq;
            int ngrp;
        };
        static_assert(SPLIT != 0, "the parameter list restated here is the split kernels'");
        static_assert(offsetof(SplitKernArgs, partials) == sizeof(DeviceLayout) + 16 && offsetof(SplitKernArgs, done_seq) == sizeof(DeviceLayout) + 48,
                      "the hand-off's arguments behind the layout, the points and their count");
        typedef __attribute__((address_space(4))) const SplitKernArgs k_args;
        unsigned long long ka_ = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka_));
        k_args* const a_ = (k_args*)ka_;
        partials = a_->partials;
        llk_out = a_->llk_out;
        ticket = a_->ticket;
        done_flag = a_->done_flag;
        done_seq = a_->done_seq;
        num_valid = a_->num_valid;
    }
    if (stamps && lane == 0 && !hook_mine) atomicMax(&stamps[4], wall_clock64());   // the wave that is done with its tiles last
    // ---- deterministic block reduction -> one partial per (point, block) ----
    const uint32_t nres = dyn ? ntile_blk : (uint32_t)nwave;   // result slots per group
    // Every point at once, SIXTEEN lanes (one DPP row) per point: lane j of the row multiplies the slots j, j + 16, ... in index
    // order, then the row's sixteen products meet through four DPP moves -- mirror of the row, mirror of its halves, quad
    // permutes over distance 1 and 2: VALU moves, no trip through the LDS crossbar -- and the row's lane 0 takes the point's
    // only logarithm.  (Until round 4's second session a WAVE reduced a point, and a wave's three points of a 48-point launch
    // one after the other: 64-lane butterflies of ds_bpermutes with a renormalisation per step, 4.9 us between "last wave
    // done with its tiles" and "block reduced" in the launch's timeline -- tools/stamps.py.)  The order of the products is a
    // function of the slot count alone, the same for every wave shape and kernel, so a point's value still does not depend
    // on how it was evaluated.  Sixteen factors >= 2^-64 cannot underflow: one renormalisation after the butterfly.
    __syncthreads();
    {
        const uint32_t j16 = (uint32_t)lane & 15u;
        for (int b = tid >> 4; b < NVS * NPT; b += nthread >> 4) {          // (uniform over a row of 16 lanes)
            const int vsb = SPLIT ? b / NPT : 0, bl = b - vsb * NPT;
            const int grp = bl / NP, bb = bl - grp * NP;
            ScaledProd p{1.0, 0.0};
            const uint32_t nres_b = SPLIT ? nt_of((uint32_t)vsb) : nres;
            for (uint32_t i = j16; i < nres_b; i += 16) {
                const size_t o = ((((size_t)grp * NVS + vsb) * nres + i) * NP + bb) * 2;
                p.m *= tile_llk[o];
                p.e += tile_llk[o + 1];
                sp_renorm(p);                              // a slot can be as small as 2^-64
            }
            auto row_move = [&](double x, auto ctrl) -> double {
                constexpr int kCtrl = decltype(ctrl)::value;
                return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(x), kCtrl, 0xf, 0xf, false),
                                        __builtin_amdgcn_update_dpp(0, __double2loint(x), kCtrl, 0xf, 0xf, false));
            };
            auto row_step = [&](auto ctrl) {
                const double om = row_move(p.m, ctrl), oe = row_move(p.e, ctrl);
                p.m *= om;
                p.e += oe;
            };
            row_step(std::integral_constant<int, 0x140>());     // row_mirror:      lane j <- lane 15 - j
            row_step(std::integral_constant<int, 0x141>());     // row_half_mirror: lane j <- lane 7 - j of its half
            row_step(std::integral_constant<int, 0xB1>());      // quad_perm [1,0,3,2]
            row_step(std::integral_constant<int, 0x4E>());      // quad_perm [2,3,0,1]
            sp_renorm(p);
            // the only logarithm of this (workgroup, point): log(prod lk) = log(m) + e*ln2
            if (j16 == 0) red[b] = log_nonneg(p.m) + p.e * 6.93147180559945286227e-01;
        }
    }
    __syncthreads();
    if (VB2_STAMPS_OF(L) && tid == 0) {
        const unsigned long long t5 = wall_clock64();
        if (stamps) stamps[5] = t5;
        if (blk == 0 && nblk > 32 && !hook.no_collect()) VB2_STAMPS_OF(L)[20 * 8 + 7] += t5 - VB2_STAMPS_OF(L)[7];     // (accumulated: since "has the round")
    }
    }      // (!collect_only)
    // A result that the host waits for (done_flag: llk_out is mapped host memory) is stored THROUGH the caches (a relaxed
    // system-scope store); before the flag goes out the storing lanes wait for their stores' acknowledgements (vmcnt).
    // Round 3 stored plainly and then fenced -- __threadfence_system, an ACQ_REL counter and a RELEASE flag store: three
    // write-backs / invalidations of the whole L2 -- which was 10 of the 20 us an EMPTY cohort step took (round 4 ablation).
    auto put_result = [&](int b, double v) {
        if (done_flag) __hip_atomic_store(&llk_out[b], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else llk_out[b] = v;
    };
    if (ticket == nullptr) {                     // two-kernel mode: llk_finalize_kernel follows
        if (tid < NPT) partials[(size_t)tid * nblk + blk] = red[tid];
        return;
    }
    // SPLIT: one arrival ticket per share of the point groups, d_ticket[0 .. NVS) -- see below; the host's flag goes up behind the
    // LAST share's results: the shares' finalising workgroups are counted at d_ticket[NVS] the way a cohort step's samples are
    unsigned int* const my_ticket = SPLIT && ticket ? ticket + blk % (uint32_t)NVS : ticket;
    if constexpr (SPLIT != 0) {
        batch_done = ticket ? ticket + NVS : nullptr;
        batch_active = (unsigned int)NVS;
    }
    if (tag == 0) {
        // ---- single-launch mode A (large batches): the last workgroup to arrive sums all partials ----
        // Hand-off through 8-byte agent-scope atomics on both sides (write-through stores,
        // L1-bypassing loads), drained before the ticket is drawn: placement independent.
        if (tid < NVS * NPT) {
            // (SPLIT: the sums of this workgroup's points over the virtual blocks vb0 + j * vstep, where a plain launch has them)
            const int vsb = SPLIT ? tid / NPT : 0, bl = tid - vsb * NPT;
            __hip_atomic_store(&partials[(size_t)(p_off + bl) * nblk + (vb0 + (uint32_t)vsb * vstep)], red[tid],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned int* last_flag = queue;                                    // the queue is drained
        if constexpr (SPLIT != 0) {
            // One ticket per share j = blk % NVS of the point groups: the nblk / NVS workgroups of a share hold, between them, every
            // virtual block's sum of that share's points, so the share's last arriver adds up ITS points the moment its share is
            // complete -- a third of the arrivals on each counter, a third of the reload for each of three workgroups side by side.
            // A share's sums are all stored by wave 0 when they fit a wave (48 of a 48-point launch): that wave waits for its own
            // stores, draws the ticket behind them, and the workgroup meets at ONE barrier.
            if (NVS * NPT <= 64) {
                if (wave == 0) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lane == 0) {
                        const unsigned int t = __hip_atomic_fetch_add(my_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        *last_flag = (t == nblk / (uint32_t)NVS - 1) ? 1u : 0u;
                    }
                }
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    const unsigned int t = __hip_atomic_fetch_add(my_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *last_flag = (t == nblk / (uint32_t)NVS - 1) ? 1u : 0u;
                }
            }
        } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT);
            *last_flag = (t == nblk - 1) ? 1u : 0u;
        }
        }
        __syncthreads();
        if (*last_flag == 0u) return;
        // same summation order as llk_finalize_kernel: lane-strided, then a wave butterfly
        const int nbt = (int)nblk;
        // (a wave's points side by side -- three of a 48-point launch: their loads, each a trip to memory, are in flight
        // together, and so are their butterflies; every point's sum in the order it always had)
        // (SPLIT: the points [pt_lo, pt_hi) of this workgroup's share, one per wave of a 48-point launch)
        constexpr int kSide = SPLIT ? 1 : 3;
        const int pt_lo = SPLIT ? p_off : 0;
        const int pt_hi = SPLIT ? (p_off + NPT < num_valid ? p_off + NPT : num_valid) : num_valid;
        for (int b0 = pt_lo + wave; b0 < pt_hi; b0 += kSide * nwave) {
            double s[kSide];
#pragma unroll
            for (int u = 0; u < kSide; ++u) s[u] = 0;
            for (int base = 0; base < nbt; base += 8 * 64) {
                double x[kSide][8];
#pragma unroll
                for (int u = 0; u < kSide; ++u) {
                    const int b = b0 + u * nwave;
                    const double* p = partials + (size_t)(b < pt_hi ? b : b0) * nbt;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int i = base + q * 64 + lane;
                        x[u][q] = i < nbt ? __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                          : 0.0;
                    }
                }
#pragma unroll
                for (int u = 0; u < kSide; ++u)
#pragma unroll
                    for (int q = 0; q < 8; ++q) s[u] += x[u][q];
            }
#pragma unroll
            for (int u = 0; u < kSide; ++u) {
                const int b = b0 + u * nwave;
                const double t = wave_sum(s[u]);
                if (lane == 0 && b < pt_hi) put_result(b, t);
            }
        }
        if (tid == 0) __hip_atomic_store(my_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
    // ---- single-launch mode B (small batches, resident search): workgroup 0 collects all partials ----
    // Every workgroup publishes its NPT sums plus a check word (XOR of position-dependent word
    // hashes ^ mix(launch tag)) with write-through stores and is done: no drain, no arrival counter.
    // Workgroup 0 polls the NPT+1 words of each workgroup with L1-bypassing loads until the
    // check word fits -- stale words of an earlier launch or a half-arrived set fail it -- so
    // the hand-off costs one store propagation plus one read instead of three dependent
    // round trips through the fabric (store drain, ticket atomic, reload).
    unsigned long long* pw = reinterpret_cast<unsigned long long*>(partials);
    if (wave == 0 && !collect_only) {
        const unsigned long long bits = lane < NPT ? (unsigned long long)__double_as_longlong(red[lane]) : 0ull;
        // (the sums first: they do not wait for the check word; then the check word from lane 0, which has the XOR of the
        // NPT word hashes after log2(NPT) exchange steps -- a search round's four words: two quad permutes -- instead of a
        // 64-lane butterfly of six: the check word is what workgroup 0 waits for)
        if (lane < NPT)
            __hip_atomic_store(&pw[(size_t)lane * nblk + blk], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long x = lane < NPT ? word_hash(bits, (unsigned)lane) : 0ull;
        int top = 1;
        while (top < NPT) top <<= 1;
        for (int off = top >> 1; off >= 1; off >>= 1) x ^= __shfl_xor(x, off, 64);
        if (lane == 0)
            __hip_atomic_store(&pw[(size_t)NPT * nblk + blk], x ^ resident_mix(tag), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (collect_only ? false : (blk != 0 || hook.no_collect())) return;
    if (!hook.sum_stage()) __syncthreads();            // the table is dead: its space stages the partials
    const int nb = (int)nblk;
    double* stage = hook.sum_stage() ? hook.sum_stage() : lds;      // [NPT][nb]
    {
        const unsigned long long want = resident_mix(tag);
        const unsigned long long t_wait = wall_clock64();
        for (int b = tid; b < nb; b += nthread) {      // one thread per workgroup's set
            // (Not waiting for this workgroup's own set -- it is in its LDS already -- was measured twice and dropped: the set
            // that arrives last is not this workgroup's own.  HISTORY.md, rounds 3 and 4.)
            for (unsigned it = 0;; ++it) {
                // check word and the first words are requested together, NP + 1 loads in flight
                unsigned long long x = __hip_atomic_load(&pw[(size_t)NPT * nb + b], __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
                for (int w0 = 0; w0 < NPT; w0 += NP) {       // NPT is a multiple of NP (4 or 8)
                    unsigned long long v[NP];
#pragma unroll
                    for (int u = 0; u < NP; ++u)
                        v[u] = __hip_atomic_load(&pw[(size_t)(w0 + u) * nb + b], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                    for (int u = 0; u < NP; ++u) {
                        x ^= word_hash(v[u], (unsigned)(w0 + u));
                        stage[(size_t)(w0 + u) * nb + b] = __longlong_as_double((long long)v[u]);
                    }
                }
                if (x == want) break;
                // a quarter of a second (100 MHz ticks): a workgroup is missing -- part of the grid is not on the CUs
                // (a shared GPU).  The caller sees NaN and redoes the step with the arrival-ticket hand-off, which
                // waits for nobody.  (Round 2 waited two seconds: the hiccup of a co-residency failure is this wait.)
                if ((it & 63) == 63 && wall_clock64() - t_wait > kHandoffGiveUpTicks) {
                    for (int w = 0; w < NPT; ++w) stage[(size_t)w * nb + b] = __builtin_nan("");
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
    }
    __syncthreads();
    // same summation order as llk_finalize_kernel: lane-strided, then a wave butterfly
    for (int b = wave; b < num_valid; b += nwave) {
        const double* p = stage + (size_t)b * nb;
        double s = 0;
        for (int base = 0; base < nb; base += 8 * 64) {
            double x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = base + q * 64 + lane;
                x[q] = i < nb ? p[i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) s += x[q];
        }
        s = wave_sum(s);
        if (lane == 0) put_result(b, s);                 // NaN if a workgroup never reported
    }
    }
    if (VB2_STAMPS_OF(L) && tid == 0) {
        const unsigned long long t6 = wall_clock64();
        if (stamps) stamps[6] = t6;
        if ((collect_only || (blk == 0 && !hook.no_collect())) && nblk > 32) VB2_STAMPS_OF(L)[21 * 8 + 7] += t6 - VB2_STAMPS_OF(L)[7];
    }
    if (done_flag && !(kAblate & kAblNoSignal)) {
        // host hand-off without a stream synchronisation: results (in mapped host memory)
        // first, then the sequence number the host is spinning on.  In a multi-sample launch
        // the sample that completes last (batch_done counter) is the one that signals.
        // (every sample's results are acknowledged before its count goes up; the counter's own order then puts the
        // last sample's flag behind all of them.  Relaxed operations: nothing else of this launch is read by the host.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            bool signal = true;
            if (batch_done) {
                const unsigned int t = __hip_atomic_fetch_add(batch_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                signal = (t == batch_active - 1);
                if (signal) __hip_atomic_store(batch_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // (a system-scope RELEASE store, in this one workgroup: VERDICT r5 #6 -- no measurable cost against the relaxed store,
            // profiles/r06/ab_flag_release.txt; the host's NaN prefill of the result words stays as the second line)
            if (signal)
                __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace vb2

#endif  // VB2_EVAL_BODY_H_
