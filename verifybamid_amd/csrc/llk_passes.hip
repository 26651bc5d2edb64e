// llk_passes.hip -- the second unit of the evaluation kernels (device code: eval_body.h), compiled under LLVM's default
// instruction scheduler: llk_eval_passes_kernel (wide quality alphabets: the passes of one launch) and the cohort kernels
// llk_eval_multi_kernel, each with its launcher.  The iterative-ILP scheduler that the main unit llk_kernels.hip takes (+1.1 %
// on the 48-point launch, -1.2 % on OptimizeLLK) costs llk_eval_passes_kernel 7 % (118 codes: 566 -> 525 k evals/s) and the
// cohort steps of two and more points 1 % (a cohort search 3 %: 700 -> 678 samples/s).  Taking a kernel's address in its
// launcher is what instantiates it, here and nowhere else.
#include "llk_kernels.h"

#include <hip/hip_runtime.h>

#include "eval_body.h"

namespace vb2 {

// A call of more points than the LDS holds tables for -- wide quality alphabets: 118 codes x 8 points are 48.5 KB per point
// group, two groups per workgroup -- as ONE launch of several passes (round 4; before: one launch per 16 points, each with
// its own start-up, table build, tail and hand-off, ~10 us of a 41.6 us launch).  A pass is eval_body on its own points,
// its own stretch of the partial sums and its own arrival ticket; a workgroup that has delivered a pass's sums starts on the
// next pass at once -- only the workgroup that arrives last at a pass adds that pass up -- so the hand-offs of all passes but
// the last hide behind the other workgroups' work.  Same grid, same groups, same order as the separate launches: the same
// bits.  The results of the earlier passes are stored through the caches like the last one's (eval_body does that when it
// is given a flag to raise: theirs is a scratch word on the device), and acknowledged before the storing workgroup draws
// its next ticket, so the flag the host waits for is behind every pass's results.
// (the 8-point shape on the queue; run words: beside the compact exp table -- launch_passes)
template <int KSEL_, bool PD_>
struct PassesEval : EvalConfig {
    static constexpr int MODE = 2, QUEUE = 1, KSEL = KSEL_, ESH = PD_ ? 8 : 6;
    static constexpr bool PD = PD_;
};

template <int KSEL, bool PD = false>
__global__ void __launch_bounds__(Geom<2>::kMaxWaves * 64, Geom<2>::kWavesPerSimd)
llk_eval_passes_kernel(const DeviceLayout L, const double* __restrict__ points, int num_valid, int points_per_pass,
                       double* __restrict__ partials, double* __restrict__ llk_out, unsigned int* __restrict__ tickets,
                       unsigned long long* __restrict__ done_flag, unsigned long long done_seq,
                       unsigned long long* __restrict__ scratch_flag)
{
    const int stride = 2 * L.num_pc + 1;
    int pass = 0;
    for (int first = 0; first < num_valid; first += points_per_pass, ++pass) {
        const int left = num_valid - first;
        const int nv = left < points_per_pass ? left : points_per_pass;
        const bool last = left <= points_per_pass;
        if (pass > 0) __syncthreads();                      // the pass before is done with the workgroup's LDS
        eval_body<PassesEval<KSEL, PD>>(
            L, nullptr, 0, points + (size_t)first * stride, nv, partials + (size_t)first * gridDim.x, llk_out + first,
            tickets + pass, (last || !done_flag) ? done_flag : scratch_flag, done_seq, blockIdx.x, gridDim.x, nullptr, 0u,
            (nv + 7) / 8, 0ull, Schedule{nullptr, nullptr});
    }
}

// see llk_eval_passes_kernel.  Needs the work queue (a slot per item: the launches it replaces take it too at these sizes).
hipError_t launch_passes(const DeviceLayout& L, const double* d_points, int num_valid, int groups_per_launch,
                         double* d_partials, double* d_out, unsigned int* d_tickets,
                         unsigned long long* done_flag, unsigned long long done_seq, hipStream_t stream, bool* taken)
{
    *taken = false;
    if (L.known_af != nullptr) return hipSuccess;
    // point groups per pass: what fits beside the compact exp table (4 KiB instead of 16: see exp_nonpos) -- 118 codes: three
    // groups instead of two, i.e. 75 work items for a workgroup's 16 waves instead of 50 (5 rounds at 94 % instead of 4 at
    // 78 %) and two passes per 48 points instead of three
    constexpr int kCompactExpTabDoubles = 64 * 8;
    int g = kMaxGroups;
    LaunchGeom gm = launch_geom(L, 2, g);
    while (g > 1 && eval_shmem_np(L, 8, gm.grid, gm.block_waves, g, kCompactExpTabDoubles) > (size_t)kLdsLimitBytes) {
        --g;
        gm = launch_geom(L, 2, g);
    }
    const int ngroup = (num_valid + 7) / 8;
    const int npass = (ngroup + g - 1) / g;
    // only where the passes are fewer than the launches they replace (118 codes: 2 for 3, 125 -> 120 us per 48 points; 72
    // codes: 2 for 2 -- measured equal, 92.3 / 93.4 us, and the launches keep the conflict-free exp table)
    if (npass >= (ngroup + groups_per_launch - 1) / groups_per_launch) return hipSuccess;
    const int gpp = (ngroup + npass - 1) / npass;            // balanced: 6 groups at 4 per pass -> 3 + 3, not 4 + 2
    if (npass > kTicketScratchWord) return hipSuccess;
    gm = launch_geom(L, 2, gpp);
    if (!eval_is_dynamic(L, (uint32_t)gm.grid, gm.block_waves, gpp)) return hipSuccess;
    const size_t shmem = eval_shmem_np(L, 8, gm.grid, gm.block_waves, gpp, kCompactExpTabDoubles);
    if (shmem > (size_t)kLdsLimitBytes) return hipSuccess;
    const void* fn = L.pd ? (L.num_pc == 4 ? reinterpret_cast<const void*>(&llk_eval_passes_kernel<4, true>)
                             : L.num_pc == 2 ? reinterpret_cast<const void*>(&llk_eval_passes_kernel<2, true>)
                                             : reinterpret_cast<const void*>(&llk_eval_passes_kernel<0, true>))
                     : L.num_pc == 4 ? reinterpret_cast<const void*>(&llk_eval_passes_kernel<4>)
                     : L.num_pc == 2 ? reinterpret_cast<const void*>(&llk_eval_passes_kernel<2>)
                                     : reinterpret_cast<const void*>(&llk_eval_passes_kernel<0>);
    hipError_t e = raise_lds_limit(fn);
    if (e != hipSuccess) return e;
    DeviceLayout Lc = L;
    const double* a_points = d_points;
    int a_nv = num_valid, a_ppp = 8 * gpp;
    unsigned long long a_seq = done_seq;
    unsigned long long* a_scratch = reinterpret_cast<unsigned long long*>(d_tickets + kTicketScratchWord);
    void* args[] = {&Lc, &a_points, &a_nv, &a_ppp, &d_partials, &d_out, &d_tickets, &done_flag, &a_seq, &a_scratch};
    *taken = true;
    return hipLaunchKernel(fn, dim3(gm.grid), dim3(gm.block_waves * 64), args, shmem, stream);
}

// Multi-sample launch (BASELINE configs[4]: a cohort in lock-step): workgroup w serves sample
// w / bps as that sample's workgroup w % bps.  Every sample has its own layout, parameter rows,
// partials, ticket and output slot; samples with num_valid == 0 sit this step out.
// STATIC: every sample of the launch is known (on the host) to run the static deal: the item loop is compiled for it
// alone, and pipelined across items (eval_body: PIPE); else each sample's way of dealing is decided in the kernel.
template <int MODE_, bool W16_, int KSEL_, int STATIC, bool PD_>
struct MultiEval : EvalConfig {
    static constexpr int MODE = MODE_, QUEUE = STATIC ? 0 : -1, KSEL = KSEL_;
    static constexpr bool W16 = W16_, STREAM = true, PD = PD_;
};
template <int MODE, bool W16, int KSEL = 0, int STATIC = 0, bool PD = false>    // KSEL 2 / 4: every sample has that --NumPC and no known-AF column
__global__ void __launch_bounds__(Geom<MODE>::kMaxWaves * 64, Geom<MODE>::kWavesPerSimd)
llk_eval_multi_kernel(const DeviceLayout* __restrict__ layouts, const Schedule* __restrict__ scheds,
                      const double* __restrict__ points,
                      const int* __restrict__ num_valid, double* __restrict__ partials,
                      double* __restrict__ llk_out, unsigned int* __restrict__ tickets, int bps,
                      unsigned long long* __restrict__ done_flag, unsigned long long done_seq,
                      unsigned int* __restrict__ batch_done, unsigned int batch_active, int use_ticket,
                      const MultiInline mi)
{
    constexpr int NP = ModeNp<MODE>::value;
    const int s = blockIdx.x / bps;
    // (mi: the step's point counts and parameter rows as kernel arguments when they fit -- a step of 32 samples x 1 point
    // or 16 x 2 --: otherwise every workgroup reads them from mapped host memory, two dependent trips over PCIe, ~2.4 us
    // of the ~20 an empty step took in round 3)
    const int nv = (kAblate & kAblNoMap) ? NP : mi.count > 0 ? (int)mi.nv[s] : num_valid[s];
    if (nv <= 0) return;                                   // uniform for the workgroup
    const DeviceLayout L = layouts[s];
    const int stride = 2 * L.num_pc + 1;
    eval_body<MultiEval<MODE, W16, KSEL, STATIC, PD>>(L, mi.v + (size_t)s * NP * stride, mi.count, points + (size_t)s * NP * stride, nv,
                          partials + (size_t)s * (NP + 1) * bps, llk_out + (size_t)s * NP, tickets + s,
                          done_flag, done_seq, (uint32_t)(blockIdx.x % bps), (uint32_t)bps,
                          batch_done, batch_active, 1, use_ticket ? 0ull : done_seq,
                          scheds ? scheds[s] : Schedule{nullptr, nullptr});
}

// The cohort kernels of one wave shape
template <int MODE>
static hipError_t launch_multi_mode(const MultiLaunch& ml, hipStream_t stream)
{
    const dim3 grid(ml.num_sample * ml.bps), block(ml.block_waves * 64);
    // The 16-bit run lists (half the bytes of the run words from HBM) in every wave shape.  With round 4's decode -- one
    // byte permute + one 24-bit multiply per run, as many instructions as the 32-bit word's and + add -- and the item
    // loop compiled for the static deal alone (PIPE), they also pay where a step is VALU-bound: 32 C3 samples x 4 points
    // 202 -> 189 us, x 8 points 365 -> 346 us on one box (round 3, with a five-instruction decode and the deal decided
    // in the kernel: 231 -> 307 us, hence "1 and 2 points only" until round 5); 1 point 130.6 -> 117.5, 2 points 139.2 ->
    // 127.9 us when they came in.
    const int use_ticket = ml.force_ticket ? 1 : 0;
    auto go = [&](auto kernel) -> hipError_t {
        hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(kernel));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, block, ml.shmem, stream, ml.d_layouts, ml.d_scheds, ml.d_points,
                           ml.d_num_valid, ml.d_partials, ml.d_out, ml.d_tickets, ml.bps, ml.done_flag, ml.done_seq,
                           ml.d_batch_done, ml.batch_active, use_ticket, ml.inl);
        return hipGetLastError();
    };
    // (every shape also compiled for --NumPC 2 / 4 without a known-AF column: one-point steps of 32 samples 99 -> 94 us)
    if (ml.pd) {                      // (every sample a probability-domain context)
        if constexpr (MODE == 4 || MODE == 5) {    // (the one- and two-point shapes stream the 8-bit step lists when every sample has them: eval_body, walk_pd8)
            if (ml.w16) {
                if (ml.all_static) {
                    if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, true, 4, 1, true>);
                    if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, true, 2, 1, true>);
                    return go(&llk_eval_multi_kernel<MODE, true, 0, 1, true>);
                }
                if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, true, 4, 0, true>);
                if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, true, 2, 0, true>);
                return go(&llk_eval_multi_kernel<MODE, true, 0, 0, true>);
            }
        }
        if (ml.all_static) {
            if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, false, 4, 1, true>);
            if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, false, 2, 1, true>);
            return go(&llk_eval_multi_kernel<MODE, false, 0, 1, true>);
        }
        if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, false, 4, 0, true>);
        if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, false, 2, 0, true>);
        return go(&llk_eval_multi_kernel<MODE, false, 0, 0, true>);
    }
    if (ml.w16) {
        if (ml.all_static) {          // (the pipelined item loop: compiled for the static deal only)
            if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, true, 4, 1>);
            if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, true, 2, 1>);
            return go(&llk_eval_multi_kernel<MODE, true, 0, 1>);
        }
        if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, true, 4>);
        if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, true, 2>);
        return go(&llk_eval_multi_kernel<MODE, true>);
    }
    if (ml.ksel == 4) return go(&llk_eval_multi_kernel<MODE, false, 4>);
    if (ml.ksel == 2) return go(&llk_eval_multi_kernel<MODE, false, 2>);
    return go(&llk_eval_multi_kernel<MODE, false>);
}

hipError_t launch_llk_eval_multi(const MultiLaunch& ml, hipStream_t stream)
{
    // wave shape by points per sample: 8 -> MODE 2, 4 -> 3, 2 -> 5, 1 -> 4
    switch (ml.np) {
    case 8: return launch_multi_mode<2>(ml, stream);
    case 1: return launch_multi_mode<4>(ml, stream);
    case 2: return launch_multi_mode<5>(ml, stream);
    default: return launch_multi_mode<3>(ml, stream);
    }
}

}  // namespace vb2
