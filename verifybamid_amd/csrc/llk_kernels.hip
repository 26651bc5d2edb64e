// llk_kernels.hip -- the main unit of the evaluation kernels (device code: eval_body.h; work decomposition: there and in
// DESIGN.md), compiled under LLVM's iterative-ILP scheduler (csrc/Makefile: LLKFLAGS): the single-sample kernels
// llk_eval_kernel and llk_eval_split_kernel, the resident search kernel (resident_kernel.inc), llk_finalize_kernel and the
// small kernels, each with its launcher, the launch geometry and LDS sizes every launcher shares, and raise_lds_limit.
// The pass-per-group and cohort kernels, which that scheduler slows down, are in llk_passes.hip with their launchers; the
// host functions that need no kernel symbol are in llk_host.cpp.
#include "llk_kernels.h"

#include <hip/hip_runtime.h>

#include "eval_body.h"
#include "tunables.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <type_traits>

namespace vb2 {

// What each kernel of this unit takes of the evaluation body (eval_body.h, EvalConfig).  The plain launches: a row's table
// reads before its multiplies, in every probability-domain shape
template <int MODE_, int QUEUE_, int KSEL_, bool PD_>
struct PlainEval : EvalConfig {
    static constexpr int MODE = MODE_, QUEUE = QUEUE_, KSEL = KSEL_;
    static constexpr bool PD = PD_, READS_AHEAD = true;
};
// ... the split launch: the 8-point probability-domain shape on the queue with everything that shape has; its tile butterfly
// is a reduce-scatter, one point per lane (EPI_SCATTER), and its item loop's uniform address arithmetic is the scalar unit's
// (ADDR_SCALAR); six ways, where a workgroup has one point group for the whole launch, the projection's coefficients stay in the
// lanes of the DPP rows (COEF_DPP: --NumPC 4 and 2)
template <int KSEL_, int S>
struct SplitEval : EvalConfig {
    static constexpr int MODE = 2, QUEUE = 1, KSEL = KSEL_, SPLIT = S;
    static constexpr bool PD = true, READS_AHEAD = true, ITEM_AHEAD = true, EPI_X8 = true, EPI_SCATTER = true, ADDR_SCALAR = true;
    static constexpr bool COEF_DPP = S == kMaxGroups;
};

template <int MODE, int QUEUE, int KSEL = 0, bool PD = false>
__global__ void __launch_bounds__(Geom<MODE>::kMaxWaves * 64, Geom<MODE>::kWavesPerSimd)
llk_eval_kernel(const DeviceLayout L, const InlinePoints ip, const double* __restrict__ points,
                int num_valid, double* __restrict__ partials, double* __restrict__ llk_out,
                unsigned int* __restrict__ ticket, unsigned long long* __restrict__ done_flag,
                unsigned long long done_seq, int ngrp, unsigned long long tag, const Schedule sch)
{
    eval_body<PlainEval<MODE, QUEUE, KSEL, PD>>(L, ip.v, ip.count, points, num_valid, partials, llk_out, ticket,
                                                done_flag, done_seq, blockIdx.x, gridDim.x, nullptr, 0u, ngrp, tag, sch);
}

// see eval_body, SPLIT
template <int KSEL, int S>
__global__ void __launch_bounds__(Geom<2>::kMaxWaves * 64, Geom<2>::kWavesPerSimd)
llk_eval_split_kernel(const DeviceLayout L, const double* __restrict__ points, int num_valid, double* __restrict__ partials,
                      double* __restrict__ llk_out, unsigned int* __restrict__ ticket, unsigned long long* __restrict__ done_flag,
                      unsigned long long done_seq, int ngrp)
{
    eval_body<SplitEval<KSEL, S>>(L, nullptr, 0, points, num_valid, partials, llk_out, ticket, done_flag,
                                  done_seq, blockIdx.x, gridDim.x, nullptr, 0u, ngrp, 0ull,
                                  Schedule{nullptr, nullptr});
}

// ... in sets of kMaxGroups workgroups, one point group apiece (eval_body, SPLIT == kMaxGroups): launches of kMaxGroups groups
template <int KSEL>
__global__ void __launch_bounds__(Geom<2>::kMaxWaves * 64, Geom<2>::kWavesPerSimd)
llk_eval_split6_kernel(const DeviceLayout L, const double* __restrict__ points, int num_valid, double* __restrict__ partials,
                       double* __restrict__ llk_out, unsigned int* __restrict__ ticket, unsigned long long* __restrict__ done_flag,
                       unsigned long long done_seq, int ngrp)
{
    eval_body<SplitEval<KSEL, kMaxGroups>>(L, nullptr, 0, points, num_valid, partials, llk_out, ticket, done_flag,
                                           done_seq, blockIdx.x, gridDim.x, nullptr, 0u, ngrp, 0ull,
                                           Schedule{nullptr, nullptr});
}

#include "resident_kernel.inc"

// Sums the per-block partials in a fixed order -> bitwise reproducible: wave w takes
// points w, w+4, ...; lane l adds blocks l, l+64, ... (8 independent loads in flight),
// then a butterfly over the wave.
__global__ void __launch_bounds__(256)
llk_finalize_kernel(const double* __restrict__ partials, int nb, int num_point,
                    double* __restrict__ llk_out, unsigned long long* __restrict__ done_flag,
                    unsigned long long done_seq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < num_point; b += 4) {
        const double* p = partials + (size_t)b * nb;
        double s = 0;
        for (int base = 0; base < nb; base += 8 * 64) {
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * 64 + lane;
                x[u] = i < nb ? p[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += x[u];
        }
        s = wave_sum(s);
        if (lane == 0) {
            if (done_flag) __hip_atomic_store(&llk_out[b], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else llk_out[b] = s;
        }
    }
    if (done_flag) {                    // (stores through the caches, acknowledged, then the flag: see eval_body)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------
bool eval_takes_the_queue(const DeviceLayout& L, int nblk, int nwave, int ngrp)
{
    return eval_is_dynamic(L, (uint32_t)nblk, nwave, ngrp);
}

static size_t split_shmem(const DeviceLayout& L, int grid, int block_waves, int ngrp_total, int ways);

LaunchGeom launch_geom(const DeviceLayout& L, int btl, int ngrp)
{
    const int max_waves = Geom<2>::kMaxWaves;
    const int grid_target = Geom<2>::kBlocksPerCU * L.num_cu;
    (void)btl;
    int bw = (L.num_mt + grid_target - 1) / grid_target;
    bw = bw < 4 ? 4 : (bw > max_waves ? max_waves : bw);
    int grid = (L.num_mt + bw - 1) / bw;
    grid = grid < 1 ? 1 : (grid > grid_target ? grid_target : grid);
    if (L.pd && grid > (L.num_mt >> 1)) grid = L.num_mt >> 1 > 0 ? L.num_mt >> 1 : 1;      // (a workgroup owns pairs of tiles)
    // A dictionary whose tables of a full launch (kMaxGroups groups) do not fit PAIRS of workgroups is split three ways
    // (eval_body, SPLIT): the grid -- the same for every launch kind of the context, so that a point's sum is the same bits in
    // all of them -- is then a multiple of 6 (256 CUs: 252 workgroups).  (The rule asks about pairs and nothing else: that sets
    // of six exist -- split_ways -- does not enter, the grid of a context is what it was before them.)
    if (L.pd && grid >= 12 && split_shmem(L, grid & ~1, max_waves, kMaxGroups, 2) > (size_t)kLdsLimitBytes)
        grid -= grid % 6;
    // Several point groups: a workgroup's work items are (tile, group) pairs, so a small sample -- a marker shard
    // of an 8-GPU run: 12 500 markers = 3-4 tiles per workgroup -- still has work for 16 waves, and 1 024 threads
    // to build its six tables with (4-wave workgroups took 47 us for a 48-point launch on 12 500 markers, against
    // 74 us on 100 000).  The grid, hence the tiles a workgroup owns, stays what it was.
    if (ngrp > 1) {
        const int items = (int)owned_most(L.pd ? 1 : 0, (uint32_t)L.num_mt, (uint32_t)grid) * ngrp;
        if (items > bw) bw = items > max_waves ? max_waves : items;
    }
    return LaunchGeom{grid, bw};
}

// More than 64 KiB of dynamic LDS is an opt-in per kernel function AND per device (the function
// object is per device in the runtime), so the flag is kept per (function slot, device).
// (keyed by the function's address and the device -- ADVICE r3: the hand-numbered slots of round 3 were one
// specialisation away from a collision --: an open-addressed table of (function, device) keys, lock-free, a few dozen
// entries ever)
hipError_t raise_lds_limit(const void* fn)
{
    constexpr unsigned kCap = 1024;
    static std::atomic<uintptr_t> keys[kCap];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uintptr_t key = (reinterpret_cast<uintptr_t>(fn) << 8) ^ (uintptr_t)(dev + 1);     // (never 0)
    unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 40) % kCap;
    for (unsigned probe = 0; probe < kCap; ++probe, h = (h + 1) % kCap) {
        const uintptr_t seen = keys[h].load(std::memory_order_acquire);
        if (seen == key) return hipSuccess;
        if (seen == 0) break;
    }
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimitBytes);
    if (e != hipSuccess) return e;
    for (unsigned probe = 0; probe < kCap; ++probe, h = (h + 1) % kCap) {
        uintptr_t expect = 0;
        if (keys[h].compare_exchange_strong(expect, key, std::memory_order_acq_rel) || expect == key) break;
    }
    return hipSuccess;
}

// the single-sample kernel of a wave shape: one per way of dealing (queue / static); --NumPC 2 and 4 without a known-AF column
// have kernels of their own (the static deal of the search shapes only in the general form: a search takes the queue)
template <int MODE, bool PD>
static const void* eval_kernel_fn(int ksel, bool dyn)
{
    constexpr int kStaticQ = MODE == 2 ? 0 : 1;     // (never selected for MODE != 2: ksel is 0 there)
    return ksel == 4 ? (dyn ? reinterpret_cast<const void*>(&llk_eval_kernel<MODE, 1, 4, PD>)
                            : reinterpret_cast<const void*>(&llk_eval_kernel<MODE, kStaticQ, 4, PD>))
           : ksel == 2 ? (dyn ? reinterpret_cast<const void*>(&llk_eval_kernel<MODE, 1, 2, PD>)
                              : reinterpret_cast<const void*>(&llk_eval_kernel<MODE, kStaticQ, 2, PD>))
           : dyn  ? reinterpret_cast<const void*>(&llk_eval_kernel<MODE, 1, 0, PD>)
                  : reinterpret_cast<const void*>(&llk_eval_kernel<MODE, 0, 0, PD>);
}

template <int MODE>
static hipError_t launch_btl(const DeviceLayout& L, const double* d_points, const double* h_points,
                             int num_valid, int ngrp,
                             double* d_partials, double* d_out, unsigned int* d_ticket,
                             unsigned long long* done_flag, unsigned long long done_seq,
                             unsigned long long tag, hipStream_t stream, ScheduleProvider* sp)
{
    constexpr int NP = ModeNp<MODE>::value;     // points per group
    const LaunchGeom gm = launch_geom(L, MODE == 2 ? 2 : 1, ngrp);
    const Schedule sch = sp ? sp->get(MODE, ngrp, gm.grid, gm.block_waves) : Schedule{nullptr, nullptr};
    const size_t shmem = eval_shmem_np(L, NP, gm.grid, gm.block_waves, ngrp);
    // (the group cap of launch_llk_eval is worked out on the geometry of a kMaxGroups launch; this launch's own
    // geometry -- fewer groups, maybe fewer waves -- needs no more LDS than that today, but nothing else says so)
    if (shmem > (size_t)kLdsLimitBytes) return hipErrorInvalidConfiguration;
    // one kernel per way of dealing (queue / static); --NumPC 2 and 4 without a known-AF column have kernels of their own
    // (the static deal of the search shapes only in the general form: a search takes the queue)
    const bool dyn = eval_is_dynamic(L, (uint32_t)gm.grid, gm.block_waves, ngrp);
    const int ksel = (L.known_af == nullptr && (MODE == 2 || dyn)) ? (L.num_pc == 4 ? 4 : L.num_pc == 2 ? 2 : 0) : 0;
    const void* fn = L.pd ? eval_kernel_fn<MODE, true>(ksel, dyn) : eval_kernel_fn<MODE, false>(ksel, dyn);
    {
        hipError_t e = raise_lds_limit(fn);
        if (e != hipSuccess) return e;
    }
    InlinePoints ip;
    ip.count = 0;
    const int ndbl = num_valid * (2 * L.num_pc + 1);
    if (h_points && ndbl <= kInlinePointDoubles) {      // small batch with host-visible values
        ip.count = ndbl;
        for (int i = 0; i < ndbl; ++i) ip.v[i] = h_points[i];
    }
    {
        DeviceLayout Lc = L;
        const double* a_points = d_points;
        int a_nv = num_valid, a_ngrp = ngrp;
        unsigned long long a_seq = done_seq, a_tag = tag;
        Schedule a_sch = sch;
        void* args[] = {&Lc, &ip, &a_points, &a_nv, &d_partials, &d_out, &d_ticket, &done_flag, &a_seq, &a_ngrp, &a_tag, &a_sch};
        return hipLaunchKernel(fn, dim3(gm.grid), dim3(gm.block_waves * 64), args, shmem, stream);
    }
}

// LDS of a split launch's workgroup (eval_body, SPLIT = ways): the tables of its share of the groups, the result slots of `ways` virtual blocks
static size_t split_shmem(const DeviceLayout& L, int grid, int block_waves, int ngrp_total, int ways)
{
    // (a workgroup of a plain launch of this grid with 1 / ways of the groups, plus the other virtual blocks' result slots -- as
    // many as the first's -- and their sums)
    const size_t per = (size_t)((ngrp_total + ways - 1) / ways);
    const size_t slots1 = (size_t)owned_most(1, (uint32_t)L.num_mt, (uint32_t)(grid >= 1 ? grid : 1)) * per;
    return eval_shmem_np(L, 8, grid >= 1 ? grid : 1, block_waves, (int)per) + sizeof(double) * ((size_t)(ways - 1) * 2 * slots1 * 8 + (size_t)(ways - 1) * 8 * per);
}
// ways of a split launch of ngrp groups (0: none fits).  Sets of kMaxGroups workgroups with ONE group apiece where a launch
// has that many groups, the grid divides, the LDS holds it and the set's items fit the queue -- the same items, slots and sums
// as three ways, half the table entries per workgroup; else the fewest workgroups per set whose tables fit.
// max_ways: 3 = what the dictionary and the grid are sized on (pd_row_budget, launch_geom), Tunables::split = 3.
static int split_ways(const DeviceLayout& L, const LaunchGeom& gm, int ngrp, int max_ways = kMaxGroups)
{
    constexpr int kSix = kMaxGroups;
    if (max_ways >= kSix && tunables().split == 1 && ngrp == kSix && gm.grid >= kSix && gm.grid % kSix == 0 &&
        split_shmem(L, gm.grid, gm.block_waves, ngrp, kSix) <= (size_t)kLdsLimitBytes &&
        (uint32_t)kSix * owned_most(1, (uint32_t)L.num_mt, (uint32_t)gm.grid) <= (uint32_t)(L.dyn_limit * gm.block_waves))
        return kSix;
    for (int ways = 2; ways <= 3; ++ways) {
        if (gm.grid < ways || gm.grid % ways || (ways == 3 && tunables().split == 2)) continue;
        const int per = (ngrp + ways - 1) / ways;
        if (per * (ways - 1) >= ngrp) continue;            // (a workgroup of the set would have no group)
        if (split_shmem(L, gm.grid, gm.block_waves, ngrp, ways) <= (size_t)kLdsLimitBytes) return ways;
    }
    return 0;
}

// (test aid: split launches of this process by their ways -- vb2_debug_split_launches)
static std::atomic<long long> g_split_launches[kMaxGroups + 1];

// see eval_body, SPLIT.  *taken = false: the geometry does not allow it (the caller falls back to passes / several launches)
static hipError_t launch_split(const DeviceLayout& L, const double* d_points, int num_valid, double* d_partials, double* d_out,
                               unsigned int* d_ticket, unsigned long long* done_flag, unsigned long long done_seq,
                               hipStream_t stream, bool* taken)
{
    *taken = false;
    if (!L.pd) return hipSuccess;
    const int ngrp = (num_valid + 7) / 8;
    if (ngrp < 2) return hipSuccess;
    const LaunchGeom gm = launch_geom(L, 2, ngrp);      // (a set of workgroups has the items of one workgroup of a plain launch, `ways` times)
    const int ways = split_ways(L, gm, ngrp);
    if (ways == 0) return hipSuccess;
    // every item through the queue, a slot apiece
    const uint32_t tiles_set = (uint32_t)ways * owned_most(1, (uint32_t)L.num_mt, (uint32_t)gm.grid);
    if (tiles_set * (uint32_t)((ngrp + ways - 1) / ways) > (uint32_t)(L.dyn_limit * gm.block_waves)) return hipSuccess;
    const size_t shmem = split_shmem(L, gm.grid, gm.block_waves, ngrp, ways);
    const int ksel = L.known_af == nullptr ? (L.num_pc == 4 ? 4 : L.num_pc == 2 ? 2 : 0) : 0;
    const void* fn = ways == kMaxGroups
                         ? (ksel == 4 ? reinterpret_cast<const void*>(&llk_eval_split6_kernel<4>)
                            : ksel == 2 ? reinterpret_cast<const void*>(&llk_eval_split6_kernel<2>)
                                        : reinterpret_cast<const void*>(&llk_eval_split6_kernel<0>))
                     : ways == 2 ? (ksel == 4 ? reinterpret_cast<const void*>(&llk_eval_split_kernel<4, 2>)
                                  : ksel == 2 ? reinterpret_cast<const void*>(&llk_eval_split_kernel<2, 2>)
                                              : reinterpret_cast<const void*>(&llk_eval_split_kernel<0, 2>))
                               : (ksel == 4 ? reinterpret_cast<const void*>(&llk_eval_split_kernel<4, 3>)
                                  : ksel == 2 ? reinterpret_cast<const void*>(&llk_eval_split_kernel<2, 3>)
                                              : reinterpret_cast<const void*>(&llk_eval_split_kernel<0, 3>));
    hipError_t e = raise_lds_limit(fn);
    if (e != hipSuccess) return e;
    DeviceLayout Lc = L;
    const double* a_points = d_points;
    int a_nv = num_valid, a_ngrp = ngrp;
    unsigned long long a_seq = done_seq;
    void* args[] = {&Lc, &a_points, &a_nv, &d_partials, &d_out, &d_ticket, &done_flag, &a_seq, &a_ngrp};
    *taken = true;
    g_split_launches[ways].fetch_add(1, std::memory_order_relaxed);
    return hipLaunchKernel(fn, dim3(gm.grid), dim3(gm.block_waves * 64), args, shmem, stream);
}

long long split_launches(int ways)
{
    return ways >= 0 && ways <= kMaxGroups ? g_split_launches[ways].load(std::memory_order_relaxed) : -1;
}

hipError_t launch_llk_eval(const DeviceLayout& L, int num_point, const double* d_points,
                           const double* h_points, double* d_partials, double* d_out,
                           unsigned int* d_ticket,
                           unsigned long long* done_flag, unsigned long long done_seq,
                           unsigned long long* tag_counter, hipStream_t stream, int reduce_override,
                           ScheduleProvider* sched)
{
    const Tunables& tn = tunables();
    unsigned int* tk = tn.single_launch ? d_ticket : nullptr;
    const int reduce_mode = reduce_override ? reduce_override : tn.reduce;
    const int stride = 2 * L.num_pc + 1;
    int done = 0;
    while (done < num_point) {
        const int left = num_point - done;
        const double* p = d_points + (size_t)done * stride;
        const double* hp = h_points ? h_points + (size_t)done * stride : nullptr;
        // up to max_groups x 8 points per launch (more points amortise the fixed costs)
        const LaunchGeom gm2 = launch_geom(L, 2, kMaxGroups);
        // (8-point groups need the wide table rows; a context whose dictionary is too big for
        // 16-bit offsets into wide rows has narrow ones and evaluates 4 points per launch)
        const int cap = L.row_bytes == kRowBytesWide ? 8 * max_groups(L, 2, gm2.grid, gm2.block_waves) : 4;
        // probability-domain contexts: pairs of workgroups split the point groups (Tunables::split 0: passes)
        if (tn.split && L.pd && tk && reduce_mode != 2 && cap >= 8 && left > cap) {
            const int take = left < kMaxPointsPerLaunch ? left : kMaxPointsPerLaunch;
            bool taken = false;
            unsigned long long* dfp = (done + take >= num_point) ? done_flag : nullptr;
            hipError_t es = launch_split(L, p, take, d_partials, d_out + done, tk, dfp, done_seq, stream, &taken);
            if (es != hipSuccess) return es;
            if (taken) {
                done += take;
                continue;
            }
        }
        // more points than one launch's tables hold: the passes of ONE launch (Tunables::passes 0: a launch per `cap` points)
        if (tn.passes && tk && reduce_mode != 2 && L.row_bytes == kRowBytesWide && cap >= 8 && left > cap) {
            const int take = left < kMaxPointsPerLaunch ? left : kMaxPointsPerLaunch;
            bool taken = false;
            unsigned long long* dfp = (done + take >= num_point) ? done_flag : nullptr;
            hipError_t ep = launch_passes(L, p, take, cap / 8, d_partials, d_out + done, tk, dfp, done_seq, stream, &taken);
            if (ep != hipSuccess) return ep;
            if (taken) {
                done += take;
                continue;
            }
        }
        const int step = left < cap ? left : cap;
        const int ngrp = step > 4 ? (step + 7) / 8 : 1;
        unsigned long long* df = (done + step >= num_point) ? done_flag : nullptr;   // last launch signals
        unsigned long long* df_eval = tk ? df : nullptr;
        hipError_t e;
        // hand-off protocol: tagged sets for <= 16 points (one fabric round trip less: latency matters -- 8 points 18.6 ->
        // 16.4 us, 16 points 27.7 -> 26.6 us), arrival ticket for bigger batches (32 points 45.5 against 47.6 us, 48 points
        // 64.3 against 68.5 us: there workgroup 0's polling passes cost more than the ticket's third trip)
        const bool tagged = reduce_mode == 2 || (reduce_mode == 0 && step <= tn.tagged_max);
        const unsigned long long tag = tagged ? ++*tag_counter : 0ull;   // unique per launch on this buffer
        if (step > 4)
            e = launch_btl<2>(L, p, hp, step, ngrp, d_partials, d_out + done, tk, df_eval, done_seq, tag, stream, sched);
        else if (step == 1)
            e = launch_btl<4>(L, p, hp, step, 1, d_partials, d_out + done, tk, df_eval, done_seq, tag, stream, sched);
        else
            e = launch_btl<3>(L, p, hp, step, 1, d_partials, d_out + done, tk, df_eval, done_seq, tag, stream, sched);
        if (e != hipSuccess) return e;
        if (!tk) {
            hipLaunchKernelGGL(llk_finalize_kernel, dim3(1), dim3(256), 0, stream, d_partials,
                               launch_geom(L, step > 4 ? 2 : 1).grid, step, d_out + done, df, done_seq);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        done += step;
    }
    return hipSuccess;
}

size_t eval_shmem_np(const DeviceLayout& L, int np, int nblk, int block_waves, int ngrp, int exp_tab_doubles)
{
    if (exp_tab_doubles <= 0) exp_tab_doubles = kExpTabDoubles;
    const size_t NP = (size_t)np, G = (size_t)ngrp;
    const size_t items = (size_t)owned_most(L.pd ? 1 : 0, (uint32_t)L.num_mt, (uint32_t)nblk) * G;      // (one slot per micro-tile and group)
    const size_t fixed_tabs = L.pd ? 0 : (size_t)exp_tab_doubles + (size_t)kLogTabDoubles;      // (no exp / log table in the probability domain)
    const size_t slots = items <= (size_t)L.dyn_limit * block_waves ? items : (size_t)block_waves * G;
    const size_t bytes = sizeof(double) * (G * (L.num_code + 1) * (size_t)(L.row_bytes / 8) + G * NP + 2 +
                                           G * NP * (2 * L.num_pc + 1) + 1 + G * NP * 2 * L.num_pc +
                                           1 + 2 * (size_t)L.num_prim +
                                           fixed_tabs + 2 * slots * NP);
    // workgroup 0 stages every workgroup's partial sums ([points][workgroups]) over the dead table
    const size_t stage = sizeof(double) * G * NP * (size_t)nblk;
    return bytes > stage ? bytes : stage;
}

int pd_row_budget(int num_marker, int num_pc, int num_cu)
{
    DeviceLayout T;
    std::memset(&T, 0, sizeof(T));
    T.pd = 1;
    T.row_bytes = kRowBytesWide;
    T.num_pc = num_pc;
    T.num_mt = ((num_marker + kMtMarkers - 1) / kMtMarkers + 1) & ~1;
    T.num_cu = num_cu;
    T.dyn_limit = tunables().dyn_tiles;
    // (the tables of a 48-point launch: all six groups' in one workgroup, or -- Tunables::split = ways -- 6 / ways in each of a set)
    for (int rows = kMaxWideCodes; rows > 1; --rows) {
        T.num_code = T.num_prim = rows;
        const LaunchGeom gm = launch_geom(T, 2, kMaxGroups);
        // (priced on at most THREE ways, whatever a launch then takes: on six the budget would grow, every probability-domain
        // context would get another dictionary and every value other bits)
        const int ways = split_ways(T, gm, kMaxGroups, 3);
        const size_t need = (tunables().split != 0 && ways >= 2) ? split_shmem(T, gm.grid, gm.block_waves, kMaxGroups, ways)
                                  : eval_shmem_np(T, 8, gm.grid, gm.block_waves, kMaxGroups);
        if (need <= (size_t)kLdsLimitBytes) return rows;
    }
    return 1;
}

size_t eval_shmem_bytes(const DeviceLayout& L, int btl, int nblk, int block_waves, int ngrp)
{
    return eval_shmem_np(L, 4 * btl, nblk, block_waves, ngrp);
}

// Largest number of point groups one launch may carry: LDS (160 KiB per CU) and 4 at most.
int max_groups(const DeviceLayout& L, int btl, int nblk, int block_waves)
{
    int g = kMaxGroups;
    while (g > 1 && eval_shmem_bytes(L, btl, nblk, block_waves, g) > kLdsLimitBytes) --g;
    return g;
}

// (the kernels of the flatten -- classify_kernel, pack_layout_kernel, pack_sched_kernel, pack_codes16_kernel -- are in
// flatten_kernels.hip)

size_t resident_state_doubles(int nmax, int num_pc)
{
    return 8 + DeviceSimplex::lds_doubles(nmax, num_pc) + (size_t)resident_words(num_pc) + 2 +
           (size_t)resident_stage_doubles(nmax, num_pc);
}

uint32_t resident_cache_rows(const uint32_t* rows, int num_mt, int nblk, int own_shift)
{
    uint32_t most = 0;
    for (int b = 0; b < nblk; ++b) {
        const uint32_t ntile = owned_count(own_shift, (uint32_t)num_mt, (uint32_t)b, (uint32_t)nblk);
        uint32_t off = 0, prev = 0;
        for (uint32_t it = 0; it < ntile; ++it) {
            const uint32_t t = owned_tile(own_shift, (uint32_t)b, (uint32_t)nblk, it);
            if (t >= (uint32_t)num_mt) break;
            const uint32_t start = cache_start(own_shift != 0, off, prev, it);
            off = start + rows[t];
            prev = start;
        }
        most = std::max(most, off);
    }
    return most + 4;        // slack: the read loop requests up to kPrefetchL2 rows past a tile's last
}

hipError_t launch_llk_resident(const DeviceLayout& L, ResidentArgs* ra_io, double* d_partials,
                               unsigned int* d_ticket, hipStream_t stream, bool* cooperative)
{
    const LaunchGeom gm = launch_geom(L, 1);
    // dynamic LDS: the evaluation body's, then workgroup 0's search state (16-byte aligned)
    size_t shmem = (eval_shmem_bytes(L, 1, gm.grid, gm.block_waves, 1) + 15) / 16 * 16;
    ResidentArgs& ra = *ra_io;           // state_off / state_nmax and the LDS areas behind the state are filled in here
    ra.state_off = (int32_t)(shmem / sizeof(double));
    shmem += sizeof(double) * resident_state_doubles(ra.state_nmax, L.num_pc);
    if (shmem > (size_t)kLdsLimitBytes && ra.state_nmax > 0) {      // no room: search on the host
        ra.state_nmax = 0;
        shmem = ra.state_off * sizeof(double) + sizeof(double) * resident_state_doubles(0, L.num_pc);
    }
    if (shmem > (size_t)kLdsLimitBytes || gm.grid > L.num_cu) return hipErrorInvalidConfiguration;
    // workgroup 0's own staging area for the partial sums, if there is room (else over the dead tables, as in round 3)
    ra.sum_stage_off = 0;
    {
        const size_t at = (shmem + 15) / 16 * 16, need = sizeof(double) * 4 * (size_t)gm.grid;
        if (at + need <= (size_t)kLdsLimitBytes) {
            ra.sum_stage_off = (int32_t)(at / sizeof(double));
            shmem = at + need;
        }
    }
    const bool dyn = eval_is_dynamic(L, (uint32_t)gm.grid, gm.block_waves, 1);
    const int ksel = (dyn && L.known_af == nullptr) ? (L.num_pc == 4 ? 4 : L.num_pc == 2 ? 2 : 0) : 0;
    // the run-list cache: the paired shape on the work queue (what a search on one device runs), at most 8 tiles per wave
    bool lcache = false;
    ra.cache_off = 0;
    if (ra.cache_rows > 0 && dyn && ra.cache_tiles <= 8 * gm.block_waves) {
        ra.cache_tiles = (ra.cache_tiles + 1) & ~1;
        const size_t at = (shmem + 15) / 16 * 16;
        const size_t need = (size_t)ra.cache_tiles * 8 + (size_t)ra.cache_rows * kMtMarkers * (L.pd ? 4 : 8);
        if (at + need <= (size_t)kLdsLimitBytes) {
            ra.cache_off = (int32_t)(at / sizeof(double));
            shmem = at + need;
            lcache = true;
        }
    }
    if (!lcache) ra.cache_rows = 0;
    auto pick = [&](auto pd_tag) -> const void* {
        constexpr bool kPd = decltype(pd_tag)::value;
        return lcache ? (ksel == 4 ? reinterpret_cast<const void*>(&llk_resident_kernel<1, 4, true, kPd>)
                         : ksel == 2 ? reinterpret_cast<const void*>(&llk_resident_kernel<1, 2, true, kPd>)
                                     : reinterpret_cast<const void*>(&llk_resident_kernel<1, 0, true, kPd>))
               : ksel == 4 ? reinterpret_cast<const void*>(&llk_resident_kernel<1, 4, false, kPd>)
               : ksel == 2 ? reinterpret_cast<const void*>(&llk_resident_kernel<1, 2, false, kPd>)
               : dyn       ? reinterpret_cast<const void*>(&llk_resident_kernel<1, 0, false, kPd>)
                           : reinterpret_cast<const void*>(&llk_resident_kernel<0, 0, false, kPd>);
    };
    const void* fn = L.pd ? pick(std::true_type()) : pick(std::false_type());
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimitBytes);
    if (e != hipSuccess) return e;
    // Every workgroup must be on a CU at the same time (they all wait for the control wave and for each other's sums).
    // The grid is at most one 1024-thread workgroup per CU; a cooperative launch makes the runtime GUARANTEE that it is
    // resident as a whole (hipLaunchCooperativeKernel), where a plain one merely finds it so on a device that runs
    // nothing else.  Cooperative is the default.  Plain launches remain for: a process under a profiler (ROCm 7.2's
    // rocprofv3 crashes in its exit handler after a cooperative launch: the caller checks profiler_attached()), a
    // runtime that refuses the cooperative launch, and Tunables::coop = 0 -- the bounded waits on both sides then turn
    // a partly resident grid into a retry with plain per-step launches, not a hang.
    // one workgroup more for the control wave where the grid leaves a CU free (resident_kernel.inc: extra_ctl)
    ra.extra_ctl = (tunables().ctl_block != 0 && ra.state_nmax > 0 && dyn && gm.grid + 1 <= L.num_cu && gm.grid > 4) ? 1 : 0;
    const unsigned launch_grid = (unsigned)gm.grid + (ra.extra_ctl ? 1u : 0u);
    DeviceLayout Lc = L;
    ResidentArgs rc = ra;
    void* args[] = {&Lc, &rc, &d_partials, &d_ticket};
    if (cooperative && *cooperative) {
        e = hipLaunchCooperativeKernel(fn, dim3(launch_grid), dim3(gm.block_waves * 64), args, (unsigned int)shmem, stream);
        if (e == hipSuccess) return e;
        (void)hipGetLastError();
        *cooperative = false;
    }
    return hipLaunchKernel(fn, dim3(launch_grid), dim3(gm.block_waves * 64), args, shmem, stream);
}

// After a collective on the same stream: the reduced values go to mapped host memory, then the sequence
// number the host spins on -- the marker-shard step needs no device-to-host copy call and no stream
// synchronisation (shard.cpp).  One wave; every lane fences its own stores before the flag is written.
__global__ void __launch_bounds__(64)
publish_kernel(const double* __restrict__ src, double* __restrict__ dst_mapped, int n,
               unsigned long long* __restrict__ done_flag, unsigned long long done_seq)
{
    // (the collective's output is read past the caches -- another kernel, maybe another agent, wrote it --, the copies
    // go through them to host memory, are acknowledged, and then the flag goes out: no cache-wide fence)
    for (int j = threadIdx.x; j < n; j += 64)
        __hip_atomic_store(&dst_mapped[j], __hip_atomic_load(&src[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_publish(const double* d_src, double* d_dst_mapped, int n, unsigned long long* done_flag,
                          unsigned long long done_seq, hipStream_t stream)
{
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, stream, d_src, d_dst_mapped, n, done_flag, done_seq);
    return hipGetLastError();
}

// Zero-marker case: LLK of an empty sum.
__global__ void fill_zero_kernel(double* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0.0;
}

hipError_t launch_fill_zero(double* d_out, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(fill_zero_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_out, n);
    return hipGetLastError();
}

}  // namespace vb2
