// batch.cpp -- see batch.h.
#include "batch.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>

#include "device_util.h"
#include "estimator.h"
#include "host_clock.h"
#include "lockstep.h"
#include "stream_search.h"
#include "tunables.h"

namespace vb2 {

namespace {
constexpr int kSlot = 8;                     // point slots per sample and step (VB2_BATCH_SLOTS)
// launch shapes of a step: 0 = up to 4 points per sample, 1 = 8 points, 2 = one point, 3 = two
constexpr int kShapeNp[Batch::kShapes] = {4, 8, 1, 2};

// the layout of a slot that holds no sample (its workgroups leave before they read it)
DeviceLayout empty_layout(int num_pc, int num_cu)
{
    DeviceLayout none;
    std::memset(&none, 0, sizeof(none));
    none.num_pc = num_pc;
    none.row_bytes = kRowBytesWide;
    none.num_cu = num_cu;
    return none;
}
}

Batch::~Batch()
{
    if (device >= 0) (void)hipSetDevice(device);
    for (auto& h : half_) h.reset();                            // (they launch on lane_streams_)
    for (hipStream_t& st : lane_streams_)
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
            st = nullptr;
        }
    if (stream_) (void)hipStreamSynchronize(stream_);          // nothing of this batch is in flight any more
    if (d_slab_ && !recycle_device_slab(d_slab_, d_slab_bytes_, device)) (void)hipFree(d_slab_);
    if (h_slab_ && !recycle_pinned_slab(h_slab_, h_slab_bytes_, device)) (void)hipHostFree(h_slab_);
    if (dv_dev_ && !recycle_device_slab(dv_dev_, dv_dev_bytes_, device)) (void)hipFree(dv_dev_);
    if (dv_pin_ && !recycle_pinned_slab(dv_pin_, dv_pin_bytes_, device)) (void)hipHostFree(dv_pin_);
    if (stream_ && own_stream_ && !recycle_stream(stream_, device)) (void)hipStreamDestroy(stream_);
}

int Batch::create(vb2_ctx* const* ctxs, int num_sample, Batch** out)
{
    *out = nullptr;
    if (!ctxs || num_sample < 1) {
        set_error("vb2_batch_create: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::vector<Context*> list;
    for (int s = 0; s < num_sample; ++s) {
        if (!ctxs[s] || !ctxs[s]->impl) {
            set_error("vb2_batch_create: null context");
            return VB2_ERR_INVALID;
        }
        list.push_back(ctxs[s]->impl);
    }
    return create(list, out);
}

// Tunables::cohort_w16 = 0 (a test aid): cohort steps stream the 32-bit run lists
bool cohort_w16_enabled() { return tunables().cohort_w16 != 0; }

// Waves per workgroup of a cohort step (round 4, third part): EIGHT, and twice as many workgroups per sample, instead of
// sixteen.  A search runs its samples as two lanes whose steps take turns; with 1 024-thread workgroups a lane's launch fills
// the CUs' wave slots by itself and the other lane's launch overlaps only with its tail, with 512-thread workgroups two
// workgroups of DIFFERENT launches share a CU and one lane's table builds, barriers and hand-off run under the other's
// streaming: search only 1.356 -> 1.243 ms per sample (737 -> 801 samples/s) on the same box; a synchronous step alone
// takes what it took (75.5 / 105 us).  Tunables::cohort_bw = 16 restores the big workgroups (4 and 8 are the other values).
int cohort_waves()
{
    const int k = tunables().cohort_bw;
    return (k == 4 || k == 8 || k == 16) ? k : 8;
}

void Batch::geometry(int num_cu, int num_sample, int max_mt, int num_pc, int bps_in, int* bps, int* block_waves)
{
    // ~one workgroup per CU in total; the waves of a workgroup: one per tile it owns, 1024 threads at most, and enough
    // of them to stage a step's parameter rows
    const int max_bw = cohort_waves();
    const int wg_total = num_cu * kMaxBlockWaves / max_bw;
    *bps = bps_in > 0 ? bps_in * (kMaxBlockWaves / max_bw) : std::max(1, wg_total / std::max(1, num_sample));
    const int tiles_per_block = (max_mt + *bps - 1) / *bps;
    const int min_bw = std::max(4, (kSlot * (2 * num_pc + 1) + 127) / 128);
    *block_waves = std::max(min_bw, std::min(max_bw, tiles_per_block));
}

int Batch::regroup_bps(int num_cu, int active)
{
    int b = 1;
    while (2 * b * active <= num_cu) b *= 2;
    return b;
}

int search_speculate(int n)
{
    // Speculation (amoeba.h) trades device work for fewer dependent steps.  A small cohort's step is
    // latency-bound and {R, E, C_A, C_R} per iteration pays (2.5 points evaluated per point the
    // search needs).  A big cohort's step is throughput-bound -- its cost grows with the points in
    // it, down to the floor of streaming every sample's pileup from HBM once per step (5.7 TB/s
    // measured: a 1-point step of 32 C3 samples takes 131 us against 236 us with 4 points) -- and
    // {R, C_R} is the better trade: 1.2 steps per iteration at about half the points.  Same
    // decisions, same trajectory either way.  Tunables::cohort_speculate = 1|2|4 forces one.
    constexpr int kPairFrom = 8;
    const int forced = tunables().cohort_speculate;
    return forced > 0 ? forced : n < kPairFrom ? 4 : 2;
}

int search_lanes(int n, bool tuned, int* sizes)
{
    constexpr int kSplitFrom = 16;           // a cohort of this many samples is searched as two half-cohorts taking turns
    const Tunables& tn = tunables();
    bool split = n >= kSplitFrom;
    if (tuned && tn.cohort_split >= 0) split = tn.cohort_split != 0 && n >= 2;
    const int nlane = !split ? 1 : !tuned ? 2 : std::max(2, std::min(std::min(kMaxLanes, tn.cohort_lanes), n));
    for (int l = 0; l < nlane; ++l) sizes[l] = (int)((long)n * (l + 1) / nlane) - (int)((long)n * l / nlane);
    return nlane;
}

int Batch::prepare_for_cohort(Context* c, int group)
{
    if (group < 1 || c->L.num_mt == 0) return VB2_OK;
    int lanes[kMaxLanes];
    const int nlane = search_lanes(group, false, lanes);
    Schedule sc[kShapes];
    int first_bps = 0;
    for (int l = 0; l < nlane; ++l) {
        int bps, bw;
        geometry(c->L.num_cu, lanes[l], c->L.num_mt, c->num_pc, 0, &bps, &bw);
        if (bps == first_bps) continue;
        if (!first_bps) first_bps = bps;
        if (const int rc = c->cohort_schedules(bps, bw, sc)) return rc;
    }
    // the regrouped batches: powers of two above the lane's own (those that take the work queue need no schedule)
    for (int b = 1; b <= c->L.num_cu; b *= 2) {
        int bps, bw;
        geometry(c->L.num_cu, 1, c->L.num_mt, c->num_pc, b, &bps, &bw);      // (bps: b times the workgroups-per-CU factor)
        if (bps <= first_bps) continue;                                       // like with like
        if (eval_takes_the_queue(c->L, bps, bw, 1)) break;
        if (const int rc = c->cohort_schedules(bps, bw, sc)) return rc;
    }
    return VB2_OK;
}

int Batch::create(const std::vector<Context*>& ctxs, Batch** out, int bps_in)
{
    *out = nullptr;
    const int num_sample = (int)ctxs.size();
    if (num_sample < 1) {
        set_error("vb2_batch_create: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<Batch> b(new Batch());
    b->num_sample = num_sample;
    int max_mt = 0, num_cu = 256;
    std::vector<DeviceLayout> layouts(num_sample);
    for (int s = 0; s < num_sample; ++s) {
        Context* c = ctxs[s];
        if (s == 0) {
            b->device = c->device;
            b->num_pc = c->num_pc;
            num_cu = c->L.num_cu;
        } else if (c->device != b->device || c->num_pc != b->num_pc) {
            set_error("vb2_batch_create: contexts must share the device and --NumPC");
            return VB2_ERR_INVALID;
        }
        b->ctx_.push_back(c);
        // cohort steps stream every sample's run lists from HBM once per step: the 16-bit copy halves
        // those bytes (VB2_COHORT_W16=0: the 32-bit lists, A/B)
        if (cohort_w16_enabled() && c->L.num_mt > 0)
            if (const int rc16 = c->ensure_codes16()) return rc16;
        layouts[s] = c->L;
        layouts[s].stamps = nullptr;
        max_mt = std::max(max_mt, c->L.num_mt);
    }
    b->scan_samples();
    VB2_HIP(hipSetDevice(b->device));

    int bps = 1;
    geometry(num_cu, num_sample, max_mt, b->num_pc, bps_in, &bps, &b->block_waves_);
    b->bps_ = bps;
    for (int sh = 0; sh < kShapes; ++sh) {
        size_t need = 0;
        for (int s = 0; s < num_sample; ++s)
            need = std::max(need, eval_shmem_np(layouts[s], kShapeNp[sh], bps, b->block_waves_, 1));
        b->shmem_[sh] = need;
    }
    if (b->shmem_[1] > (size_t)kLdsLimitBytes) {
        set_error("vb2_batch_create: per-workgroup LDS need exceeds 160 KiB");
        return VB2_ERR_INVALID;
    }

    b->layouts_ = std::move(layouts);
    *out = b.release();
    return VB2_OK;
}

int Batch::create_slots(int capacity, int device, int num_pc, int num_cu, Batch** out)
{
    *out = nullptr;
    if (capacity < 1 || capacity > 64 || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("streaming batch: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<Batch> b(new Batch());
    b->num_sample = capacity;
    b->device = device;
    b->num_pc = num_pc;
    b->slots_ = true;
    b->strict_shapes = true;
    b->ctx_.assign(capacity, nullptr);
    b->layouts_.assign(capacity, empty_layout(num_pc, num_cu));
    b->bps_ = std::max(1, num_cu * (kMaxBlockWaves / cohort_waves()) / capacity);
    b->block_waves_ = cohort_waves();         // whatever the samples: a sample's sums must not depend on its neighbours
    *out = b.release();
    return VB2_OK;
}

void Batch::scan_samples()
{
    w16_ = cohort_w16_enabled();
    wide_rows_ = true;
    for (const Context* c : ctx_) {
        if (!c) continue;                                    // (an empty slot)
        if (c->L.num_mt > 0 && !c->L.codes16) w16_ = false;
        if (c->L.row_bytes != kRowBytesWide) wide_rows_ = false;
    }
}

int Batch::set_slot(int i, Context* c)
{
    if (!slots_ || i < 0 || i >= num_sample || in_flight_) {
        set_error("streaming batch: set_slot out of place");
        return VB2_ERR_INVALID;
    }
    DeviceLayout lay = empty_layout(num_pc, layouts_[i].num_cu);
    Schedule sc[kShapes];
    for (int sh = 0; sh < kShapes; ++sh) sc[sh] = Schedule{nullptr, nullptr};
    if (c) {
        if (c->device != device || c->num_pc != num_pc) {
            set_error("streaming batch: contexts must share the device and --NumPC");
            return VB2_ERR_INVALID;
        }
        if (cohort_w16_enabled() && c->L.num_mt > 0)
            if (const int rc16 = c->ensure_codes16()) return rc16;
        lay = c->L;
        lay.stamps = nullptr;
        size_t need[kShapes];
        for (int sh = 0; sh < kShapes; ++sh) need[sh] = std::max(shmem_[sh], eval_shmem_np(lay, kShapeNp[sh], bps_, block_waves_, 1));
        if (need[1] > (size_t)kLdsLimitBytes) {
            set_error("streaming batch: per-workgroup LDS need exceeds 160 KiB");
            return VB2_ERR_INVALID;
        }
        for (int sh = 0; sh < kShapes; ++sh) shmem_[sh] = need[sh];
        if (const int rc = c->cohort_schedules(bps_, block_waves_, sc, false)) return rc;
    }
    ctx_[i] = c;
    layouts_[i] = lay;
    scan_samples();
    if (!ready_ || !c) return VB2_OK;           // (ensure_resources uploads everything at the first step; an empty slot's
                                                //  workgroups leave before they read its layout)
    VB2_HIP(hipSetDevice(device));
    // slot i's layout and schedules through the slot's own stretch of pinned staging: stream-ordered before the next step;
    // the stretch is not written again before that step is over (the slot cannot change hands sooner)
    char* st = h_slot_stage_ + (size_t)i * kSlotStageBytes;
    std::memcpy(st, &lay, sizeof(lay));
    std::memcpy(st + sizeof(DeviceLayout), sc, sizeof(sc));
    VB2_HIP(hipMemcpyAsync(d_layouts_ + i, st, sizeof(DeviceLayout), hipMemcpyHostToDevice, stream_));
    for (int sh = 0; sh < kShapes; ++sh)
        VB2_HIP(hipMemcpyAsync(const_cast<Schedule*>(d_sched_arr_) + (size_t)sh * num_sample + i,
                               st + sizeof(DeviceLayout) + sh * sizeof(Schedule), sizeof(Schedule), hipMemcpyHostToDevice, stream_));
    return VB2_OK;
}

int Batch::ensure_resources()
{
    if (ready_) return VB2_OK;
    VB2_HIP(hipSetDevice(device));
    const int k = num_pc, bps = bps_;
    const size_t S = (size_t)num_sample, stride = 2 * (size_t)k + 1;
    // static schedules (llk_kernels.h) of every sample for the wave shapes of a step: the contexts keep them
    // (Context::cohort_schedules -- prepared by the reader threads in a vb2_cohort_run)
    std::vector<Schedule> arr(kShapes * S, Schedule{nullptr, nullptr});
    bool sched_ok = false;
    for (int s = 0; s < num_sample; ++s) {
        Schedule sc[kShapes];
        if (!ctx_[s]) continue;                              // (an empty slot: create_slots)
        if (const int rc = ctx_[s]->cohort_schedules(bps, block_waves_, sc, !slots_)) return rc;
        for (int sh = 0; sh < kShapes; ++sh) {
            arr[sh * S + s] = sc[sh];
            sched_ok |= sc[sh].off != nullptr;
        }
    }
    // device slab
    size_t dtot = 0;
    auto carve = [&](size_t bytes) {
        const size_t off = (dtot + 255) & ~(size_t)255;
        dtot = off + bytes;
        return off;
    };
    const size_t o_lay = carve(sizeof(DeviceLayout) * S);
    const size_t o_arr = carve(kShapes * S * sizeof(Schedule));
    const size_t o_zero = carve(0);
    const size_t o_part = carve(sizeof(double) * S * (kSlot + 1) * bps);
    const size_t o_tick = carve(sizeof(unsigned int) * S);
    const size_t o_done = carve(sizeof(unsigned int));
    dtot = (dtot + 255) & ~(size_t)255;
    d_slab_ = cached_device_slab(dtot, device, &d_slab_bytes_);
    if (!d_slab_) {
        VB2_HIP(hipMalloc(&d_slab_, dtot));
        d_slab_bytes_ = dtot;
    }
    char* dbase = static_cast<char*>(d_slab_);
    if (!stream_) {
        stream_ = cached_stream(device);
        if (!stream_) VB2_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    }
    // host image of the read-only part, uploaded on the batch's stream (the launches follow on it)
    std::vector<char> image(o_zero, 0);
    std::memcpy(image.data() + o_lay, layouts_.data(), sizeof(DeviceLayout) * S);
    std::memcpy(image.data() + o_arr, arr.data(), kShapes * S * sizeof(Schedule));
    VB2_HIP(hipMemcpyAsync(dbase, image.data(), image.size(), hipMemcpyHostToDevice, stream_));
    VB2_HIP(hipMemsetAsync(dbase + o_zero, 0, dtot - o_zero, stream_));
    VB2_HIP(hipStreamSynchronize(stream_));                       // (image is a pageable temporary)
    d_layouts_ = reinterpret_cast<DeviceLayout*>(dbase + o_lay);
    d_sched_arr_ = reinterpret_cast<const Schedule*>(dbase + o_arr);
    for (int sh = 0; sh < kShapes; ++sh)
        d_scheds_[sh] = (sched_ok || slots_) ? d_sched_arr_ + sh * S : nullptr;
    d_partials_ = reinterpret_cast<double*>(dbase + o_part);
    d_tickets_ = reinterpret_cast<unsigned int*>(dbase + o_tick);
    d_batch_done_ = reinterpret_cast<unsigned int*>(dbase + o_done);
    // pinned, device-mapped slab
    size_t htot = 0;
    auto hcarve = [&](size_t bytes) {
        const size_t off = (htot + 127) & ~(size_t)127;
        htot = off + bytes;
        return off;
    };
    const size_t p_pts = hcarve(sizeof(double) * S * kSlot * stride);
    const size_t p_out = hcarve(sizeof(double) * S * kSlot);
    const size_t p_nv = hcarve(sizeof(int) * S);
    const size_t p_done = hcarve(sizeof(unsigned long long) * 8);
    const size_t p_stage = hcarve(slots_ ? S * kSlotStageBytes : 0);
    h_slab_ = cached_pinned_slab(htot, device, &h_slab_bytes_);
    if (!h_slab_) {
        VB2_HIP(hipHostMalloc(&h_slab_, htot, hipHostMallocMapped));
        h_slab_bytes_ = htot;
    }
    std::memset(h_slab_, 0, htot);
    char* hbase = static_cast<char*>(h_slab_);
    char* hdev = nullptr;
    VB2_HIP(hipHostGetDevicePointer((void**)&hdev, h_slab_, 0));
    h_points_ = reinterpret_cast<double*>(hbase + p_pts);
    d_points_ = reinterpret_cast<double*>(hdev + p_pts);
    h_out_ = reinterpret_cast<double*>(hbase + p_out);
    d_out_ = reinterpret_cast<double*>(hdev + p_out);
    h_nv_ = reinterpret_cast<int*>(hbase + p_nv);
    d_nv_ = reinterpret_cast<int*>(hdev + p_nv);
    h_done_ = reinterpret_cast<unsigned long long*>(hbase + p_done);
    d_done_ = reinterpret_cast<unsigned long long*>(hdev + p_done);
    h_slot_stage_ = hbase + p_stage;
    seq_ = 0;
    ready_ = true;
    return VB2_OK;
}

int Batch::eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                double* llk_out)
{
    if (const int rc = eval_begin(num_point, pc1, pc2, alpha, llk_out)) return rc;
    return eval_end();
}

// The launches of a step, in order.  A launch runs ONE kind of kernel in ONE wave shape: three rules, one inside the other.
// 1. Samples of both layouts (a probability-domain context next to one that could not take that layout: deep markers,
//    quality 0): the probability-domain samples first, then the others.  A sample's values do not depend on its launch.
// 2. strict_shapes: a step's wave shape follows from the LARGEST request in it, and under the static deal the shape decides
//    which tiles a wave multiplies together -- so a sample's sums would move in their last bits with what its neighbours
//    happen to ask for (a new sample's initial simplex, a shrink).  Strict: the requests of 1-2, of 3-4 and of 5-8 points
//    leave as separate launches (the one- and two-point shapes deal and multiply alike: bit-identical, tested), so a
//    sample's values depend on its own requests only.  Mixed steps are rare (a sample starts or shrinks in 1-2 % of them):
//    the most populous class goes last, which is the launch left in flight.  A 5-8 point request of a sample with narrow
//    table rows is a class of its own, or one such neighbour would change everybody's wave shape.
// 3. A sample with a very wide dictionary (more than kMaxWideCodes codes) has narrow table rows: 4 points per launch at
//    most, so a launch of 5-8 points with such a sample in it becomes two of 4, both waited for.  (Where rule 2 applies and
//    left the launch's group whole, it takes each of the two apart: their requests are of 4 and of 1-4 points.)
void Batch::plan_step(const int32_t* num_point, std::vector<SubStep>* plan) const
{
    typedef std::vector<int32_t> Counts;
    const size_t S = (size_t)num_sample;
    auto narrow = [&](size_t s) { return ctx_[s] && ctx_[s]->L.row_bytes != kRowBytesWide; };
    auto cls_of = [&](int n, size_t s) { return n <= 0 ? -1 : n <= 2 ? 0 : n <= 4 ? 1 : narrow(s) ? 3 : 2; };
    auto several = [](const int* pop) { return (pop[0] > 0) + (pop[1] > 0) + (pop[2] > 0) + (pop[3] > 0) > 1; };
    // nearly every step is one launch of num_point as it is: *plan stays empty and nothing is allocated
    bool any_pd = false, any_log = false, narrow_in = false;
    int all_pop[4] = {0, 0, 0, 0}, max_n = 0;
    for (size_t s = 0; s < S; ++s) {
        if (num_point[s] <= 0) continue;
        max_n = std::max(max_n, (int)num_point[s]);
        narrow_in |= narrow(s);
        ++all_pop[cls_of(num_point[s], s)];
        if (ctx_[s] && ctx_[s]->L.num_mt > 0) (ctx_[s]->L.pd ? any_pd : any_log) = true;
    }
    if (!(any_pd && any_log) && !(strict_shapes && several(all_pop)) && !(max_n > 4 && !wide_rows_ && narrow_in)) return;
    // rule 2: appends np's classes to *out, the most populous last, and says whether there was more than one
    auto by_class = [&](Counts np, std::vector<Counts>* out) {
        int pop[4] = {0, 0, 0, 0}, keep = 0;
        for (size_t s = 0; s < S; ++s)
            if (np[s] > 0) ++pop[cls_of(np[s], s)];
        if (!strict_shapes || !several(pop)) {
            out->push_back(std::move(np));
            return false;
        }
        for (int c = 1; c < 4; ++c)
            if (pop[c] > pop[keep]) keep = c;
        for (int i = 0; i < 4; ++i) {
            const int c = i < 3 ? (i < keep ? i : i + 1) : keep;
            if (pop[c] == 0) continue;
            Counts part(S);
            for (size_t s = 0; s < S; ++s) part[s] = cls_of(np[s], s) == c ? np[s] : 0;
            out->push_back(std::move(part));
        }
        return true;
    };
    std::vector<Counts> groups;                    // rule 1
    groups.emplace_back(num_point, num_point + S);
    if (any_pd && any_log) {
        groups.push_back(groups[0]);
        for (size_t s = 0; s < S; ++s) groups[ctx_[s] && ctx_[s]->L.pd ? 1 : 0][s] = 0;
    }
    for (Counts& g : groups) {
        std::vector<Counts> classes;
        const bool apart = by_class(std::move(g), &classes);
        for (Counts& c : classes) {
            bool halves = false;                   // rule 3 (of the samples that take part in THIS launch)
            if (!wide_rows_ && *std::max_element(c.begin(), c.end()) > 4)
                for (size_t s = 0; s < S; ++s) halves |= c[s] > 0 && narrow(s);
            if (!halves) {
                plan->push_back(SubStep{std::move(c), 0, false});
                continue;
            }
            for (int first = 0; first < kSlot; first += 4) {
                Counts h(S);
                for (size_t s = 0; s < S; ++s) h[s] = std::max(0, std::min(4, (int)c[s] - first));
                std::vector<Counts> parts;
                if (apart) parts.push_back(std::move(h));
                else by_class(std::move(h), &parts);
                for (Counts& p : parts) plan->push_back(SubStep{std::move(p), first, true});
            }
        }
    }
}

int Batch::eval_begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                      double* llk_out)
{
    if (in_flight_) {
        set_error("vb2_batch_eval: a step is already in flight");
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipSetDevice(device));
    int max_n = 0;
    for (int s = 0; s < num_sample; ++s) {
        if (num_point[s] < 0 || num_point[s] > kSlot) {
            set_error("vb2_batch_eval: num_point out of range");
            return VB2_ERR_INVALID;
        }
        max_n = std::max(max_n, (int)num_point[s]);
    }
    if (max_n == 0) return VB2_OK;
    if (const int rc = ensure_resources()) return rc;
    std::vector<SubStep> plan;
    plan_step(num_point, &plan);
    if (plan.empty()) return launch_step(num_point, 0, pc1, pc2, alpha, llk_out);
    for (size_t i = 0; i < plan.size(); ++i) {
        if (const int rc = launch_step(plan[i].np.data(), plan[i].first, pc1, pc2, alpha, llk_out)) return rc;
        if (plan[i].wait || i + 1 < plan.size())
            if (const int rc = eval_end()) return rc;
    }
    return VB2_OK;
}

void Batch::prefill_nan()
{
    // (results come back as relaxed stores behind a relaxed flag: NaN first, so that a store still on its way when the
    // flag is seen is noticed -- Context::eval_host, settle_results)
    for (int s = 0; s < num_sample; ++s)
        for (int j = 0; j < h_nv_[s]; ++j) h_out_[(size_t)s * flight_np_ + j] = std::numeric_limits<double>::quiet_NaN();
}

int Batch::launch_step(const int32_t* np, int first, const double* pc1, const double* pc2, const double* alpha, double* llk_out)
{
    const int k = num_pc, stride = 2 * k + 1;
    const int max_n = *std::max_element(np, np + num_sample);
    unsigned int active = 0;
    // one or two points per sample (a search that speculates little or not at all): the wave takes
    // four micro-tiles, and the step costs a quarter / half of a 4-point step whose other slots
    // would replicate the last point
    const bool small = max_n <= 2;
    const int NP = max_n > 4 ? 8 : small ? max_n : 4, shape = max_n > 4 ? 1 : small ? (max_n == 1 ? 2 : 3) : 0;
    flight_nan_.resize((size_t)num_sample);
    for (int s = 0; s < num_sample; ++s) {
        int n = np[s];
        const size_t at = (size_t)s * kSlot + first;
        // a sample without active markers has LLK 0 for every point: answer it here
        if (n > 0 && (!ctx_[s] || ctx_[s]->L.num_mt == 0)) {
            for (int j = 0; j < n; ++j) llk_out[at + j] = 0.0;
            n = 0;
        }
        h_nv_[s] = n;
        if (n > 0) ++active;
        flight_nan_[s] = 0;
        const bool kaf = n > 0 && ctx_[s]->L.known_af != nullptr;
        for (int j = 0; j < n; ++j) {
            double* row = h_points_ + ((size_t)s * NP + j) * stride;
            // NaN parameters (context.h: params_hold_nan, with this sample's own known-AF flag): the answer is 0, given in
            // eval_end; the kernel evaluates a finite stand-in in the point's place, so that the step keeps its shape and a
            // caller's NaN is never taken for the hand-off's "a workgroup never reported" marker
            if (params_hold_nan(pc1 + (at + j) * k, pc2 + (at + j) * k, alpha[at + j], k, kaf)) {
                flight_nan_[s] |= (unsigned char)(1u << j);
                std::memset(row, 0, sizeof(double) * 2 * k);
                row[2 * k] = 0.5;
                continue;
            }
            std::memcpy(row, pc1 + (at + j) * k, sizeof(double) * k);
            std::memcpy(row + k, pc2 + (at + j) * k, sizeof(double) * k);
            row[2 * k] = alpha[at + j];
        }
    }
    if (active == 0) return VB2_OK;
    MultiLaunch& ml = ml_;
    ml = MultiLaunch{};
    ml.d_layouts = d_layouts_;
    ml.d_scheds = d_scheds_[shape];
    ml.d_points = d_points_;
    ml.d_num_valid = d_nv_;
    ml.d_partials = d_partials_;
    ml.d_out = d_out_;
    ml.d_tickets = d_tickets_;
    ml.d_batch_done = d_batch_done_;
    ml.done_flag = d_done_;
    ml.done_seq = ++seq_;
    ml.batch_active = active;
    ml.num_sample = num_sample;
    ml.bps = bps_;
    ml.block_waves = block_waves_;
    ml.np = NP;
    ml.shmem = shmem_[shape];
    ml.force_ticket = false;
    ml.w16 = w16_;
    for (int s2 = 0; s2 < num_sample; ++s2)
        if (h_nv_[s2] > 0 && ctx_[s2] && ctx_[s2]->L.pd) ml.pd = true;      // (the launch's samples are of one layout: plan_step)
    // (probability domain: the short copy is the 8-bit step lists -- they pay where a step is bound by what it streams: 32 C3
    // samples x 1 point 62.4 -> 58.0 us, x 2 points 77.4 -> 76.0, x 4 points 124.6 -> 126.3: the one- and two-point shapes only)
    if (ml.pd && NP > 2) ml.w16 = false;
    {   // (the pipelined item loop is compiled for the static deal: every sample of the cohort must run it)
        bool st_all = true;
        for (int s2 = 0; s2 < num_sample && st_all; ++s2)
            st_all = !ctx_[s2] || ctx_[s2]->L.num_mt == 0 || !eval_takes_the_queue(ctx_[s2]->L, bps_, block_waves_, 1);
        ml.all_static = st_all;
    }
    {   // (the cohort kernels compiled for --NumPC 2 / 4 without a known-AF column)
        bool plain = num_pc == 2 || num_pc == 4;
        for (int s2 = 0; s2 < num_sample && plain; ++s2) plain = !ctx_[s2] || ctx_[s2]->L.known_af == nullptr;
        ml.ksel = plain ? num_pc : 0;
    }
    // counts and rows as kernel arguments when they fit (saves every workgroup two trips to mapped host memory)
    ml.inl.count = 0;
    if (num_sample <= kMultiInlineSamples && (size_t)num_sample * NP * stride <= (size_t)kMultiInlineDoubles) {
        ml.inl.count = num_sample * NP * stride;
        for (int s2 = 0; s2 < num_sample; ++s2) ml.inl.nv[s2] = (unsigned char)h_nv_[s2];
        std::memcpy(ml.inl.v, h_points_, sizeof(double) * (size_t)ml.inl.count);
    }
    flight_np_ = NP;
    flight_first_ = first;
    flight_out_ = llk_out;
    prefill_nan();
    VB2_HIP(launch_llk_eval_multi(ml, stream_));
    ++num_launch;
    in_flight_ = true;
    return VB2_OK;
}

int Batch::eval_end()
{
    if (!in_flight_) return VB2_OK;                      // (nothing was launched: answered in eval_begin)
    in_flight_ = false;
    VB2_HIP(hipSetDevice(device));
    MultiLaunch& ml = ml_;
    const int NP = flight_np_;
    // (a NaN is the tagged hand-off's "a workgroup never reported" marker: redo the step once with
    // the arrival-ticket hand-off, see Context::eval_host -- NaN must not reach the optimisers)
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (attempt > 0) {
            ml.force_ticket = true;
            ml.done_seq = ++seq_;
            prefill_nan();
            VB2_HIP(launch_llk_eval_multi(ml, stream_));
            ++num_launch;
        }
        bool seen = false;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0;; ++spins) {
            if (__atomic_load_n(h_done_, __ATOMIC_ACQUIRE) == ml.done_seq) { seen = true; break; }
            if ((spins & 0x3ff) == 0x3ff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) break;
            __builtin_ia32_pause();
        }
        if (!seen) VB2_HIP(hipStreamSynchronize(stream_));
        bool any_nan = true;
        const auto ts = std::chrono::steady_clock::now();
        while (any_nan) {                         // (a store still on its way: a few microseconds; then the kernels' own marker)
            any_nan = false;
            for (int s = 0; s < num_sample && !any_nan; ++s)
                for (int j = 0; j < h_nv_[s]; ++j)
                    any_nan |= std::isnan(reinterpret_cast<volatile double*>(h_out_)[(size_t)s * NP + j]);
            if (std::chrono::steady_clock::now() - ts > std::chrono::microseconds(50)) break;
        }
        if (!any_nan) break;
    }
    for (int s = 0; s < num_sample; ++s)
        for (int j = 0; j < h_nv_[s]; ++j)
            flight_out_[(size_t)s * kSlot + flight_first_ + j] = (flight_nan_[s] >> j & 1) ? 0.0 : h_out_[(size_t)s * NP + j];
    return VB2_OK;
}

// ---------------------------------------------------------------------------
// lock-step search: every sample runs the ordinary Estimator (OptimizeLLK with its six models,
// the reference-exact simplex) as a fiber of the calling thread (lockstep.h); the parked
// requests of a step leave as ONE launch of the multi-sample kernel.
//
// A cohort of 16 samples or more (search_lanes) is searched as TWO half-cohorts taking turns: while one
// half's step is on the device, the other half's fibers run on the host (64 fiber switches and
// simplex updates are ~60 us, a quarter of the step they would otherwise be added to), and the
// next launch is already queued behind the running one, so the device never waits for the host.
//
// SearchLane is one of those halves: a gang of fibers, the batch their requests are launched on, the staging in between.
// take_turns is the loop; what a search does around a step (regrouping; refilling and retiring slots) it is given as hooks.
// ---------------------------------------------------------------------------
namespace {

struct SearchLane;
struct LaneTeam {                           // the lanes of one search and its first device-level error
    SearchLane* lanes = nullptr;
    int nlane = 0, error = 0;
    bool dbg = tunables().debug_lockstep != 0;       // what the lanes then count and time for the searches' diagnostic lines
    long steps = 0, active = 0, points = 0, by_eighths[9] = {0}, steps_by_slots[65] = {0};
    double s_launch = 0, s_wait = 0, s_resume = 0, s_flight_by_slots[65] = {0};
};

struct SearchLane {
    LaneTeam* team = nullptr;
    std::unique_ptr<FiberGang> gang;
    Batch* batch = nullptr;                 // where the next step is launched (not owned)
    std::vector<int> slot_fiber;            // slot j of `batch` carries fiber slot_fiber[j]: the identity until a lane regroups
    std::vector<int32_t> npts;
    std::vector<double> pc1, pc2, alpha, llk;
    bool flying = false;
    double t_launch = 0;

    void init(LaneTeam* t, Batch* b, int num_fiber, int max_points_per_request)
    {
        team = t;
        batch = b;
        gang.reset(new FiberGang(num_fiber, max_points_per_request));
        slot_fiber.resize(num_fiber);
        for (int i = 0; i < num_fiber; ++i) slot_fiber[i] = i;
        const size_t n = (size_t)num_fiber, k = (size_t)b->num_pc;
        npts.assign(n, 0);
        pc1.resize(n * kSlot * k); pc2.resize(n * kSlot * k); alpha.resize(n * kSlot); llk.resize(n * kSlot);
    }
    bool busy() const { return flying || gang->pending(); }
    void fail(int rc)
    {
        if (!team->error) team->error = rc;
        for (int l = 0; l < team->nlane; ++l) team->lanes[l].gang->fail(rc);
    }
    // the parked requests of the lane -> one step of its batch
    void launch()
    {
        if (team->error || !gang->pending()) return;
        const std::vector<FiberGang::Request>& req = gang->requests();
        const int nslot = (int)slot_fiber.size(), k = batch->num_pc;
        int act = 0, pts = 0;
        for (int i = 0; i < nslot; ++i) {
            const FiberGang::Request& r = req[slot_fiber[i]];
            npts[i] = gang->idle(slot_fiber[i]) ? 0 : r.n;
            if (npts[i] <= 0) continue;
            ++act; pts += r.n;
            std::memcpy(&pc1[(size_t)i * kSlot * k], r.p1, sizeof(double) * r.n * k);
            std::memcpy(&pc2[(size_t)i * kSlot * k], r.p2, sizeof(double) * r.n * k);
            std::memcpy(&alpha[(size_t)i * kSlot], r.a, sizeof(double) * r.n);
        }
        if (team->dbg) {
            ++team->steps; team->active += act; team->points += pts;
            team->by_eighths[std::min(8, (8 * act + nslot - 1) / nslot)]++;
        }
        const double tl = team->dbg ? now_s() : 0.0;
        if (const int rc = batch->eval_begin(npts.data(), pc1.data(), pc2.data(), alpha.data(), llk.data())) {
            fail(rc);
            return;
        }
        if (team->dbg) team->s_launch += (t_launch = now_s()) - tl;
        flying = true;
    }
    // wait for the lane's step, hand the values out, run its fibers up to their next requests
    void land()
    {
        if (flying) {
            flying = false;
            const double tw = team->dbg ? now_s() : 0.0;
            if (const int rc = batch->eval_end()) fail(rc);
            if (team->dbg) {
                const int ns = std::min(64, (int)slot_fiber.size());
                const double now = now_s();
                team->s_wait += now - tw;
                team->s_flight_by_slots[ns] += now - t_launch;
                ++team->steps_by_slots[ns];
            }
            if (!team->error) {
                std::vector<FiberGang::Request>& req = gang->requests();
                for (size_t i = 0; i < slot_fiber.size(); ++i)
                    if (npts[i] > 0) std::memcpy(req[slot_fiber[i]].out, &llk[i * kSlot], sizeof(double) * npts[i]);
            }
        }
        const double tr = team->dbg ? now_s() : 0.0;
        if (gang->pending()) gang->resume_parked();           // (after an error: the fibers unwind)
        if (team->dbg) team->s_resume += now_s() - tr;
    }
};

// The lanes take turns until none has a step in flight or a request parked: a lane's step is queued behind the other's step
// in flight, then that one is landed and launched again.  The hooks run ahead of every launch and behind every landing.
template <class Before, class After>
void take_turns(LaneTeam& team, Before before_launch, After after_land)
{
    for (bool busy = true; busy;) {
        busy = false;
        for (int l = 0; l < team.nlane; ++l) {
            SearchLane& next = team.lanes[(l + 1) % team.nlane];
            if (team.nlane > 1 && !next.flying) {              // queued behind the step in flight
                before_launch(next);
                next.launch();
            }
            SearchLane& cur = team.lanes[l];
            if (cur.busy()) {
                cur.land();
                after_land(cur);
            }
            before_launch(cur);
            cur.launch();
            busy |= cur.busy();
        }
    }
}

}  // namespace

int Batch::optimize(const vb2_model* models, int num_model, vb2_estimate* out)
{
    if (!models || !out || (num_model != 1 && num_model != num_sample)) {
        set_error("vb2_batch_optimize_llk: pass 1 model or one per sample");
        return VB2_ERR_INVALID;
    }
    const Tunables& tn = tunables();
    const int S = num_sample, k = num_pc, speculate = search_speculate(S);
    SearchLane lanes[kMaxLanes];
    LaneTeam team{lanes};
    int base[kMaxLanes] = {0}, count[kMaxLanes];               // lane l searches samples [base[l], base[l] + count[l])
    std::unique_ptr<Batch> regrouped[kMaxLanes];
    const int nlane = team.nlane = search_lanes(S, true, count);
    for (int l = 1; l < nlane; ++l) base[l] = base[l - 1] + count[l - 1];
    if (nlane > 1) {
        if (tn.cohort_own_queues && !lane_streams_[0]) {
            VB2_HIP(hipSetDevice(device));
            for (int h = 0; h < nlane; ++h)
                if (hipStreamCreateWithFlags(&lane_streams_[h], hipStreamNonBlocking) != hipSuccess) {
                    (void)hipGetLastError();
                    lane_streams_[h] = nullptr;
                }
        }
        for (int h = 0; h < nlane; ++h) {
            if (!half_[h] || half_[h]->num_sample != count[h]) {
                std::vector<Context*> part(ctx_.begin() + base[h], ctx_.begin() + base[h] + count[h]);
                Batch* hb = nullptr;
                if (const int rc = Batch::create(part, &hb)) return rc;
                if (lane_streams_[h]) hb->borrow_stream(lane_streams_[h]);
                half_[h].reset(hb);
            }
        }
    }
    for (int l = 0; l < nlane; ++l) lanes[l].init(&team, nlane > 1 ? half_[l].get() : this, count[l], kSlot);
    // Samples finish at different iterations (C3-shaped cohort of 32: the shortest search is over after ~60 % of the
    // longest's steps), and a step gives every sample of its batch 256 / num_sample workgroups whether it still takes part
    // or not: in round 3 a third of all steps served one or two samples on an eighth of the device.  So when half of a
    // lane's samples have finished, the rest are regrouped into a batch of their own -- twice the workgroups per sample; the
    // sums move in their last bits, as they do between group sizes (the static deal multiplies a wave's items in the wave);
    // what regroups when follows from the samples' own trajectories, so a run stays reproducible -- and again at a quarter,
    // an eighth ...
    // Tunables::cohort_regroup = 0: the fixed batch to the end (A/B).
    const bool regroup = tn.cohort_regroup != 0;
    double regroup_s = 0;
    num_regroup = 0;
    auto regroup_lane = [&](SearchLane& L) {
        if (!regroup || team.error) return;
        const int l = (int)(&L - lanes);
        const std::vector<FiberGang::Request>& req = L.gang->requests();
        int act = 0;
        for (int j : L.slot_fiber) act += req[j].n > 0;
        if (act < 1 || 2 * act > (int)L.slot_fiber.size()) return;
        std::vector<int> keep;
        std::vector<Context*> part;
        for (int j : L.slot_fiber)
            if (req[j].n > 0) {
                keep.push_back(j);
                part.push_back(ctx_[base[l] + j]);
            }
        Batch* nb = nullptr;
        const double tr0 = now_s();
        int rc = Batch::create(part, &nb, regroup_bps(ctx_[0]->L.num_cu, (int)part.size()));
        if (!rc && nlane > 1 && lane_streams_[l]) nb->borrow_stream(lane_streams_[l]);
        if (!rc) rc = nb->ensure_resources();
        if (rc) {
            delete nb;
            L.fail(rc);
            return;
        }
        regroup_s += now_s() - tr0;
        regrouped[l].reset(nb);                // (the batch it replaces has no step in flight: its slabs go back to the caches)
        L.batch = nb;
        L.slot_fiber.swap(keep);
        ++num_regroup;
    };
    std::vector<int> rcs(S, 0);
    for (int l = 0; l < nlane; ++l) {
        SearchLane& L = lanes[l];
        auto body = [&, l](int i) {
            const int s = base[l] + i;
            FiberGang::Search cfg;
            cfg.model = &models[num_model == 1 ? 0 : s];
            cfg.data_has_known_af = ctx_[s]->L.known_af != nullptr;
            cfg.speculate = speculate;
            rcs[s] = L.gang->search(i, cfg, "vb2_batch_optimize_llk", &out[s]);
        };
        if (L.gang->start(k, body) < 0) {
            // the lanes started so far have fibers parked in the middle of OptimizeLLK: tell them, and
            // run them until they have unwound (their Estimators and vectors live on the fiber stacks,
            // which the gang unmaps) before giving up
            for (int m = 0; m < l; ++m) {
                lanes[m].gang->fail(VB2_ERR_INVALID);
                while (lanes[m].gang->pending()) lanes[m].gang->resume_parked();
            }
            set_error("vb2_batch_optimize_llk: could not start the search fibers (mmap / getcontext failed)");
            return VB2_ERR_INVALID;
        }
    }
    const double t_loop0 = now_s();
    regroup_lane(lanes[0]);
    lanes[0].launch();
    take_turns(team, regroup_lane, [](SearchLane&) {});
    if (team.dbg) {
        std::fprintf(stderr, "lock-step loop %.2f ms, of which regrouping %.2f ms\n", 1e3 * (now_s() - t_loop0), 1e3 * regroup_s);
        for (int n = 1; n <= 64; ++n)
            if (team.steps_by_slots[n])
                std::fprintf(stderr, "  batches of %d: %ld steps, %.1f us from launch to landing each\n", n, team.steps_by_slots[n],
                             1e6 * team.s_flight_by_slots[n] / team.steps_by_slots[n]);
        const long* e = team.by_eighths;
        std::fprintf(stderr, "lock-step search of %d samples in %d lane(s): %ld steps, %.1f active samples and %.1f points per step "
                             "(a lane holds %d, %ld regroupings); steps by eighths of the batch active: %ld %ld %ld %ld %ld %ld %ld %ld\n",
                     S, nlane, team.steps, (double)team.active / std::max(1L, team.steps), (double)team.points / std::max(1L, team.steps),
                     count[0], (long)num_regroup, e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8]);
    }
    if (team.error) return team.error;
    for (int s = 0; s < S; ++s)
        if (rcs[s]) return rcs[s];
    return VB2_OK;
}

// ---------------------------------------------------------------------------
// stream_search.h: slots that change hands
// ---------------------------------------------------------------------------
int prepare_for_stream(Context* c, int capacity)
{
    if (!c || capacity < 1 || c->L.num_mt == 0) return VB2_OK;
    int n[kMaxLanes];
    const int nlane = search_lanes(capacity, false, n);
    Schedule sc[Batch::kShapes];
    for (int l = 0; l < nlane; ++l) {
        if (l == 1 && n[1] == n[0]) continue;
        if (const int rc = c->cohort_schedules(std::max(1, c->L.num_cu * (kMaxBlockWaves / cohort_waves()) / n[l]), cohort_waves(), sc, false)) return rc;
    }
    return VB2_OK;
}

int stream_search(int device, int num_pc, int num_cu, int capacity, StreamSource& src, const hipStream_t* lane_streams)
{
    capacity = std::max(1, std::min(capacity, 128));
    const int k = num_pc, speculate = search_speculate(capacity);
    struct Slots {                          // of a lane: [slot] the sample in it (or -1) and what its search leaves
        std::unique_ptr<Batch> batch;
        std::vector<int> id, rc;
        std::vector<vb2_estimate> est;
        std::vector<double> t0;
    } slots[kMaxLanes];
    SearchLane lanes[kMaxLanes];
    LaneTeam team{lanes};
    int cnt[kMaxLanes];
    const int nlane = team.nlane = search_lanes(capacity, false, cnt);
    for (int l = 0; l < nlane; ++l) {
        Batch* b = nullptr;
        if (const int rc = Batch::create_slots(cnt[l], device, k, num_cu, &b)) return rc;
        slots[l].batch.reset(b);
        if (lane_streams && lane_streams[l]) b->borrow_stream(lane_streams[l]);
        // A streamed sample starts whenever a slot falls free, alone.  The ten vertices of its fresh simplex as ONE request would be
        // a class of their own in that step (strict shapes: plan_step leaves the most populous class in flight and waits for the
        // others): an eight-point launch on that sample's sixteenth of the device, ~120 us during which the pipeline thread serves
        // neither lane.  In pieces of two they ride along with the other slots' steps.
        lanes[l].init(&team, b, cnt[l], std::max(1, std::min(kSlot, tunables().cohort_stream_points)));
        slots[l].id.assign(cnt[l], -1);
        slots[l].rc.assign(cnt[l], 0);
        slots[l].est.resize(cnt[l]);
        slots[l].t0.assign(cnt[l], 0.0);
    }
    for (int l = 0; l < nlane; ++l) {
        SearchLane& L = lanes[l];
        Slots& sl = slots[l];
        L.gang->open(k, [&L, &sl, &src, speculate](int i) {
            FiberGang::Search cfg;
            cfg.model = &src.model(sl.id[i]);
            cfg.data_has_known_af = sl.batch->slot(i)->L.known_af != nullptr;
            cfg.speculate = speculate;
            sl.rc[i] = L.gang->search(i, cfg, "stream_search", &sl.est[i]);
        });
    }
    bool ended = false;
    const bool dbg = team.dbg;
    long dbg_samples = 0;
    double dbg_blocked = 0, dbg_refill = 0, dbg_retire = 0;
    const double dbg_t0 = now_s();
    auto retire = [&](SearchLane& L, int i) {
        Slots& sl = slots[&L - lanes];
        const int rc = team.error ? team.error : sl.rc[i];
        src.done(sl.id[i], rc, sl.est[i], now_s() - sl.t0[i]);
        sl.id[i] = -1;
        (void)sl.batch->set_slot(i, nullptr);
    };
    // free slots of a lane <- samples that are ready; block: wait for the first one (nothing is running anywhere)
    auto refill = [&](SearchLane& L, bool block) {
        if (team.error) return;
        Slots& sl = slots[&L - lanes];
        for (int i = 0; i < L.gang->size() && !ended; ++i) {
            if (sl.id[i] >= 0) continue;
            Context* c = nullptr;
            const double tb = dbg ? now_s() : 0.0;
            const int id = src.next(block, &c);
            if (dbg && block) dbg_blocked += now_s() - tb;
            block = false;
            if (id == StreamSource::kEnd) ended = true;
            if (id < 0) break;
            sl.id[i] = id;
            sl.rc[i] = 0;
            std::memset(&sl.est[i], 0, sizeof(vb2_estimate));
            sl.t0[i] = now_s();
            ++dbg_samples;
            // (Tunables::cohort_fail_sample: a test's way to send one sample down this error path)
            const int rc_slot = id == tunables().cohort_fail_sample ? (set_error("streaming batch: sample refused (test hook)"), VB2_ERR_INVALID)
                                                                   : sl.batch->set_slot(i, c);
            if (const int rc = rc_slot) {                       // this sample cannot be searched here: the others can
                sl.rc[i] = rc;
                retire(L, i);
                --i;
                continue;
            }
            if (L.gang->spawn(i) < 0) {
                set_error("stream_search: could not start a search fiber (mmap / getcontext failed)");
                sl.rc[i] = VB2_ERR_INVALID;
                retire(L, i);
                continue;
            }
            if (L.gang->idle(i)) {                              // over before its first request
                retire(L, i);
                --i;
            }
            if (dbg) dbg_refill += now_s() - sl.t0[i < 0 ? 0 : i];
        }
    };
    // the slots whose searches are over are reported and fall free
    auto retire_idle = [&](SearchLane& L) {
        const Slots& sl = slots[&L - lanes];
        const double tr = dbg ? now_s() : 0.0;
        for (int i = 0; i < L.gang->size(); ++i)
            if (sl.id[i] >= 0 && L.gang->idle(i)) retire(L, i);
        if (dbg) dbg_retire += now_s() - tr;
    };
    for (;;) {
        take_turns(team, [&](SearchLane& L) { refill(L, false); }, retire_idle);
        if (team.error || ended) break;
        refill(lanes[0], true);                                 // nothing in flight, nothing ready: wait for a sample
        lanes[0].launch();
        if (!lanes[0].busy() && ended) break;
    }
    if (dbg) {
        const long per = std::max(1L, team.steps);
        std::fprintf(stderr, "stream search: %ld samples through %d slots in %.1f ms: %ld steps, %.1f active samples and %.1f points "
                             "per step (a lane holds %d); waited %.1f ms with nothing to do, %.1f ms taking samples in; the pipeline thread per step: "
                             "%.1f us waiting for a step to land, %.1f us in the samples' optimisers, %.1f us retiring, %.1f us launching\n",
                     dbg_samples, capacity, 1e3 * (now_s() - dbg_t0), team.steps, (double)team.active / per, (double)team.points / per, cnt[0],
                     1e3 * dbg_blocked, 1e3 * dbg_refill, 1e6 * team.s_wait / per, 1e6 * team.s_resume / per, 1e6 * dbg_retire / per,
                     1e6 * team.s_launch / per);
    }
    return team.error;
}

}  // namespace vb2
