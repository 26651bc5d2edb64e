// paired.cpp -- host side of the likelihood given priors on both components (marker_sum_kernels.hip: PairTerm; DESIGN.md
// section 16): the set of pair hypotheses on a context, its evaluation in two halves, and the refits in lock-step with the
// intended sample's PCs held.
#include "paired.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "context.h"
#include "device_util.h"
#include "lockstep.h"
#include "marker_sum_kernels.h"
#include "source.h"

namespace vb2 {

namespace {
const char* const kNoMemWho = "vb2_paired_create";   // (whichever way the set is made)
}

int Paired::make(Context* ctx, int num_hyp, const char* who, Paired** out)
{
    *out = nullptr;
    if (!ctx || num_hyp < 1 || num_hyp > 65535) {
        set_error(std::string(who) + ": invalid argument (1..65535 hypotheses)");
        return VB2_ERR_INVALID;
    }
    if (ctx->resident_active) {
        set_error(std::string(who) + ": not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<Paired> c(new Paired());
    c->ctx = ctx;
    c->num_hyp = num_hyp;
    c->given.assign((size_t)num_hyp, 0);
    const DeviceLayout& L = ctx->L;
    VB2_HIP(hipSetDevice(ctx->device));
    if (const int rc = ctx->ensure_pidx()) return rc;
    const size_t plane_bytes = std::max<size_t>(sizeof(float) * paired_hyp_floats(L) * (size_t)num_hyp, 256);
    if (const int rc = take_device(plane_bytes, ctx->device, reinterpret_cast<void**>(&c->d_planes_), &c->d_planes_bytes_, kNoMemWho))
        return rc;
    if (const int rc = c->stage_.create(ctx, (size_t)num_hyp * VB2_BATCH_SLOTS,
                                        (size_t)kMaxPointsPerLaunch * (size_t)std::max(1, marker_sum_tile_groups(L)), kNoMemWho))
        return rc;
    c->device_bytes = (int64_t)(c->d_planes_bytes_ + c->stage_.device_bytes());
    *out = c.release();
    return VB2_OK;
}

// the count of the markers a hypothesis walks: its pi2[0] plane comes down once (the marker unit holds no counter)
int Paired::count_given(const char* who)
{
    const DeviceLayout& L = ctx->L;
    const size_t mp = (size_t)L.m_pad, na = (size_t)std::max<long long>(0, (long long)L.num_active);
    std::vector<float> plane(std::max<size_t>(na, 1));
    for (int h = 0; h < num_hyp; ++h) {
        int64_t n = 0;
        if (na > 0) {
            const hipError_t e = hipMemcpy(plane.data(), d_planes_ + (size_t)h * paired_hyp_floats(L) + 3 * mp, sizeof(float) * na,
                                           hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                set_error(std::string(who) + ": the download of a plane failed: " + hipGetErrorString(e));
                return VB2_ERR_HIP;
            }
            for (size_t i = 0; i < na; ++i) n += !(plane[i] < 0.0f);
        }
        given[(size_t)h] = n;
    }
    return VB2_OK;
}

int Paired::create(Context* ctx, int num_hyp, const float* prior, Paired** out)
{
    *out = nullptr;
    if (!prior) {
        set_error("vb2_paired_create: invalid argument");
        return VB2_ERR_INVALID;
    }
    Paired* raw = nullptr;
    if (const int rc = make(ctx, num_hyp, "vb2_paired_create", &raw)) return rc;
    std::unique_ptr<Paired> c(raw);
    // the panel-order rows go up once, into a slab that goes back to the cache when the permutation is done
    const size_t bytes = sizeof(float) * 6 * (size_t)ctx->num_marker * (size_t)num_hyp;
    void* d_panel = nullptr;
    size_t d_panel_bytes = 0;
    if (const int rc = take_device(std::max<size_t>(bytes, 256), ctx->device, &d_panel, &d_panel_bytes, kNoMemWho)) return rc;
    hipError_t e = hipMemcpyAsync(d_panel, prior, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = launch_pair_permute(ctx->L, ctx->num_marker, num_hyp, static_cast<const float*>(d_panel), ctx->d_pidx, c->d_planes_,
                                ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    give_device(d_panel, d_panel_bytes, ctx->device);
    if (e != hipSuccess) {
        set_error(std::string("vb2_paired_create: prior upload failed: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    if (const int rc = c->count_given("vb2_paired_create")) return rc;
    *out = c.release();
    return VB2_OK;
}

int Paired::create_from_set(Context* ctx, SourceSet* set, int num_hyp, const int32_t* normal, double hom_min, Paired** out)
{
    *out = nullptr;
    if (!ctx || !set || !normal || !(hom_min >= 0.0 && hom_min <= 1.0)) {
        set_error("vb2_paired_create_from_set: invalid argument (hom_min within [0, 1])");
        return VB2_ERR_INVALID;
    }
    if (set->num_marker() != ctx->num_marker || set->device() != ctx->device) {
        set_error("vb2_paired_create_from_set: the context is of another panel size or on another device than the set");
        return VB2_ERR_INVALID;
    }
    std::vector<const float*> rows((size_t)std::max(num_hyp, 0));
    for (int h = 0; h < num_hyp; ++h) {
        rows[(size_t)h] = set->q_row(normal[h]);
        if (!rows[(size_t)h]) {
            set_error("vb2_paired_create_from_set: normal " + std::to_string(normal[h]) + " has no row in the set");
            return VB2_ERR_INVALID;
        }
    }
    Paired* raw = nullptr;
    if (const int rc = make(ctx, num_hyp, "vb2_paired_create_from_set", &raw)) return rc;
    std::unique_ptr<Paired> c(raw);
    // (the set's rows were written by contexts' streams that have been synchronised since: source.cpp, Context::marginals)
    hipError_t e = hipSuccess;
    for (int h = 0; h < num_hyp && e == hipSuccess; ++h)
        e = launch_pair_build(ctx->L, ctx->num_marker, rows[(size_t)h], ctx->d_pidx, hom_min,
                              c->d_planes_ + (size_t)h * paired_hyp_floats(ctx->L), ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        set_error(std::string("vb2_paired_create_from_set: building the hypotheses failed: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    if (const int rc = c->count_given("vb2_paired_create_from_set")) return rc;
    *out = c.release();
    return VB2_OK;
}

Paired::~Paired()
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // a begun evaluation reads the planes: it has to be over before they are given back
    (void)stage_.end(nullptr);
    give_device(d_planes_, d_planes_bytes_, ctx->device);
}

PointStage::Launch Paired::launcher() const
{
    return [this](int c, const double* d_rows, const int32_t* d_hyp, double* d_partial, double* d_out, hipStream_t s) {
        return launch_llk_paired(ctx->L, c, d_rows, d_hyp, d_planes_, d_partial, d_out, s);
    };
}

int Paired::eval_begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha)
{
    if (!num_point || stage_.pending()) {
        set_error("vb2_paired_eval: invalid argument");
        return VB2_ERR_INVALID;
    }
    size_t total = 0;
    if (!PointStage::count(num_hyp, num_point, &total)) {
        set_error("vb2_paired_eval: a hypothesis's point count outside 0..VB2_BATCH_SLOTS");
        return VB2_ERR_INVALID;
    }
    if (total == 0) return VB2_OK;
    if (!pc1 || !pc2 || !alpha) {
        set_error("vb2_paired_eval: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (ctx->resident_active) {
        set_error("vb2_paired_eval: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    // the synchronisation is eval_end's
    return stage_.begin(num_hyp, num_point, total, pc1, pc2, alpha, launcher());
}

int Paired::eval_end(double* llk) { return stage_.end(llk); }

int Paired::eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk)
{
    const int rc = eval_begin(num_point, pc1, pc2, alpha);
    if (rc) {
        (void)eval_end(nullptr);           // whatever reached the stream has left the stages when this returns
        return rc;
    }
    if (stage_.pending() && !llk) {
        (void)eval_end(nullptr);
        set_error("vb2_paired_eval: invalid argument");
        return VB2_ERR_INVALID;
    }
    return eval_end(llk);
}

int Paired::time_launch(int num_point, int warmup, int reps, double* ms)
{
    return stage_.time_launch(num_point, num_hyp, warmup, reps, ms, launcher());
}

namespace {
// what a hypothesis's Estimator calls: pc2 replaced by the fixed row, the gang's evaluator, and a look at the first values.
// (Under is_heter = 0 the Estimator packs pc1 = pc2 = v: the searched PCs travel on as pc1, the contaminant's.)
struct Wrap {
    void* gang_user = nullptr;
    const double* fixed = nullptr;
    int k = 0;
    bool first = true, empty = false;
    std::vector<double> p2;                // (not on the fiber's stack: alive while the request is parked)
};
int wrap_eval(void* user, int32_t n, const double* p1, const double*, const double* a, double* o)
{
    Wrap* w = static_cast<Wrap*>(user);
    w->p2.resize((size_t)std::max(n, 0) * (size_t)w->k);
    for (int i = 0; i < n; ++i) std::memcpy(&w->p2[(size_t)i * w->k], w->fixed, sizeof(double) * w->k);
    if (const int rc = FiberGang::eval_cb(w->gang_user, n, p1, w->p2.data(), a, o)) return rc;
    if (w->first) {
        w->first = false;
        bool all_zero = n > 0;
        for (int i = 0; i < n; ++i) all_zero = all_zero && o[i] == 0.0;
        if (all_zero) {
            w->empty = true;
            return VB2_ERR_INVALID;
        }
    }
    return 0;
}
}  // namespace

int paired_lockstep(PairedStep fn, void* user, int num_hyp, int num_pc, const uint8_t* known_af, const vb2_model& model,
                    const double* pc2_fixed, const int32_t* fixed_row, vb2_estimate* est, int32_t* status)
{
    const int H = num_hyp, k = num_pc;
    if (model.is_alpha_fixed) {
        set_error("vb2_paired_optimize_llk: a fixed alpha leaves the refit nothing to estimate (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    FiberGang gang(H, VB2_BATCH_SLOTS);
    std::vector<Wrap> wraps(H);
    vb2_model homo = model;                    // pc1 = pc2 = v, the reference's start, llk0 at alpha = 0
    homo.is_heter = 0;
    homo.notices = 0;                          // (the reference's phase lines belong to the run's own search)
    homo.verbose = 0;
    auto body = [&](int i) {
        wraps[i].gang_user = gang.user(i);
        wraps[i].fixed = pc2_fixed + (size_t)(fixed_row ? fixed_row[i] : i) * k;
        wraps[i].k = k;
        FiberGang::Search cfg;
        cfg.model = &homo;
        cfg.data_has_known_af = known_af && known_af[i];
        cfg.eval = wrap_eval;
        cfg.eval_user = &wraps[i];
        std::memset(&est[i], 0, sizeof(est[i]));
        status[i] = gang.search(i, cfg, "vb2_paired_optimize_llk", &est[i]);
    };
    std::vector<int32_t> npt(H);
    std::vector<double> p1, p2, al, vals;
    auto step = [&](std::vector<FiberGang::Request>& req) {
        p1.clear(); p2.clear(); al.clear();
        for (int h = 0; h < H; ++h) {
            const FiberGang::Request& q = req[h];
            npt[h] = q.n > 0 ? q.n : 0;
            if (q.n <= 0) continue;
            p1.insert(p1.end(), q.p1, q.p1 + (size_t)q.n * k);
            p2.insert(p2.end(), q.p2, q.p2 + (size_t)q.n * k);
            al.insert(al.end(), q.a, q.a + q.n);
        }
        vals.assign(al.size(), 0.0);
        if (const int rc = fn(user, npt.data(), p1.data(), p2.data(), al.data(), vals.data())) return rc;
        size_t o = 0;
        for (int h = 0; h < H; ++h) {
            if (req[h].n <= 0) continue;
            std::memcpy(req[h].out, &vals[o], sizeof(double) * req[h].n);
            o += (size_t)req[h].n;
        }
        return 0;
    };
    const int rc = gang.run(k, body, step);
    if (rc) return rc;
    for (int h = 0; h < H; ++h) {
        if (wraps[h].empty) {
            status[h] = VB2_ERR_INVALID;
            set_error("vb2_paired_optimize_llk: a hypothesis leaves the sample no marker");
        }
    }
    return VB2_OK;
}

namespace {
struct SetsStep {
    Paired* const* sets;
    int num_set, k;
};
int sets_step(void* user, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk)
{
    const SetsStep* S = static_cast<const SetsStep*>(user);
    const int k = S->k;
    // begin every set with live points, then collect: sets on different contexts overlap on the device
    std::vector<size_t> at((size_t)S->num_set + 1, 0);
    int rc = VB2_OK, hyp = 0, begun = 0;
    for (int s = 0; s < S->num_set; ++s) {
        size_t n = 0;
        for (int h = 0; h < S->sets[s]->num_hyp; ++h) n += (size_t)num_point[hyp + h];
        at[(size_t)s + 1] = at[(size_t)s] + n;
        hyp += S->sets[s]->num_hyp;
    }
    hyp = 0;
    for (int s = 0; s < S->num_set && !rc; ++s) {
        const size_t o = at[(size_t)s];
        if (at[(size_t)s + 1] > o) rc = S->sets[s]->eval_begin(num_point + hyp, pc1 + o * k, pc2 + o * k, alpha + o);
        hyp += S->sets[s]->num_hyp;
        begun = s + 1;
    }
    for (int s = 0; s < begun; ++s) {
        const int re = S->sets[s]->eval_end(rc ? nullptr : llk + at[(size_t)s]);
        if (!rc) rc = re;
    }
    return rc;
}
}  // namespace

int paired_optimize(Paired* const* sets, int num_set, const vb2_model& model, const double* pc2_fixed, vb2_estimate* est,
                    int32_t* status)
{
    if (!sets || num_set < 1 || !pc2_fixed || !est || !status) {
        set_error("vb2_paired_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    int H = 0;
    for (int s = 0; s < num_set; ++s) {
        if (!sets[s] || !sets[s]->ctx) {
            set_error("vb2_paired_optimize_llk: invalid argument");
            return VB2_ERR_INVALID;
        }
        if (sets[s]->ctx->num_pc != sets[0]->ctx->num_pc) {
            set_error("vb2_paired_optimize_llk: the sets' contexts differ in the number of PCs");
            return VB2_ERR_INVALID;
        }
        if (sets[s]->ctx->resident_active) {
            set_error("vb2_paired_optimize_llk: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
            return VB2_ERR_INVALID;
        }
        for (int t = 0; t < s; ++t)
            if (sets[t] == sets[s]) {
                set_error("vb2_paired_optimize_llk: a set is listed twice");
                return VB2_ERR_INVALID;
            }
        H += sets[s]->num_hyp;
    }
    std::vector<uint8_t> kaf((size_t)H);
    std::vector<int32_t> row((size_t)H);
    int h = 0;
    for (int s = 0; s < num_set; ++s)
        for (int j = 0; j < sets[s]->num_hyp; ++j, ++h) {
            kaf[(size_t)h] = sets[s]->ctx->L.known_af != nullptr;
            row[(size_t)h] = s;
        }
    SetsStep S{sets, num_set, sets[0]->ctx->num_pc};
    return paired_lockstep(sets_step, &S, H, S.k, kaf.data(), model, pc2_fixed, row.data(), est, status);
}

}  // namespace vb2

using vb2::set_error;

namespace {
template <class F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}
}  // namespace

extern "C" {

int vb2_paired_create(vb2_ctx* ctx, int32_t num_hyp, const float* prior, vb2_paired** out)
{
    if (!out) {
        set_error("vb2_paired_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (!ctx || !ctx->impl) {
        set_error("null vb2_ctx");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Paired* c = nullptr;
        if (const int rc = vb2::Paired::create(ctx->impl, num_hyp, prior, &c)) return rc;
        *out = new vb2_paired{c};
        return VB2_OK;
    });
}

int vb2_paired_create_from_set(vb2_ctx* ctx, vb2_source_set* set, int32_t num_hyp, const int32_t* normal, double hom_min,
                               vb2_paired** out)
{
    if (!out) {
        set_error("vb2_paired_create_from_set: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (!ctx || !ctx->impl || !set || !set->impl) {
        set_error("vb2_paired_create_from_set: null vb2_ctx or vb2_source_set");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Paired* c = nullptr;
        if (const int rc = vb2::Paired::create_from_set(ctx->impl, set->impl, num_hyp, normal, hom_min, &c)) return rc;
        *out = new vb2_paired{c};
        return VB2_OK;
    });
}

void vb2_paired_destroy(vb2_paired* pair)
{
    if (!pair) return;
    delete pair->impl;
    delete pair;
}

int vb2_paired_eval(vb2_paired* pair, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                    double* llk_out)
{
    if (!pair || !pair->impl) {
        set_error("null vb2_paired");
        return VB2_ERR_INVALID;
    }
    return pair->impl->eval(num_point, pc1, pc2, alpha, llk_out);
}

int vb2_paired_optimize_llk(vb2_paired* const* sets, int32_t num_set, const vb2_model* model, const double* pc2_fixed,
                            vb2_estimate* est_out, int32_t* status)
{
    if (!sets || num_set < 1 || !model) {
        set_error("vb2_paired_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        std::vector<vb2::Paired*> impl((size_t)num_set);
        for (int s = 0; s < num_set; ++s) {
            if (!sets[s] || !sets[s]->impl) {
                set_error("null vb2_paired");
                return VB2_ERR_INVALID;
            }
            impl[(size_t)s] = sets[s]->impl;
        }
        return vb2::paired_optimize(impl.data(), num_set, *model, pc2_fixed, est_out, status);
    });
}

int vb2_debug_paired_time(vb2_paired* pair, int32_t num_point, int32_t warmup, int32_t reps, double* ms)
{
    if (!pair || !pair->impl) return VB2_ERR_INVALID;
    return pair->impl->time_launch(num_point, warmup, reps, ms);
}

int vb2_paired_info_get(const vb2_paired* pair, vb2_paired_info* info, int64_t* given)
{
    if (!pair || !pair->impl || !info) return VB2_ERR_INVALID;
    const vb2::Paired& c = *pair->impl;
    info->num_hyp = c.num_hyp;
    info->num_marker = c.ctx->num_marker;
    info->device_bytes = c.device_bytes;
    info->num_step = c.num_step();
    info->num_launch = c.num_launch();
    if (given) std::copy(c.given.begin(), c.given.end(), given);
    return VB2_OK;
}

namespace {
struct SeamStep {
    vb2_paired_eval_fn fn;
    void* user;
    int num_hyp;
};
static int pair_seam_step(void* user, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk)
{
    const SeamStep* s = static_cast<const SeamStep*>(user);
    return s->fn(s->user, s->num_hyp, num_point, pc1, pc2, alpha, llk);
}
}  // namespace

int vb2_paired_lockstep(vb2_paired_eval_fn fn, void* user, int32_t num_hyp, int32_t num_pc, const vb2_model* model,
                        const double* pc2_fixed, vb2_estimate* est_out, int32_t* status)
{
    if (!fn || !model || !pc2_fixed || !est_out || !status || num_hyp < 1 || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_paired_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        SeamStep s{fn, user, num_hyp};
        return vb2::paired_lockstep(pair_seam_step, &s, num_hyp, num_pc, nullptr, *model, pc2_fixed, nullptr, est_out, status);
    });
}

}  // extern "C"
