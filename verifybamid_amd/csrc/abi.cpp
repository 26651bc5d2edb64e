// abi.cpp -- the extern "C" surface declared in include/vb2_abi.h.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>
#include <deque>
#include <functional>
#include <chrono>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <new>

#include "tunables.h"
#include "batch.h"
#include "context.h"
#include "estimator.h"
#include "guard.h"
#include "host_clock.h"
#include "line_search.h"
#include "lockstep.h"
#include "hostio.h"
#include "shard.h"
#include "replicates.h"
#include "read_groups.h"
#include "bgzf_inflate_kernels.h"
#include "baq_host.h"
#include "fasta_io.h"

using vb2::now_s;
using vb2::set_error;

namespace {

// Joins a helper thread on every path out of a scope: an exception on the main thread must not
// unwind past a joinable std::thread (that is std::terminate, not an error code).
struct JoinGuard {
    std::thread& t;
    explicit JoinGuard(std::thread& th) : t(th) {}
    ~JoinGuard() { if (t.joinable()) t.join(); }
};

int guard_ctx(const vb2_ctx* ctx)
{
    if (!ctx || !ctx->impl) {
        set_error("null vb2_ctx");
        return VB2_ERR_INVALID;
    }
    return VB2_OK;
}

int ctx_eval_cb(void* user, int32_t n, const double* pc1, const double* pc2, const double* alpha,
                double* out)
{
    return static_cast<vb2::Context*>(user)->eval_host(n, pc1, pc2, alpha, out);
}

// which "Estimation from ..." header the reference prints (ContaminationEstimator.cpp:98-150)
const char* estimation_title(const vb2_model& model)
{
    const bool heter = model.is_heter && !model.is_af_known;
    const bool pcfix = (model.is_pc_fixed && model.fix_pc) || model.is_af_known;
    const bool afix = !pcfix && model.is_alpha_fixed;
    if (!heter) return pcfix ? "Estimation from OptimizeHomoFixedPC:" : afix ? nullptr : "Estimation from OptimizeHomo:";
    return pcfix ? "Estimation from OptimizeHeterFixedPC:"
                 : afix ? "Estimation from OptimizeHeterFixedAlpha:" : "Estimation from OptimizeHeter:";
}

// The panel files of a run (reference order of errors: .bed, AF, .UD, .mu); .UD and .mu are parsed
// on helper threads while this one reads the .bed.
}  // namespace

namespace vb2 {
int load_panel(const vb2_run_args* a, vb2::Panel* panel)
{
    int rc_ud = VB2_OK, rc_mu = VB2_OK;
    std::string err_ud, err_mu;
    std::thread t_ud([&] {
        try { rc_ud = vb2::read_ud(a->ud_path, panel); if (rc_ud) err_ud = vb2::g_last_error; }
        catch (const std::exception& e) { rc_ud = VB2_ERR_NOMEM; err_ud = e.what(); }
    });
    std::thread t_mu([&] {
        try { rc_mu = vb2::read_mean(a->mean_path, panel); if (rc_mu) err_mu = vb2::g_last_error; }
        catch (const std::exception& e) { rc_mu = VB2_ERR_NOMEM; err_mu = e.what(); }
    });
    JoinGuard j_ud(t_ud), j_mu(t_mu);
    int rc = vb2::read_bed(a->bed_path, panel);
    if (!rc && a->known_af_path) rc = vb2::read_known_af(a->known_af_path, panel);
    if (!rc) panel->finish();
    const std::string err_main = rc ? vb2::g_last_error : std::string();
    t_ud.join();
    t_mu.join();
    if (rc) { set_error(err_main); return rc; }
    if (rc_ud) { set_error(err_ud); return rc_ud; }
    if (rc_mu) { set_error(err_mu); return rc_mu; }
    if (panel->means.size() < panel->NumMarker || panel->PosVec.size() < panel->NumMarker) {
        set_error(".UD has more rows than .mu/.bed");
        return VB2_ERR_INVALID;
    }
    return VB2_OK;
}
}  // namespace vb2

extern "C" {

int vb2_abi_version(void) { return VB2_ABI_VERSION; }

const char* vb2_last_error(void) { return vb2::g_last_error.c_str(); }

int vb2_device_count(void) { return vb2::usable_device_count(); }

int vb2_ctx_create(const vb2_input* in, const vb2_options* opt, vb2_ctx** out)
{
    if (!out) {
        set_error("vb2_ctx_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        vb2::Context* c = nullptr;
        const int rc = vb2::Context::create(in, opt, &c);
        if (rc) return rc;
        vb2_ctx* h = new vb2_ctx{c};
        *out = h;
        return VB2_OK;
    });
}

void vb2_ctx_destroy(vb2_ctx* ctx)
{
    if (!ctx) return;
    delete ctx->impl;
    delete ctx;
}

int vb2_ctx_info(const vb2_ctx* ctx, vb2_info* info)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (!info) return VB2_ERR_INVALID;
    ctx->impl->fill_info(info);
    return VB2_OK;
}

int vb2_llk_eval_batch(vb2_ctx* ctx, int32_t num_point, const double* pc1, const double* pc2,
                       const double* alpha, double* llk_out)
{
    if (int rc = guard_ctx(ctx)) return rc;
    return ctx->impl->eval_host(num_point, pc1, pc2, alpha, llk_out);
}

int vb2_llk_derivs_batch(vb2_ctx* ctx, int32_t num_point, const double* pc1, const double* pc2, const double* alpha,
                         double* llk_out, double* grad_out, double* hess_out)
{
    if (int rc = guard_ctx(ctx)) return rc;
    return ctx->impl->derivs_host(num_point, pc1, pc2, alpha, llk_out, grad_out, hess_out);
}

int vb2_llk_eval_batch_device(vb2_ctx* ctx, int32_t num_point, const double* d_points,
                              double* d_llk_out, void* stream)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (num_point < 0 || (num_point > 0 && (!d_points || !d_llk_out))) {
        set_error("vb2_llk_eval_batch_device: invalid argument");
        return VB2_ERR_INVALID;
    }
    return ctx->impl->eval_device(num_point, d_points, d_llk_out, (hipStream_t)stream);
}

// Profiling aid (not part of the public header): per-workgroup wall-clock stamps of the
// last launch when the context was created with VB2_STAMPS set.
// (test hook, not in vb2_abi.h) the host half of vb2_ctx_create without a device: digest of the flattened data
int vb2_debug_flatten_digest(const vb2_input* in, unsigned long long* digest)
{
    if (!in || !digest) return VB2_ERR_INVALID;
    try {
        return vb2::flatten_digest(in, digest);
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}

// (test hook, not in vb2_abi.h) the same digest over the data arrays as they are on the device
// What the device sustains with the evaluation kernels' instruction mix (calib_kernels.hip): out[0] FP64 FMA
// lane-instructions / s, arithmetic alone; out[1] with the table reads feeding it; out[2] the latter counting every VALU
// instruction of the loop.  bench.py's roofline quotes the kernels against these instead of a nominal clock.
int vb2_debug_issue_ceiling(int device, double* out)
{
    if (!out) return VB2_ERR_INVALID;
    if (vb2::usable_device_count() < 1) return VB2_ERR_NO_DEVICE;
    return vb2::measure_issue_ceiling(device, out) == hipSuccess ? VB2_OK : VB2_ERR_HIP;
}

int vb2_debug_layout_digest(vb2_ctx* ctx, unsigned long long* digest)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (!digest) return VB2_ERR_INVALID;
    return ctx->impl->layout_digest(digest);
}

// Test aid (not part of the public header): split launches of this process in sets of `ways` workgroups (-1: no such sets).
long long vb2_debug_split_launches(int ways) { return vb2::split_launches(ways); }

int vb2_debug_read_stamps(vb2_ctx* ctx, unsigned long long* out, int max_blocks)
{
    if (guard_ctx(ctx)) return 0;
    return ctx->impl->read_stamps(out, max_blocks);
}

// Test aid (not part of the public header): batches served by the resident search kernel.
long long vb2_debug_resident_evals(vb2_ctx* ctx)
{
    if (guard_ctx(ctx)) return -1;
    return (long long)ctx->impl->resident_evals;
}

int vb2_ctx_search_begin(vb2_ctx* ctx)
{
    if (int rc = guard_ctx(ctx)) return rc;
    (void)ctx->impl->resident_begin();         // unavailable -> plain launches, still a success
    return VB2_OK;
}

void vb2_ctx_search_end(vb2_ctx* ctx)
{
    if (guard_ctx(ctx)) return;
    ctx->impl->resident_end();
}

// Test aids (not part of the public header): Minimize() calls served by the on-device simplex;
// switch that mode off/on for one context (VB2_DEVICE_SIMPLEX does it globally).
long long vb2_debug_device_minimizes(vb2_ctx* ctx)
{
    if (guard_ctx(ctx)) return -1;
    return (long long)ctx->impl->device_minimizes;
}

void vb2_debug_set_device_simplex(vb2_ctx* ctx, int on)
{
    if (guard_ctx(ctx)) return;
    ctx->impl->device_simplex_enabled = on != 0;
}

// ... and the largest simplex dimension the context's last resident kernel kept state for (Context::resident_nmax;
// 0: none yet, the mode off, or 2 * num_pc + 1 beyond kDeviceSimplexMaxDim)
int vb2_debug_resident_nmax(vb2_ctx* ctx)
{
    if (guard_ctx(ctx)) return -1;
    return ctx->impl->resident_nmax;
}

// Test aid (no device): the point a device Minimize() of `status` hands back to the host's minimiser (estimator.cpp)
void vb2_debug_minimize_handback(int status, int dim, const double* point, const double* start, double* out)
{
    std::vector<double> v;
    vb2::minimize_handback(status, dim, point, start, &v);
    std::copy(v.begin(), v.end(), out);
}

// Test aid: is the context in resident mode right now?
// test hook (not in vb2_abi.h): `runs` OptimizeLLK searches over a caller's evaluator, advancing in
// lock-step as fibers of this thread (lockstep.h: what cohorts and multi-start searches use), every
// step's requests answered by ONE call of `eval` with all points concatenated.  Run i starts from
// start index i (vb2_search_opts semantics, seed 1).  No device involved: the CPU suite drives it
// with the oracle as evaluator and compares each run with the same search done on its own.
int vb2_debug_lockstep_optimize(vb2_eval_fn eval, void* user, int32_t num_pc, const vb2_model* model, int32_t runs,
                                int32_t speculate, vb2_estimate* out, int64_t* num_step)
{
    if (!eval || !model || !out || runs < 1 || num_pc < 1 || num_pc > VB2_MAX_PC) return VB2_ERR_INVALID;
    try {
        vb2::FiberGang gang(runs, 4);
        std::vector<int> rcs(runs, 0);
        auto body = [&](int i) {
            vb2::FiberGang::Search cfg;
            cfg.model = model;
            cfg.speculate = speculate;
            cfg.start_index = i;
            cfg.start_seed = 1;
            rcs[i] = gang.search(i, cfg, "vb2_debug_lockstep_optimize", &out[i]);
        };
        const int rc = gang.run(num_pc, body, vb2::FiberGang::concat_step(num_pc, eval, user));
        if (num_step) *num_step = gang.steps;
        if (rc) return rc < 0 ? VB2_ERR_INVALID : rc;
        for (int i = 0; i < runs; ++i)
            if (rcs[i]) return rcs[i];
        return VB2_OK;
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}

// test hook (not in vb2_abi.h): the library's bracket + Brent (line_search.h) on a caller's scalar
// function; `committed` is called for every evaluation the reference's ScalarMinimizer would make,
// in its order (a speculative batch calls f for more points); out = {min, fmin, a, b, c}.
int vb2_debug_line_search(double (*f)(void* user, double x), void (*committed)(void* user, double x, double y),
                          void* user, double lo, double hi, double tol, int speculate, double* out)
{
    struct Obj : vb2::ScalarObjective {
        double (*f)(void*, double);
        void (*committed)(void*, double, double);
        void* user;
        int EvaluateBatch(int n, const double* x, double* y) override
        {
            for (int i = 0; i < n; ++i) y[i] = f(user, x[i]);
            return 0;
        }
        void Commit(double x, double y) override
        {
            if (committed) committed(user, x, y);
        }
    } obj;
    obj.f = f;
    obj.committed = committed;
    obj.user = user;
    vb2::BrentMinimizer bm;
    bm.func = &obj;
    bm.speculate = speculate != 0;
    bm.Bracket(lo, hi);
    if (!bm.error) bm.Brent(tol);
    out[0] = bm.min; out[1] = bm.fmin; out[2] = bm.a; out[3] = bm.b; out[4] = bm.c;
    return bm.stuck ? 1 : 0;
}

int vb2_debug_resident_active(vb2_ctx* ctx)
{
    if (guard_ctx(ctx)) return 0;
    return ctx->impl->resident_active ? 1 : 0;
}

// Test aid (not part of the public header): batches created from now on stream the 16-bit (1) or the 32-bit (0)
// run lists in their 1- and 2-point steps.
void vb2_debug_set_cohort_w16(int on) { vb2::tunables().cohort_w16 = on != 0; }

// Test aid: calls of more points than one launch's tables hold as the passes of one launch (1, the default) or as separate
// launches (0)
void vb2_debug_set_eval_passes(int on) { vb2::tunables().passes = on != 0; }

// Test / tool aid: the library's run-time switches by name (tunables.h).  0 on success, VB2_ERR_INVALID for an unknown name.
int vb2_debug_set_tunable(const char* name, int value) { return vb2::set_tunable(name, value) ? VB2_OK : VB2_ERR_INVALID; }
int vb2_debug_get_tunable(const char* name, int* value) { return vb2::get_tunable(name, value) ? VB2_OK : VB2_ERR_INVALID; }

// Test aid: turn the resident search mode off/on for one context (VB2_RESIDENT does it globally).
void vb2_debug_set_resident(vb2_ctx* ctx, int on)
{
    if (guard_ctx(ctx)) return;
    ctx->impl->resident_enabled = on != 0;
}

int vb2_optimize_llk(vb2_eval_fn eval, void* user, int32_t num_pc, const vb2_model* model,
                     vb2_estimate* out, vb2_trace* trace)
{
    if (!eval || !model || !out || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    try {
        vb2::Estimator est(num_pc, eval, user);
        vb2::apply_model(est, *model);
        est.trace = trace;
        if (trace) trace->count = 0;
        const int rc = est.OptimizeLLK();
        if (rc) return rc;
        vb2::fill_estimate(est, out);
        return VB2_OK;
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}

int vb2_ctx_optimize_llk(vb2_ctx* ctx, const vb2_model* model, vb2_estimate* out, vb2_trace* trace)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (!model || !out) {
        set_error("vb2_ctx_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    vb2::Context* c = ctx->impl;
    // the whole search runs against one resident kernel when that mode is available, and each
    // Minimize() of it on the device itself (resident_kernel.inc) when the simplex fits
    if (trace && trace->capacity > 0 && c->device_simplex_enabled) (void)c->reserve_trace(trace->capacity);
    const bool resident = c->resident_begin();
    int rc;
    try {
        vb2::Estimator est(c->num_pc, ctx_eval_cb, c);
        vb2::apply_model(est, *model, c->L.known_af != nullptr);
        est.trace = trace;
        if (trace) trace->count = 0;
        if (resident && c->device_simplex_dim() > 0 && !(trace && c->trace_stage_rows < trace->capacity))
            est.dev_ctx = c;
        rc = est.OptimizeLLK();
        if (!rc) vb2::fill_estimate(est, out);
    } catch (const std::exception& e) {
        set_error(e.what());
        rc = VB2_ERR_INVALID;
    }
    if (resident) c->resident_end();
    return rc;
}

int vb2_ctx_optimize_llk_ex(vb2_ctx* ctx, const vb2_model* model, const vb2_search_opts* opts,
                            vb2_estimate* best, vb2_estimate* all)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (!model || !best) {
        set_error("vb2_ctx_optimize_llk_ex: invalid argument");
        return VB2_ERR_INVALID;
    }
    const int S = opts ? std::max(1, (int)opts->num_start) : 1;
    const bool line = opts && opts->line_search != 0;
    if (S > 64) {
        set_error("vb2_ctx_optimize_llk_ex: at most 64 starts");
        return VB2_ERR_INVALID;
    }
    if (S == 1 && !line) {
        const int rc = vb2_ctx_optimize_llk(ctx, model, best, nullptr);
        if (!rc && all) all[0] = *best;
        return rc;
    }
    vb2::Context* c = ctx->impl;
    const int k = c->num_pc;
    return vb2::guarded([&]() -> int {
        if (S == 1) {
            // one run, Brent's single-point evaluations served by the resident kernel
            const bool resident = c->resident_begin();
            vb2::Estimator est(k, ctx_eval_cb, c);
            vb2::apply_model(est, *model, c->L.known_af != nullptr);
            est.line_search = line;
            est.start_seed = opts ? opts->seed : 0u;
            if (opts && opts->start_sd > 0) est.start_sd = opts->start_sd;
            const int rc = est.OptimizeLLK();
            if (resident) c->resident_end();
            if (rc) return rc;
            vb2::fill_estimate(est, best);
            if (all) all[0] = *best;
            return VB2_OK;
        }
        // S runs as fibers of this thread: a step's points (<= 4 per run) leave as ONE launch
        vb2::FiberGang gang(S, 4);
        std::vector<vb2_estimate> ests(S);
        std::vector<int> rcs(S, 0);
        vb2_model quiet = *model;              // (the reference's phase lines once, for its own start)
        quiet.notices = 0;
        auto body = [&](int i) {
            vb2::FiberGang::Search cfg;
            cfg.model = i > 0 ? &quiet : model;
            cfg.data_has_known_af = c->L.known_af != nullptr;
            cfg.speculate = S * 4 <= vb2::kMaxPointsPerLaunch ? 4 : 2;         // the whole step in one launch
            cfg.line_search = line;
            cfg.start_index = i;
            cfg.start_seed = opts ? opts->seed : 0u;
            cfg.start_sd = opts ? opts->start_sd : 0;
            rcs[i] = gang.search(i, cfg, "vb2_ctx_optimize_llk_ex", &ests[i]);
        };
        const int rc = gang.run(k, body, vb2::FiberGang::concat_step(k, ctx_eval_cb, c));
        if (rc < 0) {
            set_error("vb2_ctx_optimize_llk_ex: getcontext failed");
            return VB2_ERR_INVALID;
        }
        if (rc) return rc;
        int win = -1;
        for (int i = 0; i < S; ++i) {
            if (rcs[i]) return rcs[i];
            // (a run that wandered into NaN territory never wins)
            if (ests[i].llk1 == ests[i].llk1 && (win < 0 || ests[i].llk1 < ests[win].llk1)) win = i;
        }
        if (win < 0) win = 0;
        *best = ests[win];
        best->reserved = win;
        if (all) std::memcpy(all, ests.data(), sizeof(vb2_estimate) * S);
        return VB2_OK;
    });
}

int vb2_batch_create(vb2_ctx* const* ctxs, int32_t num_sample, vb2_batch** out)
{
    if (!out) return VB2_ERR_INVALID;
    *out = nullptr;
    try {
        vb2::Batch* b = nullptr;
        const int rc = vb2::Batch::create(ctxs, num_sample, &b);
        if (rc) return rc;
        *out = new vb2_batch{b};
        return VB2_OK;
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_NOMEM;
    }
}

void vb2_batch_destroy(vb2_batch* b)
{
    if (!b) return;
    delete b->impl;
    delete b;
}

int vb2_batch_eval(vb2_batch* b, const int32_t* num_point, const double* pc1, const double* pc2,
                   const double* alpha, double* llk_out)
{
    if (!b || !b->impl || !num_point || !pc1 || !pc2 || !alpha || !llk_out) {
        set_error("vb2_batch_eval: invalid argument");
        return VB2_ERR_INVALID;
    }
    return b->impl->eval(num_point, pc1, pc2, alpha, llk_out);
}

// Test aid: the batch evaluates the request classes of a step as separate launches (Batch::strict_shapes: what the
// streaming cohort search's batches do)
void vb2_debug_batch_set_strict(vb2_batch* b, int on)
{
    if (b && b->impl) b->impl->strict_shapes = on != 0;
}

// Test aid (not part of the public header): batches the last vb2_batch_optimize_llk regrouped its unfinished samples into.
long long vb2_debug_batch_regroups(vb2_batch* b)
{
    return b && b->impl ? (long long)b->impl->num_regroup : -1;
}

// Test aid (not part of the public header): kernel launches the batch has made so far (a step that is launched again,
// Batch::eval_end, counts twice).
long long vb2_debug_batch_launches(vb2_batch* b)
{
    return b && b->impl ? (long long)b->impl->num_launch : -1;
}

int vb2_batch_optimize_llk(vb2_batch* b, const vb2_model* models, int32_t num_model, vb2_estimate* out)
{
    if (!b || !b->impl) {
        set_error("vb2_batch_optimize_llk: null batch");
        return VB2_ERR_INVALID;
    }
    try {
        return b->impl->optimize(models, num_model, out);
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}

int vb2_batch_derivs(vb2_batch* b, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                     double* llk_out, double* grad_out, double* hess_out)
{
    if (!b || !b->impl || !num_point) {
        set_error("vb2_batch_derivs: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        return b->impl->derivs(num_point, pc1, pc2, alpha, llk_out, grad_out, hess_out);
    });
}

int vb2_batch_interval(vb2_batch* b, const vb2_model* models, int32_t num_model, const vb2_estimate* est, vb2_interval* out,
                       int32_t* status, int64_t* num_step)
{
    if (num_step) *num_step = 0;
    if (!b || !b->impl || !models || !est || !out || !status) {
        set_error("vb2_batch_interval: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        return vb2::batch_interval(b->impl, models, num_model, est, out, status, num_step, nullptr);
    });
}

int vb2_intervals_lockstep(vb2_batch_derivs_fn fn, void* user, int32_t num_sample, int32_t num_pc, const int32_t* data_has_known_af,
                           const vb2_model* models, int32_t num_model, const vb2_estimate* est, vb2_interval* out,
                           int32_t* status, int64_t* num_step)
{
    if (num_step) *num_step = 0;
    if (!fn) {
        set_error("vb2_intervals_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        const vb2::BatchDerivsFn call = [fn, user](int32_t ns, const int32_t* np, const double* p1, const double* p2,
                                                   const double* a, double* llk, double* grad, double* hess) {
            const int rc = fn(user, ns, np, p1, p2, a, llk, grad, hess);
            if (rc) set_error("vb2_intervals_lockstep: the evaluator failed");
            return rc;
        };
        return vb2::intervals_lockstep(num_sample, num_pc, data_has_known_af, models, num_model, est, call, out, status, num_step,
                                       nullptr);
    });
}

int vb2_shard_group_create(const vb2_input* in, const int32_t* devices, int32_t num_device, vb2_shard_group** out)
{
    if (!out) return VB2_ERR_INVALID;
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        vb2::ShardGroup* g = nullptr;
        const int rc = vb2::ShardGroup::create(in, devices, num_device, &g);
        if (rc) return rc;
        *out = new vb2_shard_group{g};
        return VB2_OK;
    });
}

int vb2_rccl_unique_id(void* id128)
{
    if (!id128) return VB2_ERR_INVALID;
    return vb2::rccl_unique_id(id128);
}

int vb2_shard_group_create_rank(const vb2_input* in, int32_t device, int32_t rank, int32_t nranks,
                                const void* id128, vb2_shard_group** out)
{
    if (!out) return VB2_ERR_INVALID;
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        vb2::ShardGroup* g = nullptr;
        const int rc = vb2::ShardGroup::create_rank(in, device, rank, nranks, id128, &g);
        if (rc) return rc;
        *out = new vb2_shard_group{g};
        return VB2_OK;
    });
}

int vb2_shard_group_eval(vb2_shard_group* g, int32_t num_point, const double* pc1, const double* pc2,
                         const double* alpha, double* llk_out)
{
    if (!g || !g->impl) {
        set_error("null vb2_shard_group");
        return VB2_ERR_INVALID;
    }
    return g->impl->eval(num_point, pc1, pc2, alpha, llk_out);
}

int vb2_shard_group_optimize_llk(vb2_shard_group* g, const vb2_model* model, vb2_estimate* out, vb2_trace* trace)
{
    if (!g || !g->impl) {
        set_error("null vb2_shard_group");
        return VB2_ERR_INVALID;
    }
    try {
        return g->impl->optimize(model, out, trace);
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}

int vb2_shard_group_info(const vb2_shard_group* g, vb2_shard_info* info)
{
    if (!g || !g->impl || !info) return VB2_ERR_INVALID;
    std::memset(info, 0, sizeof(*info));
    const vb2::ShardGroup& sg = *g->impl;
    info->num_shard = (int32_t)sg.ctx.size();
    info->nranks = sg.nranks;
    info->rank = sg.rank;
    info->uses_rccl = sg.use_rccl ? 1 : 0;
    info->num_allreduce = sg.num_allreduce;
    info->partial_sums = sg.partial_sums ? 1 : 0;
    info->rccl_stub = (sg.use_rccl && vb2::rccl_is_stub()) ? 1 : 0;
    for (size_t s = 0; s < sg.ctx.size() && s < 64; ++s) {
        info->marker_lo[s] = sg.lo[s];
        info->marker_hi[s] = sg.hi[s];
        info->num_read[s] = sg.ctx[s]->num_read;
    }
    return VB2_OK;
}

int vb2_shard_range(const vb2_input* in, int32_t rank, int32_t nranks, int32_t* lo, int32_t* hi)
{
    if (!in || !in->read_off || !lo || !hi || nranks < 1 || rank < 0 || rank >= nranks || in->num_marker < 0) {
        set_error("vb2_shard_range: invalid argument");
        return VB2_ERR_INVALID;
    }
    int l = 0, h = 0;
    vb2::shard_range(in, rank, nranks, &l, &h);
    *lo = l;
    *hi = h;
    return VB2_OK;
}

void vb2_shard_group_destroy(vb2_shard_group* g)
{
    if (!g) return;
    delete g->impl;
    delete g;
}

}  // extern "C"

namespace {

// A group's own sanity check (unless disabled), BuildResolvedMarkers and status, once the panel is complete.
void finish_group(const vb2_run_args* a, size_t g, vb2_flat_groups* groups)
{
    vb2_flat& f = *groups->flat[g];
    vb2_flat_groups::Info& gi = groups->info[g];
    f.sanity_disabled = a->disable_sanity != 0;
    f.from_bam = false;
    gi.status = VB2_OK;
    if (!f.sanity_disabled) {
        std::fprintf(stderr, "NOTICE - Marker sanity check of read group %s:\n", gi.id.c_str());
        if (!vb2::sanity_check(f.panel, &f.viewer)) gi.status = VB2_ERR_SANITY;
    }
    f.resolve();
    if (gi.status == VB2_OK && (f.read_off.empty() || f.read_off.back() == 0)) gi.status = VB2_GROUP_NO_BASE;
}

// vb2_flat_load, and with groups != nullptr vb2_flat_load_groups
int flat_load_impl(const vb2_run_args* a, vb2_flat** out, vb2_flat_groups* groups)
{
    if (!a || !out || !a->ud_path || !a->mean_path || !a->bed_path || (!a->pileup_path && !a->bam_path) ||
        a->num_pc < 1 || a->num_pc > VB2_MAX_PC || (groups && (a->pileup_path || !a->bam_path))) {
        set_error(groups ? "vb2_flat_load_groups: invalid argument (read groups are read from bam_path alone)" : "vb2_flat_load: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (a->bam_adjust != 0 && a->bam_adjust != 1) {
        set_error("vb2_flat_load: bam_adjust is " + std::to_string(a->bam_adjust) + "; it is 0 (BAM records as they are) or 1 (--ApplyBAQ)");
        return VB2_ERR_INVALID;
    }
    if (a->bam_adjust == 1 && a->bam_path && !a->pileup_path && !a->reference_path) {
        set_error("vb2_flat_load: bam_adjust = 1 (--ApplyBAQ) needs reference_path, the FASTA the BAM was aligned to");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        std::unique_ptr<vb2_flat> f(new vb2_flat());
        f->panel.numPC = a->num_pc;
        int rc;
        // constructor reads the .bed (ContaminationEstimator.cpp:47), then ReadSVDMatrix
        // The four files are independent until the markers are resolved: .UD and .mu are parsed
        // on two helper threads while this one reads the .bed (the pileup reader needs it) and
        // the pileup.  Errors are reported in the reference's reading order (.bed, AF, .UD, .mu).
        const bool timing = vb2::tunables().debug_timing != 0;
        const double tl0 = now_s();
        double tl_bed = 0, tl_pile = 0, tl_join = 0;
        int rc_ud = VB2_OK, rc_mu = VB2_OK;
        std::string err_ud, err_mu;
        std::thread t_ud([&] {
            try { rc_ud = vb2::read_ud(a->ud_path, &f->panel); if (rc_ud) err_ud = vb2::g_last_error; }
            catch (const std::exception& e) { rc_ud = VB2_ERR_NOMEM; err_ud = e.what(); }
        });
        std::thread t_mu([&] {
            try { rc_mu = vb2::read_mean(a->mean_path, &f->panel); if (rc_mu) err_mu = vb2::g_last_error; }
            catch (const std::exception& e) { rc_mu = VB2_ERR_NOMEM; err_mu = e.what(); }
        });
        JoinGuard j_ud(t_ud), j_mu(t_mu);
        rc = vb2::read_bed(a->bed_path, &f->panel);
        if (!rc && a->known_af_path) rc = vb2::read_known_af(a->known_af_path, &f->panel);
        if (!rc) f->panel.finish();
        tl_bed = now_s();
        int rc_pile = VB2_OK;
        std::string err_main = rc ? vb2::g_last_error : std::string(), err_pile;
        if (!rc) {
            vb2::BamReadHow how;
            how.bam_adjust = a->bam_adjust;
            how.baq_stats = &f->baq_stats;
            const std::string ref_path = a->reference_path ? a->reference_path : "";
            rc_pile = a->pileup_path ? vb2::read_pileup(a->pileup_path, f->panel, &f->viewer)
                      : groups       ? vb2::read_bam_groups(a->bam_path, f->panel_ptr, &f->viewer, &a->mpileup, a->device, &f->bam_stats, groups,
                                                            ref_path, &how)
                                     : vb2::read_bam(a->bam_path, ref_path, f->panel, &f->viewer, &a->mpileup, a->device, &f->bam_stats, &how);
            if (rc_pile) err_pile = vb2::g_last_error;
            f->from_bam = !a->pileup_path && !rc_pile;
            f->with_baq = f->from_bam && a->bam_adjust == 1;
        }
        tl_pile = now_s();
        t_ud.join();
        t_mu.join();
        tl_join = now_s();
        if (rc) { set_error(err_main); return rc; }
        if (rc_ud) { set_error(err_ud); return rc_ud; }
        if (rc_mu) { set_error(err_mu); return rc_mu; }
        if (f->panel.means.size() < f->panel.NumMarker || f->panel.PosVec.size() < f->panel.NumMarker) {
            set_error(".UD has more rows than .mu/.bed");
            return VB2_ERR_INVALID;
        }
        if (rc_pile) { set_error(err_pile); return rc_pile; }
        f->sanity_disabled = a->disable_sanity != 0;
        if (!f->sanity_disabled && !vb2::sanity_check(f->panel, &f->viewer)) {
            if (groups)
                for (size_t g = 0; g < groups->flat.size(); ++g) finish_group(a, g, groups);
            set_error("Insufficient Available markers, check input bam depth distribution in "
                      "output pileup file after specifying --OutputPileup");
            f->resolve();
            *out = f.release();
            return VB2_ERR_SANITY;
        }
        const double tl_san = now_s();
        f->resolve();
        if (groups)
            for (size_t g = 0; g < groups->flat.size(); ++g) finish_group(a, g, groups);
        if (timing)
            std::fprintf(stderr, "vb2_flat_load: .bed %.1f ms, pileup %.1f ms, wait for .UD/.mu %.1f ms, "
                         "sanity %.1f ms, resolve %.1f ms\n", 1e3 * (tl_bed - tl0), 1e3 * (tl_pile - tl_bed),
                         1e3 * (tl_join - tl_pile), 1e3 * (tl_san - tl_join), 1e3 * (now_s() - tl_san));
        *out = f.release();
        return VB2_OK;
    });
}

}  // namespace

extern "C" {

int vb2_flat_load(const vb2_run_args* a, vb2_flat** out) { return flat_load_impl(a, out, nullptr); }

int vb2_flat_load_groups(const vb2_run_args* a, vb2_flat** whole, vb2_flat_groups** groups)
{
    if (!groups || !whole) {
        set_error("vb2_flat_load_groups: invalid argument");
        return VB2_ERR_INVALID;
    }
    *groups = nullptr;
    *whole = nullptr;
    std::unique_ptr<vb2_flat_groups> g(new (std::nothrow) vb2_flat_groups());
    if (!g) return VB2_ERR_NOMEM;
    const int rc = flat_load_impl(a, whole, g.get());
    if (*whole) *groups = g.release();
    return rc;
}

int32_t vb2_flat_groups_count(const vb2_flat_groups* g) { return g ? (int32_t)g->info.size() : 0; }

const char* vb2_flat_groups_id(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->info.size() ? g->info[(size_t)i].id.c_str() : nullptr;
}

int64_t vb2_flat_groups_records(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->info.size() ? g->info[(size_t)i].records : 0;
}

int32_t vb2_flat_groups_status(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->info.size() ? g->info[(size_t)i].status : (int32_t)VB2_ERR_INVALID;
}

const vb2_flat* vb2_flat_groups_flat(const vb2_flat_groups* g, int32_t i)
{
    return g && i >= 0 && (size_t)i < g->flat.size() ? g->flat[(size_t)i].get() : nullptr;
}

int64_t vb2_flat_groups_unassigned(const vb2_flat_groups* g) { return g ? g->unassigned : 0; }

int vb2_flat_groups_seconds(const vb2_flat_groups* g, double* seconds_device, double* seconds_copyback)
{
    if (!g || !seconds_device || !seconds_copyback) return VB2_ERR_INVALID;
    *seconds_device = g->seconds_device;
    *seconds_copyback = g->seconds_copyback;
    return VB2_OK;
}

void vb2_flat_groups_free(vb2_flat_groups* g) { delete g; }

const vb2_input* vb2_flat_input(const vb2_flat* f) { return f ? &f->input : nullptr; }

int vb2_flat_stats(const vb2_flat* f, vb2_run_result* out)
{
    if (!f || !out) return VB2_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->num_marker = (int32_t)f->panel.NumMarker;
    out->num_site = f->num_site;
    out->num_bases = f->viewer.numBases;
    out->avg_depth = f->viewer.avgDepth;
    out->sd_depth = f->viewer.sdDepth;
    return VB2_OK;
}

void vb2_flat_free(vb2_flat* f) { delete f; }

int vb2_flat_bam_stats(const vb2_flat* f, vb2_bam_stats* out)
{
    if (!f || !out || !f->from_bam) {
        set_error("vb2_flat_bam_stats: not a vb2_flat loaded from a BAM");
        return VB2_ERR_INVALID;
    }
    *out = f->bam_stats;
    return VB2_OK;
}

int vb2_flat_baq_stats(const vb2_flat* f, vb2_baq_stats* out)
{
    if (!f || !out || !f->with_baq) {
        set_error("vb2_flat_baq_stats: not a vb2_flat loaded from a BAM with bam_adjust = 1");
        return VB2_ERR_INVALID;
    }
    *out = f->baq_stats;
    return VB2_OK;
}

struct vb2_baq_result {
    vb2::BaqRecords r;
};

int vb2_baq_records(const char* bam_path, const char* bed_path, const char* reference_path, const vb2_mpileup_opts* opts, int where,
                    int device, vb2_baq_result** out)
{
    if (!bam_path || !bed_path || !out) {
        set_error("vb2_baq_records: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        std::unique_ptr<vb2_baq_result> r(new vb2_baq_result());
        if (int rc = vb2::baq_records_file(bam_path, bed_path, reference_path ? reference_path : "", opts, where, device, &r->r)) return rc;
        *out = r.release();
        return VB2_OK;
    });
}

int64_t vb2_baq_result_num(const vb2_baq_result* r) { return r ? (int64_t)r->r.outcome.size() : 0; }
int64_t vb2_baq_result_qual_bytes(const vb2_baq_result* r) { return r ? (int64_t)r->r.qual.size() : 0; }

int vb2_baq_result_copy(const vb2_baq_result* r, uint64_t* qual_off, uint8_t* qual, int16_t* mapq, uint8_t* outcome, int32_t* cap4)
{
    if (!r) return VB2_ERR_INVALID;
    const vb2::BaqRecords& b = r->r;
    if (qual_off) std::copy(b.qual_off.begin(), b.qual_off.end(), qual_off);
    if (qual) std::copy(b.qual.begin(), b.qual.end(), qual);
    if (mapq) std::copy(b.mapq.begin(), b.mapq.end(), mapq);
    if (outcome) std::copy(b.outcome.begin(), b.outcome.end(), outcome);
    if (cap4) std::copy(b.cap4.begin(), b.cap4.end(), cap4);
    return VB2_OK;
}

int vb2_baq_result_stats(const vb2_baq_result* r, vb2_baq_stats* out)
{
    if (!r || !out) return VB2_ERR_INVALID;
    *out = r->r.stats;
    return VB2_OK;
}

void vb2_baq_result_free(vb2_baq_result* r) { delete r; }

int vb2_baq_case(const uint8_t* ref, int32_t l_ref, const uint8_t* query, const uint8_t* qual, int32_t l_query, int32_t bw, int32_t* state,
                 uint8_t* q, int32_t* undefined)
{
    if (l_query < 0 || l_ref < 0 || bw < 0 || (l_query > 0 && (!query || !qual || !state || !q)) || (l_ref > 0 && !ref)) {
        set_error("vb2_baq_case: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        const int u = vb2::baq::run_case(ref, l_ref, query, qual, l_query, bw, state, q);
        if (undefined) *undefined = u;
        return VB2_OK;
    });
}

int32_t vb2_baq_quantise(double z) { return vb2::baq::quantise(vb2::baq::tables().thresh, z); }

uint64_t vb2_baq_work_bytes(int32_t l_ref, int32_t l_query, int32_t bw) { return vb2::baq::work_bytes(l_ref, l_query, bw); }

int vb2_fasta_fetch(const char* fasta_path, const char* name, int64_t beg, int64_t end, uint8_t* out, int64_t* length)
{
    if (!fasta_path || !name) {
        set_error("vb2_fasta_fetch: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&]() -> int {
        vb2::fasta::Index idx;
        std::string err;
        if (int rc = vb2::fasta::open_index(fasta_path, &idx, &err)) {
            set_error(err);
            return rc;
        }
        const int s = idx.find(name);
        if (s < 0) {
            set_error(std::string("--Reference: ") + fasta_path + " has no sequence " + name);
            return VB2_ERR_INVALID;
        }
        if (length) *length = idx.seqs[(size_t)s].length;
        if (!out) return VB2_OK;
        if (beg < 0 || end < beg || end > idx.seqs[(size_t)s].length) {
            set_error("vb2_fasta_fetch: the span passes the sequence");
            return VB2_ERR_INVALID;
        }
        if (int rc = vb2::fasta::fetch_nt16(idx, s, beg, end, out, &err)) {
            set_error(err);
            return rc;
        }
        return VB2_OK;
    });
}

struct vb2_bam_scan_result {
    std::vector<uint64_t> voffset;
    vb2_bam_stats stats;
    std::string sample;
    std::vector<std::string> group_id;      // with VB2_BAM_SCAN_GROUPS
    std::vector<uint16_t> group;            // ... parallel to voffset
};

int vb2_bam_scan_ex(const char* bam_path, const char* bed_path, uint32_t flags, vb2_bam_scan_result** out)
{
    if (!bam_path || !bed_path || !out || (flags & ~VB2_BAM_SCAN_GROUPS)) {
        set_error("vb2_bam_scan: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return vb2::guarded([&]() -> int {
        std::unique_ptr<vb2_bam_scan_result> s(new vb2_bam_scan_result());
        const bool want = (flags & VB2_BAM_SCAN_GROUPS) != 0;
        if (int rc = vb2::bam_scan_file(bam_path, bed_path, &s->voffset, &s->stats, &s->sample, want ? &s->group_id : nullptr,
                                        want ? &s->group : nullptr))
            return rc;
        *out = s.release();
        return VB2_OK;
    });
}

int vb2_bam_scan(const char* bam_path, const char* bed_path, vb2_bam_scan_result** out) { return vb2_bam_scan_ex(bam_path, bed_path, 0, out); }

int32_t vb2_bam_scan_num_group(const vb2_bam_scan_result* scan) { return scan ? (int32_t)scan->group_id.size() : 0; }

const char* vb2_bam_scan_group_id(const vb2_bam_scan_result* scan, int32_t group)
{
    return scan && group >= 0 && (size_t)group < scan->group_id.size() ? scan->group_id[(size_t)group].c_str() : nullptr;
}

int64_t vb2_bam_scan_record_groups(const vb2_bam_scan_result* scan, uint16_t* group, int64_t capacity)
{
    if (!scan) return VB2_ERR_INVALID;
    const int64_t n = (int64_t)scan->group.size();
    for (int64_t i = 0; group && i < n && i < capacity; ++i) group[i] = scan->group[(size_t)i];
    return n;
}

int vb2_bam_scan_stats(const vb2_bam_scan_result* scan, vb2_bam_stats* out)
{
    if (!scan || !out) return VB2_ERR_INVALID;
    *out = scan->stats;
    return VB2_OK;
}

int64_t vb2_bam_scan_records(const vb2_bam_scan_result* scan, uint64_t* voffset, int64_t capacity)
{
    if (!scan) return VB2_ERR_INVALID;
    const int64_t n = (int64_t)scan->voffset.size();
    for (int64_t i = 0; voffset && i < n && i < capacity; ++i) voffset[i] = scan->voffset[(size_t)i];
    return n;
}

const char* vb2_bam_scan_sample(const vb2_bam_scan_result* scan) { return scan ? scan->sample.c_str() : ""; }

void vb2_bam_scan_free(vb2_bam_scan_result* scan) { delete scan; }

int vb2_bgzf_inflate(const uint8_t* file_bytes, int64_t n_bytes, int32_t device, uint8_t* out, int64_t out_capacity, int64_t* out_bytes,
                     int32_t* block_status, int32_t status_capacity, int32_t* num_block)
{
    if (n_bytes < 0 || (!file_bytes && n_bytes > 0) || out_capacity < 0 || (!out && out_capacity > 0) || !out_bytes || status_capacity < 0 ||
        (!block_status && status_capacity > 0) || !num_block) {
        set_error("vb2_bgzf_inflate: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out_bytes = 0;
    *num_block = 0;
    return vb2::guarded([&]() -> int {
        if (vb2::usable_device_count() < 1) {
            set_error("vb2_bgzf_inflate: no gfx950 device is visible (the host's inflate is zlib's, not this entry's)");
            return VB2_ERR_NO_DEVICE;
        }
        std::string err;
        const size_t batch = (size_t)std::max(vb2::tunables().bam_batch_kb, 1) << 10;
        const int rc = vb2::bgzf_inflate_buffer(file_bytes, (uint64_t)n_bytes, device, batch, out, out_capacity, out_bytes, block_status,
                                                status_capacity, num_block, &err);
        if (rc) set_error(err);
        return rc;                     // bamio's codes are the ABI's
    });
}

int vb2_cohort_bam_stats(int32_t sample, vb2_bam_stats* out)
{
    if (!out || !vb2::cohort_bam_stats_get(sample, out)) {
        set_error("vb2_cohort_bam_stats: not a sample of the last cohort run that was read from a BAM");
        return VB2_ERR_INVALID;
    }
    return VB2_OK;
}

// (tests) how a cohort treats a line of its list (0 text, 1 BAM, 2 CRAM, by name and by the CRAM magic), the host pool
// of one of its BAM loads among `readers` reader threads, and the most BAM loads in flight on one device in the last run
int vb2_debug_list_entry_kind(const char* path)
{
    if (!path) return -1;
    vb2::ListEntry k = vb2::classify_list_entry(path);
    if (k == vb2::ListEntry::kText && vb2::has_cram_magic(path)) k = vb2::ListEntry::kCram;
    return (int)k;
}
int vb2_debug_cohort_bam_pool(int readers) { return vb2::cohort_bam_pool(readers); }
int vb2_debug_cohort_bam_peak(void) { return vb2::cohort_bam_peak(); }

int vb2_bgzf_inflate_stats(vb2_bgzf_stats* out, int32_t reset)
{
    if (!out && !reset) return VB2_ERR_INVALID;
    vb2::InflateTotals t;
    vb2::inflate_totals(&t, reset != 0);
    if (out) {
        out->blocks = t.blocks;
        out->refused = t.refused;
        out->batches = t.batches;
        out->bytes_raw = t.bytes_raw;
        out->bytes_inflated = t.bytes_inflated;
        out->seconds_upload = t.seconds_upload;
        out->seconds_kernel = t.seconds_kernel;
        out->seconds_copyback = t.seconds_copyback;
        out->seconds_stage = t.seconds_stage;
    }
    return VB2_OK;
}

int vb2_ctx_interval(vb2_ctx* ctx, const vb2_model* model, const vb2_estimate* est, vb2_interval* out)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (!model || !est || !out) {
        set_error("vb2_ctx_interval: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::ctx_interval(ctx->impl, *model, *est, out);
}

}  // extern "C"

namespace {

// vb2_run, and with ci != nullptr vb2_run_interval; hook (may be null): a stage on the run's context after the search
// groups (may be null): loaded beside the whole sample (vb2_run_read_groups searches them afterwards)
int run_impl(const vb2_run_args* a, vb2_run_result* out, vb2_interval* ci, const vb2::RunHook* hook, vb2_flat_groups* groups = nullptr)
{
    if (!a || !out) {
        set_error("vb2_run: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (ci && a->devices && a->num_device > 1) {
        set_error("--ConfidenceInterval takes one device: it cannot be combined with marker shards over several --Devices");
        return VB2_ERR_INVALID;
    }
    const double t0 = now_s();
    // The HIP runtime takes ~0.2 s to come up in a fresh process: start that now, on a helper
    // thread, while this one reads the input files (errors surface later, in vb2_ctx_create).
    std::thread warm([dev = a->device] {
        if (dev >= 0) (void)hipSetDevice(dev);
        (void)hipFree(nullptr);
        (void)hipGetLastError();
    });
    vb2_flat* flat = nullptr;
    int rc;
    const bool notices = a->model.notices != 0;
    // main.cpp:321-378: the reference times "Load SVD reference data", "Read pileup" and "Marker
    // sanity check" one after the other; here the panel files and the pileup are read
    // concurrently, so the three are one phase
    if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Load SVD reference data + Read pileup + Marker sanity check\n");
    {
        JoinGuard j_warm(warm);
        rc = flat_load_impl(a, &flat, groups);
    }
    if (notices) {
        std::fprintf(stderr, "NOTICE - Finished phase: Load SVD reference data + Read pileup + Marker sanity check  "
                             "[%.3f seconds]\n", now_s() - t0);
        if (!rc && !a->disable_sanity) std::fprintf(stderr, "NOTICE - Passing Marker Sanity Check...\n");
    }
    std::unique_ptr<vb2_flat> holder(flat);
    if (rc == VB2_ERR_SANITY && flat && a->output_pileup && a->output_prefix)
        vb2::write_pileup(a->output_prefix, *flat);
    if (rc) return rc;
    vb2_flat_stats(flat, out);
    if (a->output_pileup && a->output_prefix && (rc = vb2::write_pileup(a->output_prefix, *flat)))
        return rc;

    vb2_model model = a->model;
    if (flat->panel.isAFknown) model.is_af_known = 1;
    const double t_flat0 = now_s();
    if (a->devices && a->num_device > 1) {
        // --Devices a,b,...: the sample's markers sharded over the devices (vb2_shard_group_*)
        if (a->search.num_start > 1 || a->search.line_search) {      // (never silently ignored)
            set_error("--NumStart / --LineSearch are single-device options: they cannot be combined with marker "
                      "shards over several --Devices");
            return VB2_ERR_INVALID;
        }
        vb2_shard_group* grp = nullptr;
        if ((rc = vb2_shard_group_create(&flat->input, a->devices, a->num_device, &grp))) return rc;
        out->seconds_load = now_s() - t0;
        if (notices)
            std::fprintf(stderr, "NOTICE - Finished phase: Flatten + upload to %d devices (marker shards, %s)  "
                                 "[%.3f seconds]\n", (int)a->num_device,
                         grp->impl->use_rccl ? "RCCL all-reduce" : "host sum", now_s() - t_flat0);
        const double t1 = now_s();
        if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Optimize likelihood\n");
        rc = vb2_shard_group_optimize_llk(grp, &model, &out->est, nullptr);
        out->seconds_optimize = now_s() - t1;
        if (notices)
            std::fprintf(stderr, "NOTICE - Finished phase: Optimize likelihood  [%.3f seconds]\n", out->seconds_optimize);
        vb2_shard_group_destroy(grp);
        if (rc) return rc;
    } else {
        vb2_options opt{};
        opt.device = (a->devices && a->num_device == 1) ? a->devices[0] : a->device;
        vb2_ctx* ctx = nullptr;
        if ((rc = vb2_ctx_create(&flat->input, &opt, &ctx))) return rc;
        out->seconds_load = now_s() - t0;
        if (notices)
            std::fprintf(stderr, "NOTICE - Finished phase: Flatten + upload to %s  [%.3f seconds]\n",
                         ctx->impl->device_name, now_s() - t_flat0);
        const double t1 = now_s();
        if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Optimize likelihood\n");      // main.cpp:382
        rc = (a->search.num_start > 1 || a->search.line_search)
                 ? vb2_ctx_optimize_llk_ex(ctx, &model, &a->search, &out->est, nullptr)
                 : vb2_ctx_optimize_llk(ctx, &model, &out->est, nullptr);
        out->seconds_optimize = now_s() - t1;
        if (notices)
            std::fprintf(stderr, "NOTICE - Finished phase: Optimize likelihood  [%.3f seconds]\n", out->seconds_optimize);
        if (!rc && ci) {
            const double t2 = now_s();
            if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Confidence interval\n");
            rc = vb2_ctx_interval(ctx, &model, &out->est, ci);
            if (notices)
                std::fprintf(stderr, "NOTICE - Finished phase: Confidence interval  [%.3f seconds, %lld derivative launches]\n",
                             now_s() - t2, (long long)ci->num_launch);
        }
        if (!rc && hook) rc = (*hook)(ctx, *flat, model, out->est);
        vb2_ctx_destroy(ctx);
        if (rc) return rc;
    }

    vb2::print_summary(estimation_title(model), a->num_pc, out->est);
    if (a->output_prefix) {
        if ((rc = vb2::write_ancestry(a->output_prefix, a->num_pc, out->est.pc, out->est.pc2))) return rc;
        // main.cpp:398-400: #READS is viewer.numBases for BAM input, "NA" for pileup input
        if ((rc = vb2::write_selfsm(a->output_prefix, *flat, out->est, a->pileup_path != nullptr))) return rc;
        if (ci && (rc = vb2::write_ci(a->output_prefix, *ci))) return rc;
    }
    if (ci) std::fprintf(stderr, "NOTICE - FREEMIX 95%% CI (profile likelihood): [%g, %g]\n", ci->lo, ci->hi);
    return VB2_OK;
}

}  // namespace

namespace vb2 {
int run_with_hook(const vb2_run_args* args, vb2_run_result* out, const RunHook& hook) { return run_impl(args, out, nullptr, &hook); }
}  // namespace vb2

extern "C" {

int vb2_run(const vb2_run_args* a, vb2_run_result* out) { return run_impl(a, out, nullptr, nullptr); }

int vb2_run_read_groups(const vb2_run_args* a, vb2_run_result* whole, int32_t capacity, vb2_group_result* group_results,
                        int32_t* num_group)
{
    if (!a || !whole || !num_group || capacity < 0 || (capacity > 0 && !group_results)) {
        set_error("vb2_run_read_groups: invalid argument");
        return VB2_ERR_INVALID;
    }
    *num_group = 0;
    if (!a->bam_path || a->pileup_path) {
        set_error("--PerReadGroup needs --BamFile (and no --PileupFile): read groups are read from a BAM's header and RG:Z fields");
        return VB2_ERR_INVALID;
    }
    if (a->devices && a->num_device > 1) {
        set_error("--PerReadGroup takes one device: it cannot be combined with marker shards over several --Devices");
        return VB2_ERR_INVALID;
    }
    if (a->search.num_start > 1 || a->search.line_search) {
        set_error("--PerReadGroup cannot be combined with --NumStart / --LineSearch: the groups are searched in lock-step by the "
                  "reference's optimiser");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<vb2_flat_groups> groups(new (std::nothrow) vb2_flat_groups());
    if (!groups) return VB2_ERR_NOMEM;
    if (int rc = run_impl(a, whole, nullptr, nullptr, groups.get())) return rc;
    return vb2::guarded([&]() -> int { return vb2::run_read_groups_stage(a, groups.get(), capacity, group_results, num_group); });
}

int vb2_run_interval(const vb2_run_args* a, vb2_run_result* out, vb2_interval* ci)
{
    if (!ci) {
        set_error("vb2_run_interval: invalid argument");
        return VB2_ERR_INVALID;
    }
    return run_impl(a, out, ci, nullptr);
}

}  // extern "C"
