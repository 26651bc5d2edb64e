// abi.cpp -- the extern "C" surface declared in include/vb2_abi.h: version, error, contexts, searches, batches, shards,
// intervals and the single-sample runs.  Every entry checks its arguments and forwards; what may throw runs inside
// vb2::guarded.  The input side (vb2_flat_*, the BAM reader's diagnostics): abi_input.cpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "tunables.h"
#include "batch.h"
#include "context.h"
#include "estimator.h"
#include "guard.h"
#include "line_search.h"
#include "lockstep.h"
#include "hostio.h"
#include "shard.h"
#include "read_groups.h"
#include "run.h"

using vb2::set_error;

namespace {

int guard_ctx(const vb2_ctx* ctx)
{
    if (!ctx || !ctx->impl) {
        set_error("null vb2_ctx");
        return VB2_ERR_INVALID;
    }
    return VB2_OK;
}

// A search's resident kernel (Context::resident_begin; `on`: the mode was available), ended on every path out of the search
struct ResidentSearch {
    vb2::Context* c;
    const bool on;
    explicit ResidentSearch(vb2::Context* ctx) : c(ctx), on(ctx->resident_begin()) {}
    ResidentSearch(const ResidentSearch&) = delete;
    ResidentSearch& operator=(const ResidentSearch&) = delete;
    ~ResidentSearch() { if (on) c->resident_end(); }
};

int ctx_eval_cb(void* user, int32_t n, const double* pc1, const double* pc2, const double* alpha,
                double* out)
{
    return static_cast<vb2::Context*>(user)->eval_host(n, pc1, pc2, alpha, out);
}

}  // namespace

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
    // (a launch shape's first use builds its schedule on the host: Context::get)
    return vb2::guarded([&] { return ctx->impl->eval_host(num_point, pc1, pc2, alpha, llk_out); });
}

int vb2_llk_derivs_batch(vb2_ctx* ctx, int32_t num_point, const double* pc1, const double* pc2, const double* alpha,
                         double* llk_out, double* grad_out, double* hess_out)
{
    if (int rc = guard_ctx(ctx)) return rc;
    return vb2::guarded([&] { return ctx->impl->derivs_host(num_point, pc1, pc2, alpha, llk_out, grad_out, hess_out); });
}

int vb2_llk_eval_batch_device(vb2_ctx* ctx, int32_t num_point, const double* d_points,
                              double* d_llk_out, void* stream)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (num_point < 0 || (num_point > 0 && (!d_points || !d_llk_out))) {
        set_error("vb2_llk_eval_batch_device: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] { return ctx->impl->eval_device(num_point, d_points, d_llk_out, (hipStream_t)stream); });
}

// Profiling aid (not part of the public header): per-workgroup wall-clock stamps of the
// last launch when the context was created with VB2_STAMPS set.
// (test hook, not in vb2_abi.h) the host half of vb2_ctx_create without a device: digest of the flattened data
int vb2_debug_flatten_digest(const vb2_input* in, unsigned long long* digest)
{
    if (!in || !digest) return VB2_ERR_INVALID;
    return vb2::guarded([&] { return vb2::flatten_digest(in, digest); });
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
    return vb2::guarded([&]() -> int {
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
    });
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
    return vb2::guarded([&]() -> int {
        vb2::Estimator est(num_pc, eval, user);
        vb2::apply_model(est, *model);
        est.trace = trace;
        if (trace) trace->count = 0;
        const int rc = est.OptimizeLLK();
        if (rc) return rc;
        vb2::fill_estimate(est, out);
        return VB2_OK;
    });
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
    return vb2::guarded([&]() -> int {
        ResidentSearch resident(c);
        vb2::Estimator est(c->num_pc, ctx_eval_cb, c);
        vb2::apply_model(est, *model, c->L.known_af != nullptr);
        est.trace = trace;
        if (trace) trace->count = 0;
        if (resident.on && c->device_simplex_dim() > 0 && !(trace && c->trace_stage_rows < trace->capacity))
            est.dev_ctx = c;
        const int rc = est.OptimizeLLK();
        if (!rc) vb2::fill_estimate(est, out);
        return rc;
    });
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
            ResidentSearch resident(c);
            vb2::Estimator est(k, ctx_eval_cb, c);
            vb2::apply_model(est, *model, c->L.known_af != nullptr);
            est.line_search = line;
            est.start_seed = opts ? opts->seed : 0u;
            if (opts && opts->start_sd > 0) est.start_sd = opts->start_sd;
            const int rc = est.OptimizeLLK();
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
    return vb2::guarded([&]() -> int {
        vb2::Batch* b = nullptr;
        const int rc = vb2::Batch::create(ctxs, num_sample, &b);
        if (rc) return rc;
        *out = new vb2_batch{b};
        return VB2_OK;
    });
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
    // (a step of mixed request classes plans its launches in vectors: Batch::plan_step)
    return vb2::guarded([&] { return b->impl->eval(num_point, pc1, pc2, alpha, llk_out); });
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
    return vb2::guarded([&] { return b->impl->optimize(models, num_model, out); });
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
    return vb2::guarded([&] { return g->impl->eval(num_point, pc1, pc2, alpha, llk_out); });
}

int vb2_shard_group_optimize_llk(vb2_shard_group* g, const vb2_model* model, vb2_estimate* out, vb2_trace* trace)
{
    if (!g || !g->impl) {
        set_error("null vb2_shard_group");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] { return g->impl->optimize(model, out, trace); });
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

int vb2_ctx_interval(vb2_ctx* ctx, const vb2_model* model, const vb2_estimate* est, vb2_interval* out)
{
    if (int rc = guard_ctx(ctx)) return rc;
    if (!model || !est || !out) {
        set_error("vb2_ctx_interval: invalid argument");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] { return vb2::ctx_interval(ctx->impl, *model, *est, out); });
}

int vb2_run(const vb2_run_args* a, vb2_run_result* out)
{
    return vb2::guarded([&] { return vb2::run_sample(a, out); });
}

int vb2_run_read_groups(const vb2_run_args* a, vb2_run_result* whole, int32_t capacity, vb2_group_result* group_results,
                        int32_t* num_group)
{
    return vb2::guarded([&]() -> int {
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
        if (int rc = vb2::run_sample(a, whole, vb2::RunStage(), groups.get())) return rc;
        return vb2::run_read_groups_stage(a, groups.get(), capacity, group_results, num_group);
    });
}

}  // extern "C"
