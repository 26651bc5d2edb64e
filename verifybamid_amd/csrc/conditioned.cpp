// conditioned.cpp -- host side of the likelihood given a hypothesised contaminant (marker_sum_kernels.hip; DESIGN.md section
// 13): what fills the planes of a set of hypotheses (the rest of the set: row_set.cpp), and the refits' options (refit.h).
#include "conditioned.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "context.h"
#include "guard.h"
#include "marker_sum_kernels.h"
#include "source.h"

namespace vb2 {

namespace {
const RowSet::Kind kKind = {
    "vb2_conditioned_eval", "a hypothesis's", "hypotheses", "vb2_conditioned_create" /* (whichever way the set is made) */, false,
    [](const DeviceLayout& L) { return sizeof(float) * conditioned_hyp_floats(L); },
    [](const DeviceLayout& L, int num_point, const double* d_rows, const int32_t* d_hyp, const void* d_planes, double* d_partial,
       double* d_out, hipStream_t s) {
        return launch_llk_conditioned(L, num_point, d_rows, d_hyp, static_cast<const float*>(d_planes), d_partial, d_out, s);
    }};

// pc1 = pc2 = v, the reference's start, with pc1 -- the contaminant's -- held on the way to the evaluator
Refit refit_options(const double* pc1_fixed)
{
    Refit o;
    o.who = "vb2_conditioned_optimize_llk";
    o.empty_message = "vb2_conditioned_optimize_llk: the sample counts no marker under a hypothesis";
    o.held = Refit::kPc1;
    o.fixed = pc1_fixed;
    o.homogeneous = o.refuse_fixed_alpha = true;
    return o;
}
}  // namespace

Conditioned::Conditioned() : RowSet(kKind) {}

int Conditioned::create(Context* ctx, int num_hyp, const float* prior, Conditioned** out)
{
    *out = nullptr;
    if (!prior) {
        set_error("vb2_conditioned_create: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<Conditioned> c(new Conditioned());
    if (const int rc = c->init(ctx, num_hyp, "vb2_conditioned_create")) return rc;
    const size_t bytes = sizeof(float) * 3 * (size_t)ctx->num_marker * (size_t)num_hyp;
    if (const int rc = c->upload(prior, bytes, "vb2_conditioned_create: prior upload failed: ", [&](const void* d_panel) {
            return launch_prior_permute(ctx->L, ctx->num_marker, num_hyp, static_cast<const float*>(d_panel), ctx->d_pidx, c->planes(),
                                        ctx->stream);
        }))
        return rc;
    *out = c.release();
    return VB2_OK;
}

int Conditioned::create_from_set(Context* ctx, SourceSet* set, int num_hyp, const int32_t* candidate, Conditioned** out)
{
    *out = nullptr;
    if (!ctx || !set || !candidate) {
        set_error("vb2_conditioned_create_from_set: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (set->num_marker() != ctx->num_marker || set->device() != ctx->device) {
        set_error("vb2_conditioned_create_from_set: the context is of another panel size or on another device than the set");
        return VB2_ERR_INVALID;
    }
    std::vector<const float*> rows((size_t)std::max(num_hyp, 0));
    for (int h = 0; h < num_hyp; ++h) {
        rows[(size_t)h] = set->q_row(candidate[h]);
        if (!rows[(size_t)h]) {
            set_error("vb2_conditioned_create_from_set: candidate " + std::to_string(candidate[h]) + " has no row in the set");
            return VB2_ERR_INVALID;
        }
    }
    std::unique_ptr<Conditioned> c(new Conditioned());
    if (const int rc = c->init(ctx, num_hyp, "vb2_conditioned_create_from_set")) return rc;
    // (the set's rows were written by contexts' streams that have been synchronised since: source.cpp, Context::marginals)
    hipError_t e = hipSuccess;
    for (int h = 0; h < num_hyp && e == hipSuccess; ++h)
        e = launch_prior_permute(ctx->L, ctx->num_marker, 1, rows[(size_t)h], ctx->d_pidx,
                                 c->planes() + (size_t)h * conditioned_hyp_floats(ctx->L), ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        set_error(std::string("vb2_conditioned_create_from_set: the copy of the rows failed: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    *out = c.release();
    return VB2_OK;
}

int conditioned_lockstep(vb2_conditioned_eval_fn fn, void* user, int num_hyp, int num_pc, const vb2_model& model,
                         const double* pc1_fixed, vb2_estimate* est, int32_t* status)
{
    return refit_lockstep(refit_options(pc1_fixed), fn, user, num_hyp, num_pc, model, est, status);
}

int conditioned_optimize(Conditioned* const* sets, int num_set, const vb2_model& model, const double* pc1_fixed,
                         vb2_estimate* est, int32_t* status)
{
    return optimize_sets(sets, num_set, refit_options(pc1_fixed), model, est, status);
}

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

extern "C" {

int vb2_conditioned_create(vb2_ctx* ctx, int32_t num_hyp, const float* prior, vb2_conditioned** out)
{
    if (!out) {
        set_error("vb2_conditioned_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (!ctx || !ctx->impl) {
        set_error("null vb2_ctx");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Conditioned* c = nullptr;
        if (const int rc = vb2::Conditioned::create(ctx->impl, num_hyp, prior, &c)) return rc;
        *out = new vb2_conditioned{c};
        return VB2_OK;
    });
}

int vb2_conditioned_create_from_set(vb2_ctx* ctx, vb2_source_set* set, int32_t num_hyp, const int32_t* candidate,
                                    vb2_conditioned** out)
{
    if (!out) {
        set_error("vb2_conditioned_create_from_set: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (!ctx || !ctx->impl || !set || !set->impl) {
        set_error("vb2_conditioned_create_from_set: null vb2_ctx or vb2_source_set");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Conditioned* c = nullptr;
        if (const int rc = vb2::Conditioned::create_from_set(ctx->impl, set->impl, num_hyp, candidate, &c)) return rc;
        *out = new vb2_conditioned{c};
        return VB2_OK;
    });
}

void vb2_conditioned_destroy(vb2_conditioned* cond)
{
    if (!cond) return;
    delete cond->impl;
    delete cond;
}

int vb2_conditioned_eval(vb2_conditioned* cond, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                         double* llk_out)
{
    if (!cond || !cond->impl) {
        set_error("null vb2_conditioned");
        return VB2_ERR_INVALID;
    }
    return cond->impl->eval(num_point, pc1, pc2, alpha, llk_out);
}

int vb2_conditioned_optimize_llk(vb2_conditioned* const* sets, int32_t num_set, const vb2_model* model, const double* pc1_fixed,
                                 vb2_estimate* est_out, int32_t* status)
{
    if (!sets || num_set < 1 || !model) {
        set_error("vb2_conditioned_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        std::vector<vb2::Conditioned*> impl((size_t)num_set);
        for (int s = 0; s < num_set; ++s) {
            if (!sets[s] || !sets[s]->impl) {
                set_error("null vb2_conditioned");
                return VB2_ERR_INVALID;
            }
            impl[(size_t)s] = sets[s]->impl;
        }
        return vb2::conditioned_optimize(impl.data(), num_set, *model, pc1_fixed, est_out, status);
    });
}

int vb2_debug_conditioned_time(vb2_conditioned* cond, int32_t num_point, int32_t warmup, int32_t reps, double* ms)
{
    if (!cond || !cond->impl) return VB2_ERR_INVALID;
    return cond->impl->time_launch(num_point, warmup, reps, ms);
}

int vb2_conditioned_info_get(const vb2_conditioned* cond, vb2_conditioned_info* info)
{
    if (!cond || !cond->impl || !info) return VB2_ERR_INVALID;
    const vb2::Conditioned& c = *cond->impl;
    info->num_hyp = c.num_row;
    info->num_marker = c.ctx->num_marker;
    info->device_bytes = c.device_bytes;
    info->num_step = c.num_step();
    info->num_launch = c.num_launch();
    return VB2_OK;
}

int vb2_conditioned_lockstep(vb2_conditioned_eval_fn fn, void* user, int32_t num_hyp, int32_t num_pc, const vb2_model* model,
                             const double* pc1_fixed, vb2_estimate* est_out, int32_t* status)
{
    if (!fn || !model || !pc1_fixed || !est_out || !status || num_hyp < 1 || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_conditioned_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        return vb2::conditioned_lockstep(fn, user, num_hyp, num_pc, *model, pc1_fixed, est_out, status);
    });
}

}  // extern "C"
