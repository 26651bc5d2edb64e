// paired.cpp -- host side of the likelihood given priors on both components (marker_sum_kernels.hip: PairTerm; DESIGN.md
// section 16): what fills the planes of a set of pair hypotheses (the rest of the set: row_set.cpp), and the options of the
// refits with the intended sample's PCs held (refit.h).
#include "paired.h"

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
    "vb2_paired_eval", "a hypothesis's", "hypotheses", "vb2_paired_create" /* (whichever way the set is made) */, false,
    [](const DeviceLayout& L) { return sizeof(float) * paired_hyp_floats(L); },
    [](const DeviceLayout& L, int num_point, const double* d_rows, const int32_t* d_hyp, const void* d_planes, double* d_partial,
       double* d_out, hipStream_t s) {
        return launch_llk_paired(L, num_point, d_rows, d_hyp, static_cast<const float*>(d_planes), d_partial, d_out, s);
    }};

// pc1 = pc2 = v, the reference's start, with pc2 -- the intended sample's -- held on the way to the evaluator: the searched
// PCs travel on as pc1, the contaminant's
Refit refit_options(const double* pc2_fixed)
{
    Refit o;
    o.who = "vb2_paired_optimize_llk";
    o.empty_message = "vb2_paired_optimize_llk: a hypothesis leaves the sample no marker";
    o.held = Refit::kPc2;
    o.fixed = pc2_fixed;
    o.homogeneous = o.refuse_fixed_alpha = true;
    return o;
}
}  // namespace

Paired::Paired() : RowSet(kKind) {}

// the count of the markers a hypothesis walks: its pi2[0] plane comes down once (the marker unit holds no counter)
int Paired::count_given(const char* who)
{
    const DeviceLayout& L = ctx->L;
    const size_t mp = (size_t)L.m_pad, na = (size_t)std::max<long long>(0, (long long)L.num_active);
    std::vector<float> plane(std::max<size_t>(na, 1));
    given.assign((size_t)num_row, 0);
    for (int h = 0; h < num_row; ++h) {
        int64_t n = 0;
        if (na > 0) {
            const hipError_t e = hipMemcpy(plane.data(), planes() + (size_t)h * paired_hyp_floats(L) + 3 * mp, sizeof(float) * na,
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
    std::unique_ptr<Paired> c(new Paired());
    if (const int rc = c->init(ctx, num_hyp, "vb2_paired_create")) return rc;
    const size_t bytes = sizeof(float) * 6 * (size_t)ctx->num_marker * (size_t)num_hyp;
    if (const int rc = c->upload(prior, bytes, "vb2_paired_create: prior upload failed: ", [&](const void* d_panel) {
            return launch_pair_permute(ctx->L, ctx->num_marker, num_hyp, static_cast<const float*>(d_panel), ctx->d_pidx, c->planes(),
                                       ctx->stream);
        }))
        return rc;
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
    std::unique_ptr<Paired> c(new Paired());
    if (const int rc = c->init(ctx, num_hyp, "vb2_paired_create_from_set")) return rc;
    // (the set's rows were written by contexts' streams that have been synchronised since: source.cpp, Context::marginals)
    hipError_t e = hipSuccess;
    for (int h = 0; h < num_hyp && e == hipSuccess; ++h)
        e = launch_pair_build(ctx->L, ctx->num_marker, rows[(size_t)h], ctx->d_pidx, hom_min,
                              c->planes() + (size_t)h * paired_hyp_floats(ctx->L), ctx->stream);
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

int paired_lockstep(vb2_paired_eval_fn fn, void* user, int num_hyp, int num_pc, const vb2_model& model, const double* pc2_fixed,
                    vb2_estimate* est, int32_t* status)
{
    return refit_lockstep(refit_options(pc2_fixed), fn, user, num_hyp, num_pc, model, est, status);
}

int paired_optimize(Paired* const* sets, int num_set, const vb2_model& model, const double* pc2_fixed, vb2_estimate* est,
                    int32_t* status)
{
    return optimize_sets(sets, num_set, refit_options(pc2_fixed), model, est, status);
}

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

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
    info->num_hyp = c.num_row;
    info->num_marker = c.ctx->num_marker;
    info->device_bytes = c.device_bytes;
    info->num_step = c.num_step();
    info->num_launch = c.num_launch();
    if (given) std::copy(c.given.begin(), c.given.end(), given);
    return VB2_OK;
}

int vb2_paired_lockstep(vb2_paired_eval_fn fn, void* user, int32_t num_hyp, int32_t num_pc, const vb2_model* model,
                        const double* pc2_fixed, vb2_estimate* est_out, int32_t* status)
{
    if (!fn || !model || !pc2_fixed || !est_out || !status || num_hyp < 1 || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_paired_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int { return vb2::paired_lockstep(fn, user, num_hyp, num_pc, *model, pc2_fixed, est_out, status); });
}

}  // extern "C"
