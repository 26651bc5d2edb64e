// refbias.cpp -- host side of the reference bias (refbias_kernels.hip): what fills the rows of a set
// (the rest of the set: row_set.cpp), its lock-step refits (refit.h), the fixed procedure that maximises the profile
// likelihood over beta -- written once, so that the device and the numpy restatement go through the same code --, and the
// file flow behind --RefBias.
#include "refbias.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "context.h"
#include "guard.h"
#include "hostio.h"
#include "refbias_kernels.h"
#include "run.h"

namespace vb2 {

namespace {
const RowSet::Kind kKind = {
    "vb2_refbias_eval", "a row's", "rows", "vb2_refbias_create", false,
    [](const DeviceLayout&) { return sizeof(double); },
    [](const DeviceLayout& L, int num_point, const double* d_rows, const int32_t* d_row_of, const void* d_beta, double* d_partial,
       double* d_out, hipStream_t s) {
        return launch_llk_bias(L, num_point, d_rows, d_row_of, static_cast<const double*>(d_beta), d_partial, d_out, s);
    }};

// the model's own search from the reference start: no side is held
Refit refit_options(const uint8_t* known_af, int64_t* num_step)
{
    Refit o;
    o.who = "vb2_refbias_optimize_llk";
    o.empty_message = "vb2_refbias_optimize_llk: the sample counts no marker";
    o.refuse_fixed_alpha = true;
    o.known_af = known_af;
    o.num_step = num_step;
    return o;
}

bool beta_in_domain(double b) { return b >= kBiasMin && b <= kBiasMax; }      // (false for a NaN)

int set_eval_cb(void* user, int32_t, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk)
{
    return static_cast<RefBias*>(user)->eval(num_point, pc1, pc2, alpha, llk);
}
}  // namespace

RefBias::RefBias() : RowSet(kKind) {}

int RefBias::create(Context* ctx, int num_row, const double* beta, RefBias** out)
{
    *out = nullptr;
    if (!beta) {
        set_error("vb2_refbias_create: invalid argument");
        return VB2_ERR_INVALID;
    }
    for (int r = 0; r < num_row; ++r)
        if (!beta_in_domain(beta[r])) {
            set_error("vb2_refbias_create: beta of row " + std::to_string(r) + " lies outside [0.25, 0.75]");
            return VB2_ERR_INVALID;
        }
    if (ctx && ctx->L.pd && ctx->pd_max_bound > kPdMaxBound / 2) {
        set_error("vb2_refbias_create: the sample's deepest marker may fall below 2^-450 at beta = 0.5, and a reference bias can "
                  "double that: too deep for the probability-domain layout under a bias; make the context with the tunable pd = 0 "
                  "(run words take any depth)");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<RefBias> b(new RefBias());
    if (const int rc = b->init(ctx, num_row, "vb2_refbias_create")) return rc;
    hipError_t e = hipMemcpyAsync(b->d_payload_, beta, sizeof(double) * (size_t)num_row, hipMemcpyHostToDevice, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);      // (beta is the caller's: read before this returns)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        set_error(std::string("vb2_refbias_create: beta upload failed: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    *out = b.release();
    return VB2_OK;
}

int RefBias::optimize(const vb2_model& model, vb2_estimate* est, int32_t* status)
{
    if (!est || !status) {
        set_error("vb2_refbias_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (ctx->resident_active) {
        set_error("vb2_refbias_optimize_llk: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    const std::vector<uint8_t> kaf((size_t)num_row, ctx->L.known_af != nullptr ? 1 : 0);
    return refit_lockstep(refit_options(kaf.data(), nullptr), set_eval_cb, this, num_row, ctx->num_pc, model, est, status);
}

// ---------------------------------------------------------------------------
// the estimate of beta
// ---------------------------------------------------------------------------
namespace {
// one lock-step call's rows on their way to the caller's evaluator
struct Call {
    vb2_refbias_eval_fn fn;
    void* user;
    const double* beta;
};
int call_eval(void* user, int32_t num_row, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
              double* llk)
{
    const Call* c = static_cast<const Call*>(user);
    return c->fn(c->user, num_row, num_point, c->beta, pc1, pc2, alpha, llk);
}

constexpr int kUnits = 1024;                       // a grid value is 0.25 + n / 1024, n = 0..512: exact
double beta_of(int n) { return kBiasMin + (double)n / (double)kUnits; }

// index of the largest value, the lowest on ties
int best_of(const double* l, int n)
{
    int b = 0;
    for (int i = 1; i < n; ++i)
        if (l[i] > l[b]) b = i;
    return b;
}
}  // namespace

int refbias_fit(vb2_refbias_eval_fn fn, void* user, int num_pc, const vb2_model& model, bool data_has_known_af,
                vb2_refbias_fit* out)
{
    std::memset(out, 0, sizeof(*out));
    out->beta = out->beta_se = out->alpha_bias = out->llk1_bias = out->llk1_at_half = out->alpha_at_half = out->lrt = NAN;
    if (model.is_alpha_fixed) {
        set_error("vb2_refbias_lockstep: a fixed alpha leaves the refit nothing to estimate (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    // the searches of one lock-step call; their (beta, llk1) pairs are appended in row order
    std::vector<vb2_estimate> est;
    const auto run = [&](const std::vector<double>& beta) -> int {
        const int R = (int)beta.size();
        est.assign((size_t)R, vb2_estimate{});
        std::vector<int32_t> status((size_t)R, 0);
        const std::vector<uint8_t> kaf((size_t)R, data_has_known_af ? 1 : 0);
        int64_t steps = 0;
        Call c{fn, user, beta.data()};
        const int rc = refit_lockstep(refit_options(kaf.data(), &steps), call_eval, &c, R, num_pc, model, est.data(), status.data());
        out->num_step += steps;
        if (rc) return rc;
        for (int r = 0; r < R; ++r)
            if (status[(size_t)r] != VB2_OK) {
                out->status = status[(size_t)r];
                return VB2_ERR_INVALID;
            }
        for (int r = 0; r < R && out->num_pair < VB2_REFBIAS_NUM_PAIR; ++r) {
            out->pair_beta[out->num_pair] = beta[(size_t)r];
            out->pair_llk1[out->num_pair] = -est[(size_t)r].llk1;
            ++out->num_pair;
        }
        out->num_refit += R;
        return VB2_OK;
    };

    // round 0: the nine values 0.25 + j / 16
    int idx[9], step = kUnits / 16;
    double l[9];
    std::vector<double> beta(9);
    for (int j = 0; j < 9; ++j) beta[(size_t)j] = beta_of(idx[j] = j * step);
    if (const int rc = run(beta)) return rc;
    for (int j = 0; j < 9; ++j) l[j] = -est[(size_t)j].llk1;
    out->llk1_at_half = l[4];
    out->alpha_at_half = est[4].alpha;
    out->num_round = 1;
    // three refinements: nine values between the best value's neighbours, six of them new
    static const int kNew[6] = {1, 2, 3, 5, 6, 7};
    for (int round = 1; round <= 3; ++round) {
        const int c = std::min(std::max(best_of(l, 9), 1), 7);
        const int lo = idx[c - 1];
        const double keep[3] = {l[c - 1], l[c], l[c + 1]};
        step /= 4;
        for (int i = 0; i < 9; ++i) idx[i] = lo + i * step;
        l[0] = keep[0], l[4] = keep[1], l[8] = keep[2];
        beta.resize(6);
        for (int i = 0; i < 6; ++i) beta[(size_t)i] = beta_of(idx[kNew[i]]);
        if (const int rc = run(beta)) return rc;
        for (int i = 0; i < 6; ++i) l[kNew[i]] = -est[(size_t)i].llk1;
        out->num_round = round + 1;
    }
    // the vertex through the best value and its neighbours (spacing 2^-10); the curvature through the ends and the centre
    // (2^-8): the searches leave about 1e-3 nats of noise on every value, which the narrow triple's second difference --
    // a tenth of a nat at a standard error of 0.003 -- would carry into the standard error
    const int b = best_of(l, 9);
    const double h = (double)step / (double)kUnits;
    double bhat = beta_of(idx[b]);
    if (b == 0 || b == 8) {
        out->at_bound = (idx[b] == 0 || idx[b] == kUnits / 2) ? 1 : 0;
    } else {
        const double d2 = l[b - 1] - 2.0 * l[b] + l[b + 1];
        if (d2 < 0.0) bhat += 0.5 * h * (l[b - 1] - l[b + 1]) / d2;
        bhat = std::min(std::max(bhat, beta_of(idx[b - 1])), beta_of(idx[b + 1]));
    }
    const double curv = (l[0] - 2.0 * l[4] + l[8]) / (16.0 * h * h);
    out->beta = bhat;
    out->beta_se = curv < 0.0 ? std::sqrt(-1.0 / curv) : NAN;
    // the final search at the estimate
    beta.assign(1, bhat);
    if (const int rc = run(beta)) return rc;
    out->alpha_bias = est[0].alpha;
    out->llk1_bias = -est[0].llk1;
    std::memcpy(out->pc, est[0].pc, sizeof(out->pc));
    std::memcpy(out->pc2, est[0].pc2, sizeof(out->pc2));
    out->lrt = 2.0 * (out->llk1_bias - out->llk1_at_half);
    return VB2_OK;
}

namespace {
// the evaluator of refbias_fit on a context: one set per lock-step call, made when the call's rows change
struct CtxEval {
    Context* ctx;
    std::unique_ptr<RefBias> set;
    std::vector<double> beta;
};
int ctx_eval(void* user, int32_t num_row, const int32_t* num_point, const double* beta, const double* pc1, const double* pc2,
             const double* alpha, double* llk)
{
    CtxEval* e = static_cast<CtxEval*>(user);
    if (!e->set || (int)e->beta.size() != num_row || std::memcmp(e->beta.data(), beta, sizeof(double) * (size_t)num_row) != 0) {
        e->set.reset();
        RefBias* s = nullptr;
        if (const int rc = RefBias::create(e->ctx, num_row, beta, &s)) return rc;
        e->set.reset(s);
        e->beta.assign(beta, beta + num_row);
    }
    return e->set->eval(num_point, pc1, pc2, alpha, llk);
}
}  // namespace

int refbias_fit_ctx(Context* ctx, const vb2_model& model, vb2_refbias_fit* out)
{
    if (ctx->resident_active) {
        set_error("vb2_refbias_fit_ctx: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    CtxEval e{ctx, nullptr, {}};
    return refbias_fit(ctx_eval, &e, ctx->num_pc, model, ctx->L.known_af != nullptr, out);
}

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

extern "C" {

int vb2_refbias_create(vb2_ctx* ctx, int32_t num_row, const double* beta, vb2_refbias** out)
{
    if (!out) {
        set_error("vb2_refbias_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (!ctx || !ctx->impl) {
        set_error("null vb2_ctx");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::RefBias* b = nullptr;
        if (const int rc = vb2::RefBias::create(ctx->impl, num_row, beta, &b)) return rc;
        *out = new vb2_refbias{b};
        return VB2_OK;
    });
}

void vb2_refbias_destroy(vb2_refbias* set)
{
    if (!set) return;
    delete set->impl;
    delete set;
}

int vb2_refbias_eval(vb2_refbias* set, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                     double* llk_out)
{
    if (!set || !set->impl) {
        set_error("null vb2_refbias");
        return VB2_ERR_INVALID;
    }
    return set->impl->eval(num_point, pc1, pc2, alpha, llk_out);
}

int vb2_refbias_optimize_llk(vb2_refbias* set, const vb2_model* model, vb2_estimate* est_out, int32_t* status)
{
    if (!set || !set->impl || !model) {
        set_error("vb2_refbias_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int { return set->impl->optimize(*model, est_out, status); });
}

int vb2_debug_refbias_time(vb2_refbias* set, int32_t num_point, int32_t warmup, int32_t reps, double* ms)
{
    if (!set || !set->impl) return VB2_ERR_INVALID;
    return set->impl->time_launch(num_point, warmup, reps, ms);
}

int vb2_refbias_info_get(const vb2_refbias* set, vb2_refbias_info* info)
{
    if (!set || !set->impl || !info) return VB2_ERR_INVALID;
    const vb2::RefBias& b = *set->impl;
    info->num_row = b.num_row;
    info->num_marker = b.ctx->num_marker;
    info->device_bytes = b.device_bytes;
    info->num_step = b.num_step();
    info->num_launch = b.num_launch();
    return VB2_OK;
}

int vb2_refbias_fit_ctx(vb2_ctx* ctx, const vb2_model* model, vb2_refbias_fit* out)
{
    if (!ctx || !ctx->impl || !model || !out) {
        set_error("vb2_refbias_fit_ctx: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int { return vb2::refbias_fit_ctx(ctx->impl, *model, out); });
}

int vb2_refbias_lockstep(vb2_refbias_eval_fn fn, void* user, int32_t num_pc, const vb2_model* model, int32_t data_has_known_af,
                         vb2_refbias_fit* out)
{
    if (!fn || !model || !out || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_refbias_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int { return vb2::refbias_fit(fn, user, num_pc, *model, data_has_known_af != 0, out); });
}

int vb2_run_refbias(const vb2_run_args* args, vb2_run_result* out, vb2_refbias_fit* fit)
{
    if (!args || !out) {
        set_error("vb2_run_refbias: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (args->devices && args->num_device > 1) {
        set_error("--RefBias takes one device: it cannot be combined with marker shards over several --Devices");
        return VB2_ERR_INVALID;
    }
    if (args->model.is_alpha_fixed) {
        set_error("--RefBias cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate");
        return VB2_ERR_INVALID;
    }
    vb2_refbias_fit f;
    std::memset(&f, 0, sizeof(f));
    vb2::RunStage stage;
    stage.on_context = [&](vb2_ctx* ctx, const vb2_flat& flat, const vb2_model& model, const vb2_estimate& whole) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        if (const int rc = vb2::refbias_fit_ctx(ctx->impl, model, &f)) return rc;
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double freemix = whole.alpha < 0.5 ? whole.alpha : 1 - whole.alpha;
        const double freemix_bias = f.alpha_bias < 0.5 ? f.alpha_bias : 1 - f.alpha_bias;
        if (args->output_prefix) {
            const int rc = vb2::write_text_file(std::string(args->output_prefix) + ".RefBias", [&](std::ostream& fout) {
                fout << "#SEQ_ID\tFREEMIX\tFREEMIX_BIAS\tREF_BIAS\tREF_BIAS_SE\tLRT\tFREELK1_BIAS\tFREELK1_HALF\tAT_BOUND\n";
                fout << flat.viewer.SEQ_SM << "\t" << freemix << "\t" << freemix_bias << "\t" << f.beta << "\t";
                if (f.beta_se == f.beta_se) fout << f.beta_se;
                else fout << "NA";
                fout << "\t" << f.lrt << "\t" << f.llk1_bias << "\t" << f.llk1_at_half << "\t" << f.at_bound << "\n";
            });
            if (rc) return rc;
        }
        std::fprintf(stderr, "NOTICE - REF_BIAS %g (SE %g), LRT %g against 0.5; FREEMIX %g with the bias fitted, %g at 0.5%s  [%d searches, "
                             "%lld lock-step steps, %.3f seconds]\n", f.beta, f.beta_se, f.lrt, freemix_bias, freemix,
                     f.at_bound ? "; the estimate lies on the domain's bound" : "", (int)f.num_refit, (long long)f.num_step, seconds);
        return VB2_OK;
    };
    return guarded([&] {
        const int rc = vb2::run_sample(args, out, stage);
        if (fit) *fit = f;
        return rc;
    });
}

}  // extern "C"
