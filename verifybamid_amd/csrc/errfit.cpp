// errfit.cpp -- empirical base-error rates fitted jointly with FREEMIX (errfit.h): the procedure, its
// two drivers (the device; a caller's callbacks) and the file flow behind --FitError.
#include "errfit.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "context.h"
#include "err_table.h"
#include "errstat.h"
#include "estimator.h"
#include "guard.h"
#include "hostio.h"
#include "run.h"

namespace vb2 {

namespace {

constexpr int kQ = VB2_ERR_NUM_QUAL;

}  // namespace

void errfit_search_point(const vb2_estimate& est, int k, bool heter, double* p1, double* p2)
{
    std::memcpy(p1, est.pc, sizeof(double) * (size_t)k);
    std::memcpy(p2, est.pc2, sizeof(double) * (size_t)k);
    if (heter && est.alpha >= 0.5) {
        std::swap(p1[0], p2[0]);
        if (k >= 2) std::swap(p1[1], p2[1]);
    }
}

int errfit_options(const vb2_model& model, const vb2_errfit_opts* opts, const char* who, double* kappa_out, double* tol_out,
                   int* max_iter_out)
{
    const std::string w(who);
    if (model.is_alpha_fixed) {
        set_error(w + ": a fixed alpha leaves the fit nothing to tell errors from (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    const double kappa = opts && opts->prior_reads != 0.0 ? opts->prior_reads : 100.0;
    const double tol = opts && opts->tol != 0.0 ? opts->tol : 1e-4;
    const int max_iter = opts && opts->max_iter != 0 ? opts->max_iter : VB2_ERRFIT_MAX_ITER;
    if (!(kappa > 0.0) || !(tol > 0.0) || max_iter < 1 || max_iter > VB2_ERRFIT_MAX_ITER) {
        set_error(w + ": prior_reads and tol are positive (0 = the defaults 100 and 1e-4), max_iter is 1.." +
                  std::to_string(VB2_ERRFIT_MAX_ITER) + " (0 = " + std::to_string(VB2_ERRFIT_MAX_ITER) + ")");
        return VB2_ERR_INVALID;
    }
    *kappa_out = kappa;
    *tol_out = tol;
    *max_iter_out = max_iter;
    return VB2_OK;
}

void errfit_nominal_table(double* eps0)
{
    for (int q = 0; q < kQ; ++q) eps0[q] = std::pow(10.0, q / -10.0);
}

double errfit_mstep(const int64_t* n, const double* s, const double* eps0, const double* eps, double kappa, double* next)
{
    double change = 0.0;
    for (int q = 0; q < kQ; ++q) {
        next[q] = eps0[q];
        if (n[q] <= 0) continue;
        // the posterior mode's share of error reads among n + kappa, kept as the nearest float32: the device fit and the
        // restatement continue from the same bits
        next[q] = (double)(float)((s[q] + kappa * eps0[q]) / ((double)n[q] + kappa));
        const double d = eps[q] > 0.0 ? std::fabs(next[q] - eps[q]) / eps[q] : (next[q] == 0.0 ? 0.0 : INFINITY);
        change = d > change ? d : change;
    }
    return change;
}

int errfit(const ErrFitSteps& steps, int num_pc, const vb2_model& model, bool data_has_known_af, const vb2_estimate& nominal,
           const vb2_errfit_opts* opts, const char* who, vb2_errfit* out)
{
    std::memset(out, 0, sizeof(*out));
    out->llk_fit = out->llk_nominal = out->alpha_nominal = out->lrt = NAN;
    double kappa = 0.0, tol = 0.0;
    int max_iter = 0;
    if (const int rc = errfit_options(model, opts, who, &kappa, &tol, &max_iter)) return rc;
    const bool heter = model.is_heter && !model.is_af_known && !data_has_known_af;
    double eps0[kQ], eps[kQ], next[kQ], p1[VB2_MAX_PC], p2[VB2_MAX_PC];
    errfit_nominal_table(eps0);
    std::memcpy(eps, eps0, sizeof(eps));
    vb2_estimate est = nominal;
    out->llk_nominal = -nominal.llk1;
    out->alpha_nominal = nominal.alpha;
    vb2_model quiet = model;                   // (the reference's phase lines belong to the run's own search)
    quiet.notices = 0;
    quiet.verbose = 0;
    for (int t = 0; t < max_iter; ++t) {
        errfit_search_point(est, num_pc, heter, p1, p2);
        if (const int rc = steps.stats(eps, p1, p2, est.alpha, out->n, out->s)) return rc;
        const double change = errfit_mstep(out->n, out->s, eps0, eps, kappa, next);
        if (const int rc = steps.search(next, &est)) {
            out->status = rc;
            return rc;
        }
        std::memcpy(eps, next, sizeof(eps));
        out->iter_llk[t] = -est.llk1;
        out->iter_change[t] = change;
        out->iter_alpha[t] = est.alpha;
        for (int q = 0; q < kQ; ++q) out->iter_err[t][q] = (float)eps[q];
        out->num_step += est.num_eval;
        out->num_iter = t + 1;
        if (change <= tol) {
            out->converged = 1;
            break;
        }
    }
    errfit_search_point(est, num_pc, heter, p1, p2);
    if (const int rc = steps.stats(eps, p1, p2, est.alpha, out->n, out->s)) return rc;
    std::memcpy(out->err, eps, sizeof(eps));
    out->est = est;
    out->llk_fit = -est.llk1;
    out->lrt = 2.0 * (out->llk_fit - out->llk_nominal);
    for (int q = 0; q < kQ; ++q) out->num_bin += out->n[q] > 0 ? 1 : 0;
    return VB2_OK;
}

int write_error_rates(const std::string& prefix, const double* err, const int64_t* n, const double* s)
{
    return write_text_file(prefix + ".ErrorRates", [&](std::ostream& fout) {
        fout << "#Q_REPORTED\tREADS\tEXPECTED_ERRORS\tERROR_RATE\tQ_EMPIRICAL\tSE_BINOM\n";
        for (int q = 0; q < VB2_ERR_NUM_QUAL; ++q) {
            if (n[q] <= 0) continue;
            const double e = err[q];
            fout << q << "\t" << (long long)n[q] << "\t" << s[q] << "\t" << e << "\t" << -10.0 * std::log10(e) << "\t"
                 << std::sqrt(e * (1.0 - e) / (double)n[q]) << "\n";
        }
    });
}

int write_errfit_files(const std::string& prefix, const std::string& seq_id, double freemix, const vb2_errfit& f)
{
    const double freemix_fit = f.est.alpha < 0.5 ? f.est.alpha : 1 - f.est.alpha;
    const int rc = write_text_file(prefix + ".ErrorFit", [&](std::ostream& fout) {
        fout << "#SEQ_ID\tFREEMIX\tFREEMIX_FIT\tLRT\tNUM_BIN\tFREELK1_FIT\tFREELK1_NOMINAL\tITERATIONS\tCONVERGED\n";
        fout << seq_id << "\t" << freemix << "\t" << freemix_fit << "\t" << f.lrt << "\t" << f.num_bin << "\t" << f.llk_fit << "\t"
             << f.llk_nominal << "\t" << f.num_iter << "\t" << f.converged << "\n";
    });
    return rc ? rc : write_error_rates(prefix, f.err, f.n, f.s);
}

namespace {
struct ErrStatDelete {
    void operator()(ErrStat* e) const { delete e; }
};
struct CtxDestroy {
    void operator()(vb2_ctx* c) const { vb2_ctx_destroy(c); }
};
}  // namespace

int errfit_input(const vb2_input* in, const vb2_options* opt, const vb2_model& model, const vb2_estimate& nominal,
                 const vb2_errfit_opts* opts, vb2_errfit* out)
{
    ErrStat* made = nullptr;
    if (const int rc = ErrStat::create(in, opt, &made)) return rc;
    std::unique_ptr<ErrStat, ErrStatDelete> set(made);
    ErrFitSteps steps;
    steps.stats = [&](const double* err, const double* pc1, const double* pc2, double alpha, int64_t* n, double* s) {
        return set->eval(err, pc1, pc2, alpha, n, s, nullptr);
    };
    steps.search = [&](const double* err, vb2_estimate* est) -> int {
        vb2_ctx* created = nullptr;
        if (const int rc = vb2_ctx_create_ex(in, opt, err, &created)) return rc;
        std::unique_ptr<vb2_ctx, CtxDestroy> ctx(created);
        vb2_model m = model;
        m.notices = 0;
        m.verbose = 0;
        return vb2_ctx_optimize_llk(ctx.get(), &m, est, nullptr);
    };
    return errfit(steps, in->num_pc, model, in->known_af != nullptr, nominal, opts, "vb2_errfit_input", out);
}

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

extern "C" {

int vb2_ctx_create_ex(const vb2_input* in, const vb2_options* opt, const double* err_table, vb2_ctx** out)
{
    if (!out) {
        set_error("vb2_ctx_create_ex: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return guarded([&]() -> int {
        vb2::Context* c = nullptr;
        if (const int rc = vb2::Context::create(in, opt, &c, err_table)) return rc;
        *out = new vb2_ctx{c};
        return VB2_OK;
    });
}

int vb2_errfit_input(const vb2_input* in, const vb2_options* opt, const vb2_model* model, const vb2_estimate* nominal,
                     const vb2_errfit_opts* fit_opts, vb2_errfit* out)
{
    if (!in || !model || !nominal || !out || in->num_pc < 1 || in->num_pc > VB2_MAX_PC) {
        set_error("vb2_errfit_input: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (model->is_alpha_fixed) {                // (before a device is looked for)
        set_error("vb2_errfit_input: a fixed alpha leaves the fit nothing to tell errors from (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    return guarded([&] { return vb2::errfit_input(in, opt, *model, *nominal, fit_opts, out); });
}

int vb2_errfit_lockstep(const vb2_errfit_fns* fns, void* user, int32_t num_pc, const vb2_model* model, int32_t data_has_known_af,
                        const vb2_estimate* nominal, const vb2_errfit_opts* fit_opts, vb2_errfit* out)
{
    if (!fns || !fns->eval || !fns->stats || !model || !nominal || !out || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_errfit_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        // the search's evaluator: the caller's, with the iteration's table in front
        struct Bound {
            const vb2_errfit_fns* fns;
            void* user;
            const double* err;
        } bound{fns, user, nullptr};
        const vb2_eval_fn eval = [](void* u, int32_t n, const double* pc1, const double* pc2, const double* alpha, double* llk) {
            const Bound* b = static_cast<const Bound*>(u);
            return b->fns->eval(b->user, b->err, n, pc1, pc2, alpha, llk);
        };
        vb2::ErrFitSteps steps;
        steps.stats = [&](const double* err, const double* pc1, const double* pc2, double alpha, int64_t* n, double* s) -> int {
            const int rc = fns->stats(user, err, pc1, pc2, alpha, n, s);
            if (rc) set_error("vb2_errfit_lockstep: the statistics callback failed");
            return rc;
        };
        steps.search = [&](const double* err, vb2_estimate* est_out) -> int {
            bound.err = err;
            vb2::Estimator est(num_pc, eval, &bound);
            vb2::apply_model(est, *model, data_has_known_af != 0);
            est.notices = false;
            est.verbose = false;
            if (const int rc = est.OptimizeLLK()) return rc;
            vb2::fill_estimate(est, est_out);
            return VB2_OK;
        };
        return vb2::errfit(steps, num_pc, *model, data_has_known_af != 0, *nominal, fit_opts, "vb2_errfit_lockstep", out);
    });
}

int vb2_err_table_read(const char* path, double* err_table, int32_t* num_taken)
{
    if (num_taken) *num_taken = 0;
    if (!path || !err_table) {
        set_error("vb2_err_table_read: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        std::string error;
        int taken = 0;
        if (!vb2::read_err_table(path, err_table, &taken, &error)) {
            set_error(error);
            return VB2_ERR_INVALID;
        }
        if (num_taken) *num_taken = taken;
        return VB2_OK;
    });
}

int vb2_run_under_table(const vb2_run_args* args, const double* err_table, vb2_run_result* out)
{
    if (!args || !out) {
        set_error("vb2_run_under_table: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (!vb2::err_table_ok(err_table, "vb2_run_under_table")) return VB2_ERR_INVALID;
    if (args->devices && args->num_device > 1) {
        set_error("--ErrorTable takes one device: it cannot be combined with marker shards over several --Devices");
        return VB2_ERR_INVALID;
    }
    vb2::RunStage stage;
    stage.err_table = err_table;
    return guarded([&] { return vb2::run_sample(args, out, stage); });
}

int vb2_run_errfit(const vb2_run_args* args, const vb2_errfit_opts* fit_opts, vb2_run_result* out, vb2_errfit* fit)
{
    if (!args || !out) {
        set_error("vb2_run_errfit: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (args->devices && args->num_device > 1) {
        set_error("--FitError takes one device: it cannot be combined with marker shards over several --Devices");
        return VB2_ERR_INVALID;
    }
    if (args->model.is_alpha_fixed) {
        set_error("--FitError cannot be combined with --FixAlpha: a fixed alpha leaves the fit nothing to tell errors from");
        return VB2_ERR_INVALID;
    }
    if (args->search.num_start > 1 || args->search.line_search) {
        set_error("--FitError cannot be combined with --NumStart / --LineSearch: every iteration's search is the reference's own");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<vb2_errfit> f(new vb2_errfit());
    std::memset(f.get(), 0, sizeof(vb2_errfit));
    vb2::RunStage stage;
    stage.on_context = [&](vb2_ctx* ctx, const vb2_flat& flat, const vb2_model& model, const vb2_estimate& whole) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        vb2_options opt{};
        opt.device = ctx->impl->device;
        if (const int rc = vb2::errfit_input(&flat.input, &opt, model, whole, fit_opts, f.get())) return rc;
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double freemix = whole.alpha < 0.5 ? whole.alpha : 1 - whole.alpha;
        const double freemix_fit = f->est.alpha < 0.5 ? f->est.alpha : 1 - f->est.alpha;
        if (args->output_prefix)
            if (const int rc = vb2::write_errfit_files(args->output_prefix, flat.viewer.SEQ_SM, freemix, *f)) return rc;
        std::fprintf(stderr, "NOTICE - FREEMIX %g with the error rates of %d qualities fitted, %g at 10^(-q/10); LRT %g; %d iterations%s  "
                             "[%lld likelihood evaluations, %.3f seconds]\n", freemix_fit, (int)f->num_bin, freemix, f->lrt,
                     (int)f->num_iter, f->converged ? "" : ", not converged", (long long)f->num_step, seconds);
        return VB2_OK;
    };
    return guarded([&] {
        const int rc = vb2::run_sample(args, out, stage);
        if (fit) *fit = *f;
        return rc;
    });
}

}  // extern "C"
