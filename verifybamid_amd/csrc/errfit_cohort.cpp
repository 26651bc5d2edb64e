// errfit_cohort.cpp -- the error-rate fit of a cohort (errfit_cohort.h): the procedure and its two
// drivers, the device and a caller's callbacks.
#include "errfit_cohort.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "context.h"
#include "errfit.h"
#include "errstat.h"
#include "estimator.h"
#include "guard.h"

namespace vb2 {

namespace {

constexpr int kQ = VB2_ERR_NUM_QUAL;

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int errfit_cohort(const ErrFitCohortSteps& steps, int num_sample, int num_pc, const vb2_model& model, bool data_has_known_af,
                  const vb2_estimate* nominal, const int32_t* enter, const vb2_errfit_opts* opts, bool pooled, const char* who,
                  vb2_errfit* fits, vb2_errfit_pool* pool)
{
    const int S = num_sample, k = num_pc;
    std::memset(pool, 0, sizeof(*pool));
    pool->lrt_sum = NAN;
    pool->pooled = pooled ? 1 : 0;
    pool->num_sample = S;
    for (int i = 0; i < S; ++i) {
        std::memset(&fits[i], 0, sizeof(vb2_errfit));
        fits[i].llk_fit = fits[i].llk_nominal = fits[i].alpha_nominal = fits[i].lrt = NAN;
    }
    double kappa = 0.0, tol = 0.0;
    int max_iter = 0;
    if (const int rc = errfit_options(model, opts, who, &kappa, &tol, &max_iter)) return rc;
    const bool heter = model.is_heter && !model.is_af_known && !data_has_known_af;

    double eps0[kQ], pool_eps[kQ], pool_next[kQ], pool_s[kQ];
    int64_t pool_n[kQ];
    errfit_nominal_table(eps0);
    std::memcpy(pool_eps, eps0, sizeof(eps0));
    std::vector<double> eps((size_t)S * kQ), next((size_t)S * kQ), s((size_t)S * kQ), p1((size_t)S * k), p2((size_t)S * k), alpha(S);
    std::vector<double> change(S);
    std::vector<int64_t> n((size_t)S * kQ);
    std::vector<vb2_estimate> est(S), found(S);
    std::vector<int32_t> fitting(S), status(S);
    int num_fitting = 0;
    for (int i = 0; i < S; ++i) {
        std::memcpy(&eps[(size_t)i * kQ], eps0, sizeof(eps0));
        fits[i].status = enter ? enter[i] : VB2_OK;
        fitting[i] = fits[i].status == VB2_OK ? 1 : 0;
        if (!fitting[i]) continue;
        est[i] = nominal[i];
        fits[i].llk_nominal = -nominal[i].llk1;
        fits[i].alpha_nominal = nominal[i].alpha;
        ++num_fitting;
    }
    pool->num_entered = num_fitting;
    const auto points = [&](const int32_t* who_is) {
        for (int i = 0; i < S; ++i) {
            if (!who_is[i]) continue;
            errfit_search_point(est[i], k, heter, &p1[(size_t)i * k], &p2[(size_t)i * k]);
            alpha[i] = est[i].alpha;
        }
    };

    for (int t = 0; t < max_iter && num_fitting > 0; ++t) {
        points(fitting.data());
        if (const int rc = steps.stats(fitting.data(), eps.data(), p1.data(), p2.data(), alpha.data(), n.data(), s.data())) return rc;
        ++pool->num_estep;
        double pool_change = 0.0;
        if (pooled) {
            // N in integers; the samples' expected errors added in list order
            std::memset(pool_n, 0, sizeof(pool_n));
            for (int q = 0; q < kQ; ++q) pool_s[q] = 0.0;
            for (int i = 0; i < S; ++i) {
                if (!fitting[i]) continue;
                for (int q = 0; q < kQ; ++q) {
                    pool_n[q] += n[(size_t)i * kQ + q];
                    pool_s[q] += s[(size_t)i * kQ + q];
                }
            }
            pool_change = errfit_mstep(pool_n, pool_s, eps0, pool_eps, kappa, pool_next);
            for (int i = 0; i < S; ++i)
                if (fitting[i]) std::memcpy(&next[(size_t)i * kQ], pool_next, sizeof(pool_next));
        } else {
            for (int i = 0; i < S; ++i)
                if (fitting[i])
                    change[i] = errfit_mstep(&n[(size_t)i * kQ], &s[(size_t)i * kQ], eps0, &eps[(size_t)i * kQ], kappa, &next[(size_t)i * kQ]);
        }
        for (int i = 0; i < S; ++i) status[i] = VB2_OK;
        if (const int rc = steps.search(fitting.data(), next.data(), found.data(), status.data())) return rc;
        for (int i = 0; i < S; ++i) {
            if (!fitting[i]) continue;
            vb2_errfit& f = fits[i];
            if (status[i] != VB2_OK) {                     // it leaves with its code and is in no later sum
                f.status = status[i];
                fitting[i] = 0;
                --num_fitting;
                continue;
            }
            est[i] = found[i];
            std::memcpy(&eps[(size_t)i * kQ], &next[(size_t)i * kQ], sizeof(eps0));
            f.iter_llk[t] = -est[i].llk1;
            f.iter_change[t] = pooled ? pool_change : change[i];
            f.iter_alpha[t] = est[i].alpha;
            for (int q = 0; q < kQ; ++q) f.iter_err[t][q] = (float)eps[(size_t)i * kQ + q];
            f.num_step += est[i].num_eval;
            f.num_iter = t + 1;
            pool->num_step += est[i].num_eval;
            if (!pooled && change[i] <= tol) {
                f.converged = 1;
                fitting[i] = 0;
                --num_fitting;
            }
        }
        pool->num_iter = t + 1;
        if (pooled) {
            std::memcpy(pool_eps, pool_next, sizeof(pool_eps));
            pool->iter_change[t] = pool_change;
            for (int q = 0; q < kQ; ++q) pool->iter_err[t][q] = (float)pool_eps[q];
            if (pool_change <= tol) {
                pool->converged = 1;
                break;
            }
        }
    }

    // the report: one more E-step of every sample that entered and did not fail, at its final estimate and table
    std::vector<int32_t> report(S);
    int num_report = 0;
    for (int i = 0; i < S; ++i) {
        report[i] = (!enter || enter[i] == VB2_OK) && fits[i].status == VB2_OK ? 1 : 0;
        num_report += report[i];
    }
    pool->num_fitted = num_report;
    std::memcpy(pool->err, pool_eps, sizeof(pool_eps));
    if (num_report > 0) {
        points(report.data());
        if (const int rc = steps.stats(report.data(), eps.data(), p1.data(), p2.data(), alpha.data(), n.data(), s.data())) return rc;
        ++pool->num_estep;
    }
    pool->lrt_sum = 0.0;
    bool all_converged = num_report > 0;
    for (int i = 0; i < S; ++i) {
        if (!report[i]) continue;
        vb2_errfit& f = fits[i];
        std::memcpy(f.n, &n[(size_t)i * kQ], sizeof(f.n));
        std::memcpy(f.s, &s[(size_t)i * kQ], sizeof(f.s));
        std::memcpy(f.err, &eps[(size_t)i * kQ], sizeof(f.err));
        f.est = est[i];
        f.llk_fit = -est[i].llk1;
        f.lrt = 2.0 * (f.llk_fit - f.llk_nominal);
        if (pooled) f.converged = pool->converged;
        all_converged = all_converged && f.converged;
        for (int q = 0; q < kQ; ++q) {
            f.num_bin += f.n[q] > 0 ? 1 : 0;
            pool->n[q] += f.n[q];
            pool->s[q] += f.s[q];
        }
        pool->lrt_sum += f.lrt;
    }
    if (!pooled) pool->converged = all_converged ? 1 : 0;
    for (int q = 0; q < kQ; ++q) pool->num_bin += pool->n[q] > 0 ? 1 : 0;
    return VB2_OK;
}

namespace {

struct BatchDelete {
    void operator()(ErrStatBatch* e) const { delete e; }
};

// contexts of the live samples under their tables, made on up to eight host threads; status [i]: the code of a sample whose
// context could not be made
void create_contexts(const vb2_input* const* in, int S, const vb2_options& opt, const int32_t* live, const double* err,
                     std::vector<vb2_ctx*>& ctx, int32_t* status, std::string* first_error)
{
    std::vector<int> todo;
    for (int i = 0; i < S; ++i)
        if (live[i]) todo.push_back(i);
    std::atomic<size_t> nextjob{0};
    std::vector<std::string> errors(S);
    const auto work = [&] {
        for (size_t j = nextjob++; j < todo.size(); j = nextjob++) {
            const int i = todo[j];
            status[i] = vb2_ctx_create_ex(in[i], &opt, err + (size_t)i * kQ, &ctx[i]);
            if (status[i]) errors[i] = g_last_error;            // (the text is the thread's own)
        }
    };
    const size_t nthr = todo.size() < 8 ? todo.size() : 8;
    std::vector<std::thread> th;
    for (size_t t = 1; t < nthr; ++t) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
    for (int i = 0; i < S; ++i)
        if (status[i] && first_error->empty()) *first_error = errors[i];
}

}  // namespace

int errfit_cohort_inputs(const vb2_input* const* in, int num_sample, const vb2_options* opt, const vb2_model& model,
                         const vb2_estimate* nominal, const int32_t* enter, const vb2_errfit_opts* opts, bool pooled,
                         vb2_errfit* fits, vb2_errfit_pool* pool)
{
    const char* who = "vb2_errfit_cohort_inputs";
    const int S = num_sample;
    int k = 0;
    bool kaf = false;
    std::vector<const vb2_input*> held(S, nullptr);
    for (int i = 0; i < S; ++i) {
        if (enter && enter[i] != VB2_OK) continue;             // (its input may be anything: it never enters)
        if (!in[i] || in[i]->num_pc < 1 || in[i]->num_pc > VB2_MAX_PC) {
            set_error(std::string(who) + ": invalid input");
            return VB2_ERR_INVALID;
        }
        const bool has = in[i]->known_af != nullptr;
        if (k != 0 && (in[i]->num_pc != k || has != kaf)) {
            set_error(std::string(who) + ": the samples of a cohort have one num_pc, and known allele frequencies all or none");
            return VB2_ERR_INVALID;
        }
        k = in[i]->num_pc;
        kaf = has;
        held[i] = in[i];
    }
    if (k == 0) k = 1;                                          // nobody enters: the procedure still fills the records
    ErrStatBatch* made = nullptr;
    if (const int rc = ErrStatBatch::create(held.data(), S, opt, &made)) return rc;
    std::unique_ptr<ErrStatBatch, BatchDelete> set(made);
    vb2_options copt{};
    copt.device = set->device;
    copt.flags = VB2_OPT_COHORT_LAYOUT;
    vb2_model quiet = model;
    quiet.notices = 0;
    quiet.verbose = 0;
    double t_stats = 0.0, t_ctx = 0.0, t_search = 0.0;
    ErrFitCohortSteps steps;
    steps.stats = [&](const int32_t* live, const double* err, const double* pc1, const double* pc2, const double* alpha,
                      int64_t* n, double* s) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = set->eval(live, err, pc1, pc2, alpha, n, s, nullptr);
        t_stats += seconds_since(t0);
        return rc;
    };
    steps.search = [&](const int32_t* live, const double* err, vb2_estimate* est, int32_t* status) -> int {
        std::vector<vb2_ctx*> ctx(S, nullptr);
        struct Cleanup {
            std::vector<vb2_ctx*>& c;
            ~Cleanup()
            {
                for (vb2_ctx* x : c) vb2_ctx_destroy(x);
            }
        } cleanup{ctx};
        auto t0 = std::chrono::steady_clock::now();
        std::string first_error;
        create_contexts(held.data(), S, copt, live, err, ctx, status, &first_error);
        if (!first_error.empty()) set_error(first_error);       // (why the first sample left, on the caller's thread)
        t_ctx += seconds_since(t0);
        std::vector<vb2_ctx*> gang;
        std::vector<int> who_is;
        for (int i = 0; i < S; ++i)
            if (live[i] && status[i] == VB2_OK) {
                gang.push_back(ctx[i]);
                who_is.push_back(i);
            }
        if (gang.empty()) return VB2_OK;
        t0 = std::chrono::steady_clock::now();
        vb2_batch* b = nullptr;
        if (const int rc = vb2_batch_create(gang.data(), (int32_t)gang.size(), &b)) return rc;
        std::vector<vb2_estimate> out(gang.size());
        const int rc = vb2_batch_optimize_llk(b, &quiet, 1, out.data());
        vb2_batch_destroy(b);
        // the gang has one code: where it fails, every sample of the gang leaves with it (the lock-step search cannot say
        // whose it is); samples outside the gang go on
        if (rc)
            for (size_t j = 0; j < gang.size(); ++j) status[who_is[j]] = rc;
        t_search += seconds_since(t0);
        for (size_t j = 0; j < gang.size(); ++j)
            if (status[who_is[j]] == VB2_OK) est[who_is[j]] = out[j];
        return VB2_OK;
    };
    const int rc = errfit_cohort(steps, S, k, model, kaf, nominal, enter, opts, pooled, who, fits, pool);
    pool->seconds_stats = t_stats;
    pool->seconds_context = t_ctx;
    pool->seconds_search = t_search;
    pool->device_bytes = set->device_bytes;
    return rc;
}

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

extern "C" {

int vb2_errfit_cohort_inputs(const vb2_input* const* in, int32_t num_sample, const vb2_options* opt, const vb2_model* model,
                             const vb2_estimate* nominal, const int32_t* enter_status, const vb2_errfit_opts* fit_opts,
                             int32_t pooled, vb2_errfit* fits, vb2_errfit_pool* pool)
{
    if (!in || !model || !nominal || !fits || !pool || num_sample < 1 || num_sample > VB2_ERRSTAT_BATCH_MAX) {
        set_error("vb2_errfit_cohort_inputs: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (model->is_alpha_fixed) {                // (before a device is looked for)
        set_error("vb2_errfit_cohort_inputs: a fixed alpha leaves the fit nothing to tell errors from (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    return guarded([&] {
        return vb2::errfit_cohort_inputs(in, num_sample, opt, *model, nominal, enter_status, fit_opts, pooled != 0, fits, pool);
    });
}

int vb2_errfit_cohort_lockstep(const vb2_errfit_cohort_fns* fns, void* user, int32_t num_sample, int32_t num_pc,
                               const vb2_model* model, int32_t data_has_known_af, const vb2_estimate* nominal,
                               const int32_t* enter_status, const vb2_errfit_opts* fit_opts, int32_t pooled, vb2_errfit* fits,
                               vb2_errfit_pool* pool)
{
    if (!fns || !fns->eval || !fns->stats || !model || !nominal || !fits || !pool || num_pc < 1 || num_pc > VB2_MAX_PC ||
        num_sample < 1 || num_sample > VB2_ERRSTAT_BATCH_MAX) {
        set_error("vb2_errfit_cohort_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        // a sample's search: the caller's evaluator with the sample and its table in front
        struct Bound {
            const vb2_errfit_cohort_fns* fns;
            void* user;
            int32_t sample;
            const double* err;
        };
        const vb2_eval_fn eval = [](void* u, int32_t n, const double* pc1, const double* pc2, const double* alpha, double* llk) {
            const Bound* b = static_cast<const Bound*>(u);
            return b->fns->eval(b->user, b->sample, b->err, n, pc1, pc2, alpha, llk);
        };
        vb2::ErrFitCohortSteps steps;
        steps.stats = [&](const int32_t* live, const double* err, const double* pc1, const double* pc2, const double* alpha,
                          int64_t* n, double* s) -> int {
            const int rc = fns->stats(user, num_sample, live, err, pc1, pc2, alpha, n, s);
            if (rc) set_error("vb2_errfit_cohort_lockstep: the statistics callback failed");
            return rc;
        };
        steps.search = [&](const int32_t* live, const double* err, vb2_estimate* est_out, int32_t* status) -> int {
            for (int32_t i = 0; i < num_sample; ++i) {
                if (!live[i]) continue;
                Bound bound{fns, user, i, err + (size_t)i * VB2_ERR_NUM_QUAL};
                vb2::Estimator est(num_pc, eval, &bound);
                vb2::apply_model(est, *model, data_has_known_af != 0);
                est.notices = false;
                est.verbose = false;
                status[i] = est.OptimizeLLK();
                if (status[i] == VB2_OK) vb2::fill_estimate(est, &est_out[i]);
            }
            return VB2_OK;
        };
        return vb2::errfit_cohort(steps, num_sample, num_pc, *model, data_has_known_af != 0, nominal, enter_status, fit_opts,
                                  pooled != 0, "vb2_errfit_cohort_lockstep", fits, pool);
    });
}

}  // extern "C"
