// interval.cpp -- standard errors and the profile-likelihood interval for FREEMIX (vb2_ctx_interval), on the derivatives
// of the LLK the device returns (Context::derivs_host, deriv_kernels.hip).  DESIGN.md section 10.
// The interval is blocking code over an evaluator of one point's derivatives: ctx_interval hands it the context's, and
// intervals_lockstep runs one such body per sample as the fibers of a FiberGang (lockstep.h), every step's parked requests
// answered by ONE call of a batched evaluator (Batch::derivs: vb2_batch_interval; a caller's: vb2_intervals_lockstep).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "batch.h"
#include "context.h"
#include "guard.h"
#include "host_clock.h"
#include "interval.h"
#include "run.h"

namespace vb2 {
namespace {

constexpr double kHalfChi2 = 1.9207294103470620;   // chi2_1(0.95) / 2
constexpr double kZ = 1.959963984540054;           // the normal's 0.975 quantile
const double kNaN = std::numeric_limits<double>::quiet_NaN();

// The free parameters of FullLLKFunc::Unpack (estimator.cpp) as the interval sees them: u = the free PCs, then alpha as
// logit when it is free.  heter: u = pc1 (and pc2 unless --FixPC); within ancestry: u = the shared PC (none with --FixPC);
// --KnownAF: the one-parameter model of alpha alone.
struct Free {
    int k = 0, nu = 0;
    bool heter = false, shared = false, pc2_free = false, alpha_free = false;
    bool one_side = false, side_pc2 = false;     // a refit with one side held: u = the other side's PCs (side_pc2: pc2's)
    std::vector<double> base1, base2;            // the fixed parts: the estimate's PCs
    void unpack(const double* u, double* pc1, double* pc2) const
    {
        for (int j = 0; j < k; ++j) { pc1[j] = base1[j]; pc2[j] = base2[j]; }
        if (nu == 0) return;
        if (shared) {
            for (int j = 0; j < k; ++j) pc1[j] = pc2[j] = u[j];
        } else if (one_side) {
            for (int j = 0; j < k; ++j) (side_pc2 ? pc2 : pc1)[j] = u[j];
        } else {
            for (int j = 0; j < k; ++j) pc1[j] = u[j];
            if (pc2_free) for (int j = 0; j < k; ++j) pc2[j] = u[k + j];
        }
    }
    // full coordinate(s) of u component i: pc1[i] -> i, pc2[i] -> k + i; a shared PC is both
    int nmap(int) const { return shared ? 2 : 1; }
    int map(int i, int t) const { return shared ? (t == 0 ? i : k + i) : (one_side && side_pc2) ? k + i : i; }
};

// One point: LLK, and its derivatives in u and alpha
struct Eval {
    double f = 0, ga = 0, haa = 0;
    std::vector<double> g, h, hua;               // [nu], [nu][nu], [nu]
};

bool solve_spd(std::vector<double> A, const std::vector<double>& b, std::vector<double>* x, int n)
{
    // Cholesky A = L L^T (in place, lower), then the two triangular solves; false: A is not positive definite
    for (int j = 0; j < n; ++j) {
        double d = A[(size_t)j * n + j];
        for (int p = 0; p < j; ++p) d -= A[(size_t)j * n + p] * A[(size_t)j * n + p];
        if (!(d > 0) || !std::isfinite(d)) return false;
        d = std::sqrt(d);
        A[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double v = A[(size_t)i * n + j];
            for (int p = 0; p < j; ++p) v -= A[(size_t)i * n + p] * A[(size_t)j * n + p];
            A[(size_t)i * n + j] = v / d;
        }
    }
    x->assign(n, 0.0);
    for (int i = 0; i < n; ++i) {
        double v = b[i];
        for (int p = 0; p < i; ++p) v -= A[(size_t)i * n + p] * (*x)[p];
        (*x)[i] = v / A[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double v = (*x)[i];
        for (int p = i + 1; p < n; ++p) v -= A[(size_t)p * n + i] * (*x)[p];
        (*x)[i] = v / A[(size_t)i * n + i];
    }
    return true;
}

class Profiler {
public:
    Profiler(const DerivFn& fn, const Free& fr) : fn_(fn), fr_(fr) {}
    int eval(const std::vector<double>& u, double a, Eval* e)
    {
        const int k = fr_.k, n = 2 * k + 1, nu = fr_.nu;
        std::vector<double> pc1(k > 0 ? k : 1), pc2(k > 0 ? k : 1), grad(n), hess((size_t)n * n);
        fr_.unpack(u.data(), pc1.data(), pc2.data());
        double llk = 0;
        if (int rc = fn_(pc1.data(), pc2.data(), a, &llk, grad.data(), hess.data())) return rc;
        ++launches;
        e->f = llk;
        e->ga = grad[2 * k];
        e->haa = hess[(size_t)2 * k * n + 2 * k];
        e->g.assign(nu, 0.0);
        e->hua.assign(nu, 0.0);
        e->h.assign((size_t)nu * nu, 0.0);
        for (int i = 0; i < nu; ++i)
            for (int t = 0; t < fr_.nmap(i); ++t) {
                const int fi = fr_.map(i, t);
                e->g[i] += grad[fi];
                e->hua[i] += hess[(size_t)fi * n + 2 * k];
                for (int j = 0; j < nu; ++j)
                    for (int s = 0; s < fr_.nmap(j); ++s) e->h[(size_t)i * nu + j] += hess[(size_t)fi * n + fr_.map(j, s)];
            }
        return VB2_OK;
    }
    // max over u of the LLK at alpha = a, from u (damped Newton: Levenberg-Marquardt with backtracking).  As alpha -> 0 the
    // contaminant's block of -H vanishes (exactly flat at 0): the damping is relative to the largest diagonal entry, so a
    // singular block gets no step and the rest converges.
    int maximise(double a, std::vector<double>* u, double* best)
    {
        Eval e;
        if (int rc = eval(*u, a, &e)) return rc;
        const int nu = fr_.nu;
        double lambda = 1e-3;
        for (int it = 0; it < 200 && nu > 0; ++it) {
            double dmax = 0;
            for (int i = 0; i < nu; ++i) dmax = std::max(dmax, std::fabs(e.h[(size_t)i * nu + i]));
            if (!(dmax > 0) || !std::isfinite(dmax)) break;
            std::vector<double> A((size_t)nu * nu), step;
            bool ok = false;
            while (!ok && lambda < 1e16) {
                for (int i = 0; i < nu; ++i)
                    for (int j = 0; j < nu; ++j) A[(size_t)i * nu + j] = -e.h[(size_t)i * nu + j];
                for (int i = 0; i < nu; ++i)
                    A[(size_t)i * nu + i] += lambda * std::max(std::fabs(e.h[(size_t)i * nu + i]), 1e-12 * dmax);
                ok = solve_spd(A, e.g, &step, nu);
                if (!ok) lambda *= 10;
            }
            if (!ok) break;
            double dec = 0;
            for (int i = 0; i < nu; ++i) dec += e.g[i] * step[i];
            if (!(dec > std::max(1e-11, 1e-15 * std::fabs(e.f)))) break;       // the Newton decrement: converged
            std::vector<double> un(*u);
            for (int i = 0; i < nu; ++i) un[i] += step[i];
            Eval en;
            if (int rc = eval(un, a, &en)) return rc;
            if (en.f >= e.f) {
                *u = un;
                e = en;
                lambda = std::max(lambda * 0.1, 1e-12);
            } else {
                lambda *= 10;
                if (lambda >= 1e16) break;
            }
        }
        *best = e.f;
        return VB2_OK;
    }
    int64_t launches = 0;

private:
    const DerivFn& fn_;
    const Free& fr_;
};

}  // namespace

int ctx_interval(Context* ctx, const vb2_model& model_in, const vb2_estimate& est, vb2_interval* out)
{
    const DerivFn fn = [ctx](const double* pc1, const double* pc2, double a, double* llk, double* grad, double* hess) {
        return ctx->derivs_host(1, pc1, pc2, &a, llk, grad, hess);
    };
    return interval_at(ctx->num_pc, ctx->L.known_af != nullptr, model_in, est, fn, out, nullptr);
}

int interval_at(int k, bool data_has_known_af, const vb2_model& model_in, const vb2_estimate& est, const DerivFn& fn,
                vb2_interval* out, const char* label, const IntervalOptions* opt)
{
    std::memset(out, 0, sizeof(*out));
    const IntervalOptions defaults;
    const IntervalOptions& o = opt ? *opt : defaults;
    const bool held = o.held != IntervalOptions::kNone;
    if (held && !o.fixed) {
        set_error("interval: a held side without its PCs");
        return VB2_ERR_INVALID;
    }
    const bool kaf = model_in.is_af_known != 0 || data_has_known_af;
    const std::string who = label ? std::string(label) + ": " : std::string();       // (a cohort run: whose NOTICE it is)
    const bool heter = model_in.is_heter && !kaf && !held;                         // apply_model (estimator.cpp)
    const bool pcfix = (model_in.is_pc_fixed && model_in.fix_pc) || kaf;
    const bool afix = !pcfix && model_in.is_alpha_fixed;
    const bool notices = model_in.notices != 0;
    Free fr;
    fr.k = k;
    fr.heter = heter;
    fr.shared = !heter && !pcfix && !held;
    fr.pc2_free = heter && !pcfix;
    fr.one_side = held && !pcfix;
    fr.side_pc2 = o.held == IntervalOptions::kPc1;
    fr.alpha_free = !afix;
    fr.nu = heter ? (pcfix ? k : 2 * k) : (pcfix ? 0 : k);
    // the search's own point: the reported PCs with the reference's swap of indices 0, 1 undone (estimator.cpp); a held
    // side is where it is held
    fr.base1.assign(est.pc, est.pc + k);
    fr.base2.assign(est.pc2, est.pc2 + k);
    if (held) (o.held == IntervalOptions::kPc1 ? fr.base1 : fr.base2).assign(o.fixed, o.fixed + k);
    const bool swapped = heter && est.alpha >= 0.5;
    if (swapped && k >= 1) {
        std::swap(fr.base1[0], fr.base2[0]);
        if (k >= 2) std::swap(fr.base1[1], fr.base2[1]);
    }
    std::vector<double> u0(fr.nu);
    for (int j = 0; j < fr.nu; ++j) u0[j] = (fr.one_side && fr.side_pc2) ? fr.base2[j] : j < k ? fr.base1[j] : fr.base2[j - k];
    if (!est.converged && notices)
        std::fprintf(stderr, "NOTICE - %sthe search did not converge: the interval is computed at its best point all the same\n",
                     who.c_str());

    Profiler prof(fn, fr);
    const double a_hat = est.alpha;
    out->alpha_free = fr.alpha_free ? 1 : 0;
    out->num_free = fr.nu + (fr.alpha_free ? 1 : 0);
    out->freemix = (!o.fold || a_hat < 0.5) ? a_hat : 1 - a_hat;

    // ---- standard errors: -H in the free parameters (alpha as x = logit alpha: da/dx = a(1-a), d2a/dx2 = a(1-a)(1-2a)) ----
    Eval e;
    if (int rc = prof.eval(u0, a_hat, &e)) return rc;
    const int nf = out->num_free, nu = fr.nu;
    std::vector<double> se(nf > 0 ? nf : 1, kNaN);
    {
        std::vector<double> A((size_t)nf * nf, 0.0);
        for (int i = 0; i < nu; ++i)
            for (int j = 0; j < nu; ++j) A[(size_t)i * nf + j] = -e.h[(size_t)i * nu + j];
        if (fr.alpha_free) {
            const double s = a_hat * (1 - a_hat), s2 = s * (1 - 2 * a_hat);
            for (int i = 0; i < nu; ++i) A[(size_t)i * nf + nu] = A[(size_t)nu * nf + i] = -e.hua[i] * s;
            A[(size_t)nu * nf + nu] = -(e.haa * s * s + e.ga * s2);
        }
        bool pd = nf > 0;
        for (int c = 0; c < nf && pd; ++c) {
            std::vector<double> col(nf, 0.0), x;
            col[c] = 1.0;
            pd = solve_spd(A, col, &x, nf);
            if (pd) se[c] = std::sqrt(x[c]);
        }
        out->pos_def = pd ? 1 : 0;
        if (!pd) {
            std::fill(se.begin(), se.end(), kNaN);
            if (notices && nf > 0)
                std::fprintf(stderr, "NOTICE - %sthe Hessian of the log-likelihood at the estimate is not negative definite "
                                     "(typical for FREEMIX near 0): standard errors are NA\n", who.c_str());
        }
    }
    out->freemix_se = fr.alpha_free ? a_hat * (1 - a_hat) * se[nu] : kNaN;

    // ---- profile interval for FREEMIX ----
    out->lo = out->hi = out->llk_lo = out->llk_hi = kNaN;
    out->llk_max = -est.llk1;
    if (fr.alpha_free) {
        const bool side = o.fold && a_hat >= 0.5;          // profile at alpha = 1 - f: the estimate's side
        const double f_hat = out->freemix;
        const double f_top = o.fold ? 0.5 : 1.0;           // where f ends
        struct Pt { double f, v; std::vector<double> u; };
        std::vector<Pt> pts;
        double llk_max = -est.llk1;
        auto lp = [&](double f, double* v) -> int {
            // warm start from the nearest point already profiled
            std::vector<double> u = u0;
            double dist = std::numeric_limits<double>::infinity();
            for (const Pt& p : pts)
                if (std::fabs(p.f - f) < dist) { dist = std::fabs(p.f - f); u = p.u; }
            double best = 0;
            const double a = side ? 1 - f : f;
            if (int rc = prof.maximise(a, &u, &best)) return rc;
            // The LLK has several local maxima in the contaminant's PCs (the AF clamps; hardly identified near alpha = 0),
            // and a chain of warm starts can end on a lower one than the estimate's own PCs give at this alpha: then the
            // climb starts from those as well, and the better end counts.
            if (!pts.empty() && fr.nu > 0) {
                Eval e0;
                if (int rc = prof.eval(u0, a, &e0)) return rc;
                if (e0.f > best) {
                    std::vector<double> v = u0;
                    double b2 = 0;
                    if (int rc = prof.maximise(a, &v, &b2)) return rc;
                    if (b2 > best) { best = b2; u = v; }
                }
            }
            pts.push_back(Pt{f, best, u});
            ++out->num_profile;
            if (best > llk_max) llk_max = best;
            *v = best;
            return VB2_OK;
        };
        double v_hat = 0, v0 = 0, v5 = 0;
        if (int rc = lp(f_hat, &v_hat)) return rc;
        if (int rc = lp(0.0, &v0)) return rc;
        if (int rc = lp(f_top, &v5)) return rc;
        // the root of lp(f) = llk_max - c between a and b (lp on opposite sides of the cut there): Illinois false position,
        // to |b - a| <= max(1e-6 f, 1e-9)
        auto root = [&](double a, double va, double b, double vb, double* r, double* vr) -> int {
            double cut = llk_max - kHalfChi2;
            double ha = va - cut, hb = vb - cut;
            int last = 0;
            double c = 0.5 * (a + b), vc = 0;
            for (int it = 0; it < 200; ++it) {
                c = (ha != hb) ? b - hb * (b - a) / (hb - ha) : 0.5 * (a + b);
                if (!(c > std::min(a, b) && c < std::max(a, b))) c = 0.5 * (a + b);
                if (int rc = lp(c, &vc)) return rc;
                cut = llk_max - kHalfChi2;
                const double hc = vc - cut;
                if ((hc < 0) == (ha < 0)) {
                    a = c; ha = hc;
                    if (last == -1) hb *= 0.5;
                    last = -1;
                } else {
                    b = c; hb = hc;
                    if (last == 1) ha *= 0.5;
                    last = 1;
                }
                if (std::fabs(b - a) <= std::max(1e-6 * c, 1e-9)) break;
            }
            *r = c;
            *vr = vc;
            return VB2_OK;
        };
        if (v0 >= llk_max - kHalfChi2) { out->lo = 0.0; out->llk_lo = v0; }
        else if (int rc = root(0.0, v0, f_hat, v_hat, &out->lo, &out->llk_lo)) return rc;
        if (v5 >= llk_max - kHalfChi2) { out->hi = f_top; out->llk_hi = v5; }
        else if (int rc = root(f_hat, v_hat, f_top, v5, &out->hi, &out->llk_hi)) return rc;
        if (llk_max > -est.llk1 + 1e-9 * std::fabs(est.llk1) && notices)
            std::fprintf(stderr, "NOTICE - %sa profile point has a higher log-likelihood (%.10g) than the search's estimate "
                                 "(%.10g): the search stopped short of the maximum\n", who.c_str(), llk_max, -est.llk1);
        out->llk_max = llk_max;
    }

    // ---- rows: FREEMIX, then the free PCs as .Ancestry prints them ----
    std::vector<double> se1(k, kNaN), se2(k, kNaN), v1(est.pc, est.pc + k), v2(est.pc2, est.pc2 + k);
    for (int j = 0; j < nu; ++j) {
        if (fr.shared) se1[j] = se2[j] = se[j];
        else if (fr.one_side) (fr.side_pc2 ? se2 : se1)[j] = se[j];
        else if (j < k) se1[j] = se[j];
        else se2[j - k] = se[j];
    }
    if (swapped && k >= 1) {                               // each SE follows its value
        std::swap(se1[0], se2[0]);
        if (k >= 2) std::swap(se1[1], se2[1]);
    }
    int r = 0;
    auto row = [&](int kind, int pc, double v, double s, double lo, double hi) {
        out->row_kind[r] = kind;
        out->row_pc[r] = pc;
        out->row_est[r] = v;
        out->row_se[r] = s;
        out->row_lo[r] = lo;
        out->row_hi[r] = hi;
        ++r;
    };
    row(0, 0, out->freemix, out->freemix_se, out->lo, out->hi);
    auto wald = [&](int kind, int j, double v, double s) { row(kind, j + 1, v, s, v - kZ * s, v + kZ * s); };
    if (fr.shared) {
        for (int j = 0; j < k; ++j) wald(3, j, v1[j], se1[j]);
    } else if (fr.one_side) {                              // the free side's PCs, as fitted: no index swap
        for (int j = 0; j < k; ++j) wald(fr.side_pc2 ? 2 : 1, j, fr.side_pc2 ? fr.base2[j] : fr.base1[j], fr.side_pc2 ? se2[j] : se1[j]);
    } else if (heter) {
        for (int j = 0; j < k; ++j) wald(1, j, v1[j], se1[j]);
        if (fr.pc2_free) {
            for (int j = 0; j < k; ++j) wald(2, j, v2[j], se2[j]);
        } else if (swapped) {
            // --FixPC at alpha >= 0.5: the swap prints the fixed values as the contaminant's PC1, PC2 (NA above) and the
            // free ones as the intended sample's -- those get their rows, so that no free parameter's SE is dropped
            for (int j = 0; j < std::min(k, 2); ++j) wald(2, j, v2[j], se2[j]);
        }
    }
    out->num_row = r;
    out->num_launch = prof.launches;
    return VB2_OK;
}

// One interval_at per sample as the fibers of a gang: see context.h.
IntervalGang::IntervalGang(int num_fiber, int num_pc) : gang_(num_fiber, 1), k_(num_pc), task_(num_fiber), rc_(num_fiber, VB2_OK)
{
    gang_.open(num_pc, [this](int i) {
        const Task& t = task_[i];
        int rc = VB2_ERR_INVALID;
        try {
            FiberGang* g = &gang_;
            void* user = g->user(i);
            const DerivFn fn = [user](const double* pc1, const double* pc2, double a, double* llk, double* grad, double* hess) {
                return FiberGang::derivs_cb(user, pc1, pc2, a, llk, grad, hess);      // (parks: no device call on this stack)
            };
            rc = interval_at(k_, t.data_has_known_af, *t.model, *t.est, fn, t.out, t.label, t.opt);
        } catch (const std::bad_alloc&) {
            rc = VB2_ERR_NOMEM;
        } catch (const std::exception& e) {
            set_error(e.what());
            rc = VB2_ERR_INVALID;
        } catch (...) {                              // nothing may unwind past the fiber's entry frame
            set_error("interval: unknown exception");
            rc = VB2_ERR_INVALID;
        }
        rc_[i] = rc;
    });
}

int IntervalGang::spawn(int i, const Task& t)
{
    task_[i] = t;
    rc_[i] = VB2_OK;
    if (gang_.spawn(i) < 0) {
        set_error("interval: no stack for a fiber");
        rc_[i] = VB2_ERR_NOMEM;
        return VB2_ERR_NOMEM;
    }
    return VB2_OK;
}

int IntervalGang::step(const BatchDerivsFn& fn)
{
    const int F = gang_.size(), k = k_, n = 2 * k + 1;
    std::vector<FiberGang::Request>& req = gang_.requests();
    np_.assign(F, 0);
    p1_.clear(); p2_.clear(); al_.clear();
    for (int i = 0; i < F; ++i) {
        if (gang_.idle(i) || req[i].n <= 0) continue;
        np_[i] = 1;
        p1_.insert(p1_.end(), req[i].p1, req[i].p1 + k);
        p2_.insert(p2_.end(), req[i].p2, req[i].p2 + k);
        al_.push_back(req[i].a[0]);
    }
    const size_t P = al_.size();
    if (P == 0) return VB2_OK;
    llk_.assign(P, 0.0);
    grad_.assign(P * n, 0.0);
    hess_.assign(P * n * n, 0.0);
    int rc = gang_.error();
    if (!rc) {
        rc = fn(F, np_.data(), p1_.data(), p2_.data(), al_.data(), llk_.data(), grad_.data(), hess_.data());
        ++steps;
        if (rc) gang_.fail(rc);                      // the fibers see it at resume and unwind
    }
    size_t o = 0;
    for (int i = 0; i < F && !rc; ++i) {
        if (np_[i] == 0) continue;
        req[i].out[0] = llk_[o];
        std::memcpy(req[i].grad, &grad_[o * n], sizeof(double) * n);
        std::memcpy(req[i].hess, &hess_[o * n * n], sizeof(double) * n * n);
        ++o;
    }
    gang_.resume_parked();
    return rc;
}

int intervals_lockstep(int num_sample, int num_pc, const int32_t* data_has_known_af, const vb2_model* models, int num_model,
                       const vb2_estimate* est, const BatchDerivsFn& fn, vb2_interval* out, int32_t* status, int64_t* num_step,
                       const char* const* labels, const IntervalOptions* opts)
{
    if (num_step) *num_step = 0;
    if (num_sample < 1 || num_pc < 1 || num_pc > VB2_MAX_PC || !models || (num_model != 1 && num_model != num_sample) || !est ||
        !out || !status) {
        set_error("intervals in lock-step: invalid argument (models: one entry or one per sample)");
        return VB2_ERR_INVALID;
    }
    IntervalGang g(num_sample, num_pc);
    for (int s = 0; s < num_sample; ++s) {
        IntervalGang::Task t;
        t.model = &models[num_model == 1 ? 0 : s];
        t.est = &est[s];
        t.out = &out[s];
        t.data_has_known_af = data_has_known_af && data_has_known_af[s];
        t.label = labels ? labels[s] : nullptr;
        t.opt = opts ? &opts[s] : nullptr;
        (void)g.spawn(s, t);                         // (up to its first request; a failure is the sample's own)
    }
    int rc = VB2_OK;
    while (g.pending())
        if (const int r = g.step(fn)) rc = rc ? rc : r;
    for (int s = 0; s < num_sample; ++s) status[s] = g.result(s);
    if (num_step) *num_step = g.steps;
    return rc;
}

int batch_interval(Batch* b, const vb2_model* models, int num_model, const vb2_estimate* est, vb2_interval* out, int32_t* status,
                   int64_t* num_step, const char* const* labels)
{
    std::vector<int32_t> kaf(b->num_sample, 0);
    for (int s = 0; s < b->num_sample; ++s) {
        if (!b->slot(s)) {
            set_error("vb2_batch_interval: the batch has an empty slot");
            return VB2_ERR_INVALID;
        }
        kaf[s] = b->slot(s)->L.known_af != nullptr;
    }
    // (scratch and staging before the first fiber runs: the fibers only park)
    if (const int rc = b->ensure_deriv_resources()) return rc;
    const BatchDerivsFn fn = [b](int32_t, const int32_t* np, const double* p1, const double* p2, const double* a, double* llk,
                                 double* grad, double* hess) { return b->derivs(np, p1, p2, a, llk, grad, hess); };
    return intervals_lockstep(b->num_sample, b->num_pc, kaf.data(), models, num_model, est, fn, out, status, num_step, labels);
}

// <prefix>.CI: the rows of vb2_interval, numbers in the default ostream format (as .Ancestry), NA where there is none
int write_ci(const std::string& prefix, const vb2_interval& ci)
{
    std::ofstream f(prefix + ".CI");
    if (!f) {
        set_error("cannot open " + prefix + ".CI for writing");
        return VB2_ERR_IO;
    }
    auto num = [](double v) {
        if (std::isnan(v)) return std::string("NA");
        std::ostringstream s;
        s << v;
        return s.str();
    };
    f << "#PARAM\tESTIMATE\tSTDERR\tCI_LOW\tCI_HIGH\tMETHOD\n";
    for (int r = 0; r < ci.num_row; ++r) {
        const int kind = ci.row_kind[r];
        std::string name = "FREEMIX";
        if (kind != 0)
            name = std::string(kind == 1 ? "ContaminatingSample." : kind == 2 ? "IntendedSample." : "") + "PC" +
                   std::to_string(ci.row_pc[r]);
        const char* method = kind == 0 ? (ci.alpha_free ? "profile" : "fixed") : "wald";
        f << name << "\t" << num(ci.row_est[r]) << "\t" << num(ci.row_se[r]) << "\t" << num(ci.row_lo[r]) << "\t"
          << num(ci.row_hi[r]) << "\t" << method << "\n";
    }
    if (!f) {
        set_error("cannot write " + prefix + ".CI");
        return VB2_ERR_IO;
    }
    return VB2_OK;
}

namespace {
// --ConfidenceInterval as a stage of the run: the interval on the run's context once the search is done; <prefix>.CI and its
// NOTICE after .selfSM
RunStage interval_stage(vb2_interval* ci)
{
    RunStage stage;
    stage.on_context = [ci](vb2_ctx* ctx, const vb2_flat&, const vb2_model& model, const vb2_estimate& est) -> int {
        const bool notices = model.notices != 0;
        const double t0 = now_s();
        if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Confidence interval\n");
        const int rc = ctx_interval(ctx->impl, model, est, ci);
        if (notices)
            std::fprintf(stderr, "NOTICE - Finished phase: Confidence interval  [%.3f seconds, %lld derivative launches]\n", now_s() - t0,
                         (long long)ci->num_launch);
        return rc;
    };
    stage.after_writers = [ci](const vb2_run_args& args) -> int {
        if (args.output_prefix)
            if (const int rc = write_ci(args.output_prefix, *ci)) return rc;
        std::fprintf(stderr, "NOTICE - FREEMIX 95%% CI (profile likelihood): [%g, %g]\n", ci->lo, ci->hi);
        return VB2_OK;
    };
    return stage;
}
}  // namespace

}  // namespace vb2

extern "C" int vb2_run_interval(const vb2_run_args* a, vb2_run_result* out, vb2_interval* ci)
{
    return vb2::guarded([&]() -> int {
        if (!ci) {
            vb2::set_error("vb2_run_interval: invalid argument");
            return VB2_ERR_INVALID;
        }
        if (a && out && a->devices && a->num_device > 1) {
            vb2::set_error("--ConfidenceInterval takes one device: it cannot be combined with marker shards over several --Devices");
            return VB2_ERR_INVALID;
        }
        return vb2::run_sample(a, out, vb2::interval_stage(ci));
    });
}
