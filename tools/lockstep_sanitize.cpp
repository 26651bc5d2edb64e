// lockstep_sanitize.cpp -- the lock-step interval driver (csrc/interval.cpp, csrc/lockstep.cpp) over a host evaluator, as a
// stand-alone program for AddressSanitizer and UBSan on the CPU: no device, no Python.  A concave quadratic with a
// pc1[0]-alpha coupling stands in for the likelihood; five samples under three models in one gang and each alone (the same
// bytes, steps = the longest chain), and an evaluator that fails at its third call.  Then the rows' refit driver
// (csrc/refit.cpp) with no side, pc1 and pc2 held: an ordinary case, an empty row, a failing evaluator, a fixed_row
// indirection and a fixed alpha.  From csrc/:
//   for f in interval lockstep refit estimator amoeba line_search tunables; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip -c $f.cpp -o /tmp/san_$f.o; done
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I. -Xarch_host -fsanitize=address,undefined -x hip \
//     -c ../../tools/lockstep_sanitize.cpp -o /tmp/san_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/lockstep_sanitize /tmp/san_*.o && /tmp/lockstep_sanitize
// (ASan warns once that it does not fully support swapcontext; the run must end with "ok" and no report.)
// The device-side members the host files reference are stubbed here: nothing of the device is linked.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "batch.h"
#include "context.h"
#include "interval.h"
#include "refit.h"
namespace vb2 {
thread_local std::string g_last_error;
void set_error(const std::string& m) { g_last_error = m; }
int Context::derivs_host(int, const double*, const double*, const double*, double*, double*, double*) { return VB2_ERR_INVALID; }
int Batch::derivs(const int32_t*, const double*, const double*, const double*, double*, double*, double*) { return VB2_ERR_INVALID; }
int Batch::ensure_deriv_resources() { return VB2_ERR_INVALID; }
int Context::device_minimize(MinimizeRequest*) { return VB2_ERR_INVALID; }
}
// ---- the rows' refit driver (csrc/refit.cpp) over a closed-form evaluator ----
namespace {
struct RowsEval {
    int k = 2, fail_at = 0, calls = 0, wrong = 0;
    int empty_row = -1;
    const vb2::Refit* opt = nullptr;
};
// row r's value: a concave quadratic, always negative, with its maximum at alpha = 0.05 + 0.03 r; exactly 0.0 for the empty
// row.  Counts the points whose held side is not the row's fixed PCs.
int rows_eval(void* user, int32_t num_row, const int32_t* num_point, const double* p1, const double* p2, const double* a, double* llk)
{
    RowsEval* e = static_cast<RowsEval*>(user);
    if (++e->calls == e->fail_at) return VB2_ERR_IO;
    const int k = e->k;
    size_t o = 0;
    for (int r = 0; r < num_row; ++r)
        for (int b = 0; b < num_point[r]; ++b, ++o) {
            double f = -10.0 - 1000.0 * (a[o] - 0.05 - 0.03 * r) * (a[o] - 0.05 - 0.03 * r);
            for (int j = 0; j < k; ++j)
                f -= 50.0 * (p1[o * k + j] - 0.01) * (p1[o * k + j] - 0.01) + 50.0 * (p2[o * k + j] + 0.02) * (p2[o * k + j] + 0.02);
            if (e->opt->held != vb2::Refit::kNone) {
                const double* side = e->opt->held == vb2::Refit::kPc1 ? p1 : p2;
                const double* want = e->opt->fixed + (size_t)(e->opt->fixed_row ? e->opt->fixed_row[r] : r) * k;
                if (std::memcmp(side + o * k, want, sizeof(double) * k) != 0) ++e->wrong;
            }
            llk[o] = r == e->empty_row ? 0.0 : f;
        }
    return 0;
}

// an ordinary case, an empty row, a failing evaluator and a fixed_row indirection, with no side, pc1 and pc2 held
int refit_cases()
{
    const int R = 3, k = 2;
    const double fixed[] = {0.011, -0.007, 0.02, 0.03, -0.01, 0.004};
    const int32_t indirect[] = {1, 0, 1};
    const char* const names[] = {"none", "pc1", "pc2"};
    vb2_model model;
    std::memset(&model, 0, sizeof(model));
    model.is_heter = 1;
    int bad = 0;
    for (int h = 0; h < 3; ++h) {
        int64_t steps = 0;
        vb2::Refit opt;
        opt.who = "refit_cases";
        opt.empty_message = "refit_cases: an empty row";
        opt.held = h == 0 ? vb2::Refit::kNone : h == 1 ? vb2::Refit::kPc1 : vb2::Refit::kPc2;
        opt.fixed = fixed;
        opt.homogeneous = opt.refuse_fixed_alpha = h != 0;
        opt.num_step = &steps;
        for (int c = 0; c < 4; ++c) {           // 0 ordinary, 1 an empty row, 2 the evaluator fails at its third call, 3 fixed_row
            RowsEval e;
            e.opt = &opt;
            e.empty_row = c == 1 ? 1 : -1;
            e.fail_at = c == 2 ? 3 : 0;
            opt.fixed_row = c == 3 ? indirect : nullptr;
            std::vector<vb2_estimate> est(R);
            std::vector<int32_t> status(R, -99);
            vb2::g_last_error.clear();
            const int rc = vb2::refit_lockstep(opt, rows_eval, &e, R, k, model, est.data(), status.data());
            int wrong = e.wrong;
            if (c == 2) {
                wrong += rc != VB2_ERR_IO || e.calls != 3;
                for (int r = 0; r < R; ++r) wrong += status[r] != VB2_ERR_IO;
            } else {
                wrong += rc != VB2_OK || steps != e.calls;
                for (int r = 0; r < R; ++r) {
                    if (r == e.empty_row) {
                        wrong += status[r] != VB2_ERR_INVALID || vb2::g_last_error != opt.empty_message;
                        continue;
                    }
                    wrong += status[r] != VB2_OK || !(std::fabs(est[r].alpha - (0.05 + 0.03 * r)) < 1e-3);
                }
            }
            std::printf("refit, %s held, case %d: rc %d, %d calls, status %d %d %d%s\n", names[h], c, rc, e.calls, (int)status[0],
                        (int)status[1], (int)status[2], wrong ? "  WRONG" : "");
            bad += wrong != 0;
        }
        // a fixed alpha: refused where a side is held, searched (nothing to search: the values at the fixed alpha) where not
        model.is_alpha_fixed = 1;
        model.fix_alpha = 0.02;
        RowsEval e;
        e.opt = &opt;
        std::vector<vb2_estimate> est(R);
        std::vector<int32_t> status(R, -99);
        const int rc = vb2::refit_lockstep(opt, rows_eval, &e, R, k, model, est.data(), status.data());
        if (h == 0 ? rc != VB2_OK || est[0].alpha != 0.02 : rc != VB2_ERR_INVALID || e.calls != 0) {
            ++bad;
            std::printf("refit, %s held: a fixed alpha gave rc %d\n", names[h], rc);
        }
        model.is_alpha_fixed = 0;
    }
    return bad;
}
}  // namespace

int main()
{
    const int S = 5, k = 2, n = 2 * k + 1;
    std::vector<vb2_estimate> est(S);
    std::vector<double> ca(S);
    for (int s = 0; s < S; ++s) {
        std::memset(&est[s], 0, sizeof(est[s]));
        est[s].alpha = 0.05 + 0.03 * s;
        for (int j = 0; j < k; ++j) { est[s].pc[j] = 0.01 * (j + 1); est[s].pc2[j] = -0.01 * (j + 1 + s); }
        est[s].llk1 = 1000.0;       // -LLK at the maximum
        est[s].converged = 1;
        ca[s] = 2000.0 * (s + 1);
    }
    int calls = 0;
    const vb2::BatchDerivsFn fn = [&](int32_t ns, const int32_t* np, const double* p1, const double* p2, const double* a, double* llk,
                                      double* grad, double* hess) {
        ++calls;
        size_t o = 0;
        for (int s = 0; s < ns; ++s)
            for (int b = 0; b < np[s]; ++b, ++o) {
                double f = -1000.0;
                std::vector<double> g(n), h((size_t)n * n, 0.0);
                for (int j = 0; j < n; ++j) {
                    const double v = j < k ? p1[o * k + j] : j < 2 * k ? p2[o * k + j - k] : a[o];
                    const double m = j < k ? est[s].pc[j] : j < 2 * k ? est[s].pc2[j - k] : est[s].alpha;
                    const double c = j == 2 * k ? ca[s] : 50.0 * (j + 1);
                    f -= c * (v - m) * (v - m);
                    g[j] = -2 * c * (v - m);
                    h[(size_t)j * n + j] = -2 * c;
                }
                // a coupling between pc1[0] and alpha so that the profile moves the PCs
                const double x = p1[o * k] - est[s].pc[0], y = a[o] - est[s].alpha;
                f -= 20.0 * x * y; g[0] -= 20.0 * y; g[2 * k] -= 20.0 * x;
                h[(size_t)0 * n + 2 * k] -= 20.0; h[(size_t)2 * k * n + 0] -= 20.0;
                llk[o] = f;
                std::memcpy(grad + o * n, g.data(), sizeof(double) * n);
                std::memcpy(hess + o * n * n, h.data(), sizeof(double) * n * n);
            }
        return 0;
    };
    vb2_model models[3];
    std::memset(models, 0, sizeof(models));
    models[0].is_heter = 1;                                   // default
    models[1].is_heter = 0;                                   // within ancestry
    models[2].is_heter = 1; models[2].is_alpha_fixed = 1; models[2].fix_alpha = 0.05;
    int bad = 0;
    for (int m = 0; m < 3; ++m) {
        std::vector<vb2_interval> out(S);
        std::vector<int32_t> status(S, -99);
        int64_t steps = 0;
        calls = 0;
        const int rc = vb2::intervals_lockstep(S, k, nullptr, &models[m], 1, est.data(), fn, out.data(), status.data(), &steps, nullptr);
        int64_t most = 0;
        for (int s = 0; s < S; ++s) {
            most = out[s].num_launch > most ? out[s].num_launch : most;
            if (status[s]) ++bad;
            // alone: the same bytes
            vb2_interval one; int32_t st1 = -99; int64_t steps1 = 0;
            const vb2::BatchDerivsFn fn1 = [&](int32_t, const int32_t* np, const double* p1, const double* p2, const double* a,
                                               double* llk, double* grad, double* hess) {
                std::vector<int32_t> full(S, 0); full[s] = np[0];
                return fn(S, full.data(), p1, p2, a, llk, grad, hess);
            };
            vb2::intervals_lockstep(1, k, nullptr, &models[m], 1, &est[s], fn1, &one, &st1, &steps1, nullptr);
            if (st1 || std::memcmp(&one, &out[s], sizeof(one)) != 0) { ++bad; std::printf("model %d sample %d differs alone\n", m, s); }
        }
        std::printf("model %d: rc %d, steps %lld (most launches %lld), sample 0: lo %.6f hi %.6f se %.6g\n", m, rc, (long long)steps,
                    (long long)most, out[0].lo, out[0].hi, out[0].freemix_se);
        if (rc || steps != most) ++bad;
    }
    // an evaluator that fails at its third call ends every interval
    {
        int c3 = 0;
        const vb2::BatchDerivsFn failing = [&](int32_t ns, const int32_t* np, const double* p1, const double* p2, const double* a,
                                               double* llk, double* grad, double* hess) {
            return ++c3 == 3 ? VB2_ERR_IO : fn(ns, np, p1, p2, a, llk, grad, hess);
        };
        std::vector<vb2_interval> out(S);
        std::vector<int32_t> status(S, 0);
        const int rc = vb2::intervals_lockstep(S, k, nullptr, &models[0], 1, est.data(), failing, out.data(), status.data(), nullptr, nullptr);
        if (rc != VB2_ERR_IO) ++bad;
        for (int s = 0; s < S; ++s) if (status[s] != VB2_ERR_IO) ++bad;
    }
    bad += refit_cases();
    std::printf(bad ? "FAILED (%d)\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
