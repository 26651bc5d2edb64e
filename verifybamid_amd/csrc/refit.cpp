// refit.cpp -- see refit.h.
#include "refit.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "lockstep.h"

namespace vb2 {

void set_error(const std::string& msg);         // (context.h, which this file stays clear of: it brings HIP in)

namespace {
// what a row's Estimator calls: the held side replaced by the fixed row, the gang's evaluator, and a look at the first values
struct Probe {
    void* gang_user = nullptr;
    const double* fixed = nullptr;         // null: no side is held
    bool pc1_held = false;
    int k = 0;
    bool first = true, empty = false;
    std::vector<double> rows;              // (not on the fiber's stack: alive while the request is parked)
};
int probe_eval(void* user, int32_t n, const double* p1, const double* p2, const double* a, double* o)
{
    Probe* w = static_cast<Probe*>(user);
    if (w->fixed) {
        w->rows.resize((size_t)std::max(n, 0) * (size_t)w->k);
        for (int i = 0; i < n; ++i) std::memcpy(&w->rows[(size_t)i * w->k], w->fixed, sizeof(double) * w->k);
        (w->pc1_held ? p1 : p2) = w->rows.data();
    }
    if (const int rc = FiberGang::eval_cb(w->gang_user, n, p1, p2, a, o)) return rc;
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

int refit_lockstep(const Refit& opt, RowsEvalFn fn, void* user, int num_row, int num_pc, const vb2_model& model,
                   vb2_estimate* est, int32_t* status)
{
    const int R = num_row, k = num_pc;
    if (opt.refuse_fixed_alpha && model.is_alpha_fixed) {
        set_error(std::string(opt.who) + ": a fixed alpha leaves the refit nothing to estimate (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    FiberGang gang(R, VB2_BATCH_SLOTS);
    std::vector<Probe> probes(R);
    vb2_model quiet = model;
    if (opt.homogeneous) quiet.is_heter = 0;   // llk0 at alpha = 0
    quiet.notices = 0;                         // (the reference's phase lines belong to the run's own search)
    quiet.verbose = 0;
    auto body = [&](int i) {
        probes[i].gang_user = gang.user(i);
        if (opt.held != Refit::kNone) probes[i].fixed = opt.fixed + (size_t)(opt.fixed_row ? opt.fixed_row[i] : i) * k;
        probes[i].pc1_held = opt.held == Refit::kPc1;
        probes[i].k = k;
        FiberGang::Search cfg;
        cfg.model = &quiet;
        cfg.data_has_known_af = opt.known_af && opt.known_af[i];
        cfg.eval = probe_eval;
        cfg.eval_user = &probes[i];
        std::memset(&est[i], 0, sizeof(est[i]));
        status[i] = gang.search(i, cfg, opt.who, &est[i]);
    };
    const int rc = gang.run(k, body, FiberGang::concat_step(k, [=](const int32_t* num_point, size_t, const double* p1,
                                                                   const double* p2, const double* a, double* out) {
                                return fn(user, R, num_point, p1, p2, a, out);
                            }));
    if (opt.num_step) *opt.num_step = gang.steps;
    if (rc) return rc;
    for (int r = 0; r < R; ++r)
        if (probes[r].empty) {
            status[r] = VB2_ERR_INVALID;
            set_error(opt.empty_message);
        }
    return VB2_OK;
}

}  // namespace vb2
