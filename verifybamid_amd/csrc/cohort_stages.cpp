// cohort_stages.cpp -- what a cohort run does after its last sample, each a CohortStage (cohort_stages.h): SourcesStage
// (--FindSource), RelatedStage (--FindRelated), RefitStage (--RefitSource), PairedStage (--MatchedNormal, --PairInterval);
// and the seven entry points that choose the stages of a run.  A stage that refits keeps its samples' contexts parked on
// the device; the sets it builds on them are locals of its finish(), so they are gone when the pipeline destroys the
// contexts, and then the streams they were created on.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "cohort_stages.h"
#include "conditioned.h"
#include "errfit.h"
#include "errfit_cohort.h"
#include "errstat.h"
#include "guard.h"
#include "hostio.h"
#include "paired.h"
#include "tunables.h"

using vb2::CohortEnd;
using vb2::set_error;

namespace {

const double kNaN = std::numeric_limits<double>::quiet_NaN();

bool has_file(const CohortEnd& e) { return e.a->output_prefixes && e.a->base.output_prefix; }

void notice_parked(const CohortEnd& e, const char* flag, const char* what)
{
    if (e.parked_bytes > 0)
        std::fprintf(stderr, "NOTICE - %s: the contexts of %d %s stayed on the device for the refit (%lld bytes)\n", flag,
                     (int)std::count_if(e.parked.begin(), e.parked.end(), [](vb2_ctx* c) { return c != nullptr; }), what,
                     (long long)e.parked_bytes);
}

vb2_ctx* parked(const CohortEnd& e, int s) { return (size_t)s < e.parked.size() ? e.parked[(size_t)s] : nullptr; }

// One lock-step call between its phase's notices; `call` may say something about itself for the closing one.
template <class Call>
int lockstep_phase(const vb2_model& model, const char* phase, size_t n, const char* what, Call call)
{
    std::string done;
    const double t0 = vb2::now_s();
    if (model.notices) std::fprintf(stderr, "NOTICE - Starting phase: %s (%d %s in lock-step)\n", phase, (int)n, what);
    const int rc = call(&done);
    if (model.notices) std::fprintf(stderr, "NOTICE - Finished phase: %s%s  [%.3f seconds]\n", phase, done.c_str(), vb2::now_s() - t0);
    return rc;
}

// ... and its statuses scattered: item n is who[n]'s, the call's own failure is everybody's, and a failure gives
// "NOTICE - <failed> <who[n] + first> failed" with the last error.
template <class Put>
void scatter(int rc, const std::vector<int32_t>& st, const std::vector<int>& who, const char* failed, int first, Put put)
{
    for (size_t n = 0; n < who.size(); ++n) {
        const int status = rc ? rc : st[n];
        put(who[n], n, status);
        if (status != VB2_OK) std::fprintf(stderr, "NOTICE - %s %d failed: %s\n", failed, who[n] + first, vb2::g_last_error.c_str());
    }
}

// The tail both refits share: the one-row sets on the parked contexts, ALL in one lock-step call of `optimize`;
// fit[who[n]].status becomes set n's.  The estimates, by set.
template <class Set, class Optimize, class Fit>
std::vector<vb2_estimate> refit_sets(const vb2_model& model, const char* phase, const char* failed, int first, Optimize optimize,
                                     std::vector<std::unique_ptr<Set>>& sets, const std::vector<double>& fixed,
                                     const std::vector<int>& who, std::vector<Fit>& fit)
{
    std::vector<vb2_estimate> est(sets.size());
    if (sets.empty()) return est;
    std::vector<Set*> raw;
    for (auto& p : sets) raw.push_back(p.get());
    std::vector<int32_t> st(sets.size(), VB2_ERR_INVALID);
    const int rc = lockstep_phase(model, phase, sets.size(), "searches", [&](std::string*) {
        return optimize(raw.data(), (int)raw.size(), model, fixed.data(), est.data(), st.data());
    });
    scatter(rc, st, who, failed, first, [&](int w, size_t, int status) { fit[(size_t)w].status = status; });
    return est;
}

// The scaffold of the two matrix stages: borrow the caller's arrays or, where a file or a later stage reads them, make
// room; compute; write if there is a prefix.  width: values per pair of samples.
struct Matrix {
    double* value;
    int32_t* shared;
    std::vector<double> own_value;
    std::vector<int32_t> own_shared;

    template <class Compute, class Write>
    int finish(const CohortEnd& e, bool needed, int width, Compute compute, Write write)
    {
        const int S = e.a->num_sample;
        e.set->set_count(S);
        const size_t nn = (size_t)S * (size_t)S;
        const bool file = has_file(e);
        if ((file || needed) && !value) { own_value.resize(nn * (size_t)width); value = own_value.data(); }
        if ((file || needed) && !shared) { own_shared.resize(nn); shared = own_shared.data(); }
        if (!value && !shared) return VB2_OK;
        const int rc = compute();
        return !rc && file ? write() : rc;
    }
};

struct SourcesStage : vb2::CohortStage {
    int top;
    Matrix m;
    bool needed = false;                   // a later stage reads the matrix
    SourcesStage(int top_n, double* score, int32_t* shared)
        : CohortStage("--FindSource", VB2_SET_SOURCE), top(top_n), m{score, shared, {}, {}} {}
    int finish(const CohortEnd& e) override
    {
        return m.finish(e, needed, 1, [&] { return e.set->scores(m.value, m.shared); }, [&] {
            return vb2::write_sources(e.a->base.output_prefix, e.a->num_sample, top, e.a->output_prefixes, e.out, e.status, m.value, m.shared);
        });
    }
};

// the set also keeps the second pair of planes -- one marginal launch per sample all the same
struct RelatedStage : vb2::CohortStage {
    int top;
    Matrix m;
    RelatedStage(int top_n, double* llr, int32_t* shared)
        : CohortStage("--FindRelated", VB2_SET_RELATED), top(top_n), m{llr, shared, {}, {}} {}
    int finish(const CohortEnd& e) override
    {
        for (int s = 0; s < e.a->num_sample; ++s)
            if (e.status[s] != VB2_OK)
                std::fprintf(stderr, "NOTICE - --FindRelated: sample %d failed (status %d) and is left out of the relatedness matrix\n",
                             s, (int)e.status[s]);
        return m.finish(e, false, VB2_NUM_RELATION, [&] { return e.set->relations(m.value, m.shared); }, [&] {
            return vb2::write_related(e.a->base.output_prefix, e.a->num_sample, top, e.a->output_prefixes, e.status, m.value, m.shared);
        });
    }
};

// --RefitSource, after the matrix: one refit per sample -- its best candidate, where that candidate's score is finite
// and > 0 --, each a one-hypothesis set on the sample's parked context (a sample is parked when its row was made), ALL in
// one lock-step call; fit[] and <Output>.SourceFit.  A refit that fails leaves its row NA, gives a NOTICE and does not
// fail the run.
struct RefitStage : vb2::CohortStage {
    SourcesStage& src;
    vb2_source_fit* fit_out;
    RefitStage(SourcesStage& sources, vb2_source_fit* fit) : CohortStage("--RefitSource", VB2_SET_SOURCE), src(sources), fit_out(fit)
    {
        src.needed = true;
    }
    bool keeps(int, bool row_made) const override { return row_made; }

    // the first row of sample i in .Sources: the first of the largest scores (write_sources: a stable sort); -1: none
    static int best_candidate(const double* score, int S, int i)
    {
        int best = -1;
        for (int j = 0; j < S; ++j) {
            const double v = score[(size_t)i * S + j];
            if (j == i || std::isnan(v)) continue;
            if (best < 0 || v > score[(size_t)i * S + best]) best = j;
        }
        return best;
    }

    int finish(const CohortEnd& e) override
    {
        const int S = e.a->num_sample;
        const double* score = src.m.value;
        std::vector<vb2_source_fit> fit((size_t)S);
        std::vector<std::unique_ptr<vb2::Conditioned>> sets;
        std::vector<int> who;
        std::vector<double> fixed;
        notice_parked(e, flag, "samples");
        for (int i = 0; i < S; ++i) {
            vb2_source_fit& f = fit[(size_t)i];
            std::memset(&f, 0, sizeof(f));
            f.candidate = -1;
            f.status = VB2_SOURCE_FIT_NONE;
            f.llr = f.freemix = f.freelk1 = f.alpha_given = f.lk1_given = f.lk0_given = f.delta_lk = kNaN;
            if (e.status[i] != VB2_OK || !score || src.top < 1) continue;
            const vb2_estimate& est = e.out[i].est;
            f.freemix = est.alpha < 0.5 ? est.alpha : 1 - est.alpha;
            f.freelk1 = est.llk1;
            const int best = best_candidate(score, S, i);
            if (best < 0) continue;
            f.candidate = best;
            f.llr = score[(size_t)i * S + best];
            f.markers = src.m.shared ? src.m.shared[(size_t)i * S + best] : 0;
            if (!(std::isfinite(f.llr) && f.llr > 0) || !parked(e, i)) continue;
            // the target's search point, as the source set took it: its pc1 is what the refit holds
            vb2::Context* c = parked(e, i)->impl;
            std::vector<double> p1, p2;
            vb2::search_point(*c, e.model, est, &p1, &p2, nullptr);
            vb2::Conditioned* set = nullptr;
            const int32_t cand = best;
            if (const int rc = vb2::Conditioned::create_from_set(c, e.set, 1, &cand, &set)) {
                f.status = rc;
                std::fprintf(stderr, "NOTICE - --RefitSource: sample %d is not refitted: %s\n", i, vb2::g_last_error.c_str());
                continue;
            }
            sets.emplace_back(set);
            who.push_back(i);
            fixed.insert(fixed.end(), p1.begin(), p1.end());
        }
        const std::vector<vb2_estimate> est = refit_sets(e.model, "Refit given the source", "--RefitSource: the refit of sample", 0,
                                                         vb2::conditioned_optimize, sets, fixed, who, fit);
        for (size_t n = 0; n < who.size(); ++n) {
            vb2_source_fit& f = fit[(size_t)who[n]];
            if (f.status != VB2_OK) continue;
            f.alpha_given = est[n].alpha;
            f.lk1_given = est[n].llk1;
            f.lk0_given = est[n].llk0;
            f.delta_lk = (-f.lk1_given) - (-f.freelk1);
        }
        if (fit_out) std::memcpy(fit_out, fit.data(), sizeof(vb2_source_fit) * (size_t)S);
        return has_file(e) ? vb2::write_source_fit(e.a->base.output_prefix, S, e.a->output_prefixes, fit.data()) : VB2_OK;
    }
};

// --MatchedNormal: the listed normals get a q row in the set, the listed tumours' contexts are parked -- whether or not a
// row was made --, and after the last sample there is one refit per pair whose tumour and normal were both searched: a
// one-hypothesis set on the tumour's context, built on the device from the normal's q row, ALL in one lock-step call;
// fits[] and <Output>.PairFit.  A refit that fails leaves NA, gives a NOTICE and does not fail the run.  --PairInterval:
// then ONE vb2_paired_interval over the refitted pairs, before the sets go -- ci[] and <Output>.PairCI.
struct PairedStage : vb2::CohortStage {
    typedef std::vector<std::unique_ptr<vb2::Paired>> Sets;
    std::vector<int32_t> tumour, normal;       // [pair] sample indices
    std::vector<char> is_tumour, is_normal;    // [sample]
    double hom_min;
    vb2_pair_fit* fit_out;
    bool interval;
    vb2_interval* ci_out;

    PairedStage(int num_sample, int num_pair, const int32_t* t, const int32_t* n, double hom, vb2_pair_fit* fits, bool with_interval,
                vb2_interval* ci)
        : CohortStage("--MatchedNormal", VB2_SET_SOURCE), tumour(t, t + num_pair), normal(n, n + num_pair),
          is_tumour((size_t)num_sample, 0), is_normal((size_t)num_sample, 0), hom_min(hom), fit_out(fits), interval(with_interval), ci_out(ci)
    {
        for (int p = 0; p < num_pair; ++p) {
            is_tumour[(size_t)t[p]] = 1;
            is_normal[(size_t)n[p]] = 1;
        }
    }
    bool wants_row(int s) const override { return is_normal[(size_t)s] != 0; }
    bool keeps(int s, bool) const override { return is_tumour[(size_t)s] != 0; }

    // fit[] as it stands before the refit, and a set for every pair that can be refitted: who[n] is set n's pair, fixed
    // its normal's intended PCs
    void build_sets(const CohortEnd& e, std::vector<vb2_pair_fit>& fit, Sets& sets, std::vector<int>& who, std::vector<double>& fixed)
    {
        auto folded = [](double a) { return a < 0.5 ? a : 1 - a; };
        for (int p = 0; p < (int)tumour.size(); ++p) {
            const int t = tumour[(size_t)p], n = normal[(size_t)p];
            vb2_pair_fit& f = fit[(size_t)p];
            std::memset(&f, 0, sizeof(f));
            f.tumour = t;
            f.normal = n;
            f.status = VB2_PAIR_FIT_NONE;
            f.normal_freemix = f.freemix = f.freelk1 = f.alpha_paired = f.lk1_paired = f.lk0_paired = kNaN;
            if (e.status[t] != VB2_OK || e.status[n] != VB2_OK) {
                std::fprintf(stderr, "NOTICE - --MatchedNormal: pair %d is not refitted: its %s failed (status %d)\n", p + 1,
                             e.status[t] != VB2_OK ? "tumour" : "normal", (int)(e.status[t] != VB2_OK ? e.status[t] : e.status[n]));
                continue;
            }
            const vb2_estimate& est = e.out[n].est;
            f.normal_freemix = folded(est.alpha);
            f.freemix = folded(e.out[t].est.alpha);
            f.freelk1 = e.out[t].est.llk1;
            f.status = VB2_ERR_INVALID;
            if (!parked(e, t)) {
                std::fprintf(stderr, "NOTICE - --MatchedNormal: pair %d is not refitted: the tumour's context is gone\n", p + 1);
                continue;
            }
            // the normal's search point, as the source set took it: its pc2 -- the intended sample's -- is what the refit holds
            vb2::Context* c = parked(e, t)->impl;
            std::vector<double> p1, p2;
            vb2::search_point(*c, e.model, est, &p1, &p2, nullptr);
            vb2::Paired* set = nullptr;
            const int32_t nrm = n;
            if (const int rc = vb2::Paired::create_from_set(c, e.set, 1, &nrm, hom_min, &set)) {
                f.status = rc;
                std::fprintf(stderr, "NOTICE - --MatchedNormal: pair %d is not refitted: %s\n", p + 1, vb2::g_last_error.c_str());
                continue;
            }
            f.markers = (int32_t)set->given[0];
            sets.emplace_back(set);
            who.push_back(p);
            fixed.insert(fixed.end(), p2.begin(), p2.end());
        }
    }

    // --PairInterval: the intervals of the refitted pairs, ALL in one lock-step gang on the parked contexts
    void intervals(const CohortEnd& e, const Sets& sets, const std::vector<int>& who, const std::vector<double>& fixed,
                   const std::vector<vb2_estimate>& est, const std::vector<vb2_pair_fit>& fit, std::vector<vb2_interval>& ci,
                   std::vector<int32_t>& ci_status)
    {
        std::vector<vb2::Paired*> raw;
        std::vector<int> pair_of;
        std::vector<double> fixed_l;
        std::vector<vb2_estimate> est_l;
        const int k = e.a->base.num_pc;
        for (size_t i = 0; i < who.size(); ++i) {
            if (fit[(size_t)who[i]].status != VB2_OK) continue;
            raw.push_back(sets[i].get());
            pair_of.push_back(who[i]);
            fixed_l.insert(fixed_l.end(), fixed.begin() + (long)i * k, fixed.begin() + (long)(i + 1) * k);
            est_l.push_back(est[i]);
        }
        if (raw.empty()) return;
        std::vector<vb2_interval> ci_l(raw.size());
        std::vector<int32_t> st_l(raw.size(), VB2_ERR_INVALID);
        const int rc = lockstep_phase(e.model, "Intervals given the matched normal", raw.size(), "intervals", [&](std::string* done) {
            int64_t steps = 0;
            const int r = vb2::paired_interval(raw.data(), (int)raw.size(), e.model, fixed_l.data(), est_l.data(), ci_l.data(),
                                               st_l.data(), &steps);
            *done = " (" + std::to_string((long long)steps) + " launch pairs)";
            return r;
        });
        scatter(rc, st_l, pair_of, "--PairInterval: the interval of pair", 1, [&](int p, size_t i, int status) {
            ci_status[(size_t)p] = status;
            if (status == VB2_OK) ci[(size_t)p] = ci_l[i];
        });
    }

    int finish(const CohortEnd& e) override
    {
        const int P = (int)tumour.size();
        std::vector<vb2_pair_fit> fit((size_t)P);
        Sets sets;
        std::vector<int> who;
        std::vector<double> fixed;
        notice_parked(e, flag, "tumours");
        build_sets(e, fit, sets, who, fixed);
        const std::vector<vb2_estimate> est = refit_sets(e.model, "Refit given the matched normal", "--MatchedNormal: the refit of pair",
                                                         1, vb2::paired_optimize, sets, fixed, who, fit);
        for (size_t i = 0; i < who.size(); ++i) {
            vb2_pair_fit& f = fit[(size_t)who[i]];
            if (f.status != VB2_OK) continue;
            f.alpha_paired = est[i].alpha;
            f.lk1_paired = est[i].llk1;
            f.lk0_paired = est[i].llk0;
        }
        std::vector<vb2_interval> ci((size_t)P);
        std::vector<int32_t> ci_status((size_t)P, VB2_PAIR_FIT_NONE);
        if (P > 0) std::memset(ci.data(), 0, sizeof(vb2_interval) * (size_t)P);
        if (interval) {
            intervals(e, sets, who, fixed, est, fit, ci, ci_status);
            if (ci_out) std::memcpy(ci_out, ci.data(), sizeof(vb2_interval) * (size_t)P);
        }
        if (fit_out) std::memcpy(fit_out, fit.data(), sizeof(vb2_pair_fit) * (size_t)P);
        if (!has_file(e)) return VB2_OK;
        const int rc = vb2::write_pair_fit(e.a->base.output_prefix, P, e.a->pileup_paths, fit.data());
        if (rc || !interval) return rc;
        return vb2::write_pair_ci(e.a->base.output_prefix, P, e.a->pileup_paths, fit.data(), ci.data(), ci_status.data());
    }
};

// ---- the entry points' checks, in the order every one of them makes them ----

// --CohortFitError: the error-rate fit of the cohort's samples (errfit_cohort.h).  The stage takes the
// retiring samples' flattened inputs, with the raw arrays in them, and in finish() fits them in lock-step -- per sample, or
// pooled into one table -- through one ErrStatBatch per chunk of at most 64 samples.
struct ErrFitStage : vb2::CohortStage {
    const vb2_errfit_opts* opts;
    const bool pooled;
    vb2_errfit* fits_out;
    vb2_errfit_pool* pool_out;
    std::vector<std::unique_ptr<vb2_flat>> flats;
    std::vector<vb2_estimate> est;
    ErrFitStage(int S, const vb2_errfit_opts* o, bool pool_them, vb2_errfit* fits, vb2_errfit_pool* pool)
        : CohortStage("--CohortFitError", 0), opts(o), pooled(pool_them), fits_out(fits), pool_out(pool), flats((size_t)S), est((size_t)S)
    {
    }
    bool takes_flat() const override { return true; }
    void take_flat(int s, std::unique_ptr<vb2_flat> f, const vb2_estimate& e) override
    {
        flats[(size_t)s] = std::move(f);
        est[(size_t)s] = e;
    }

    int finish(const CohortEnd& e) override
    {
        const int S = e.a->num_sample, kMax = VB2_ERRSTAT_BATCH_MAX;
        if (pooled && S > kMax) {
            set_error("--PooledError: one pool holds at most " + std::to_string(kMax) + " samples, the list has " + std::to_string(S));
            return VB2_ERR_INVALID;
        }
        vb2_options opt{};
        opt.device = e.a->base.num_device > 0 && e.a->base.devices ? e.a->base.devices[0] : e.a->base.device;
        // the raw inputs stay on the device for the whole fit: all of a chunk or nothing
        for (int c0 = 0; c0 < S; c0 += kMax) {
            const int n = std::min(kMax, S - c0);
            long long need = 0;
            bool panel_counted = false;
            for (int i = c0; i < c0 + n; ++i)
                if (e.status[i] == VB2_OK && flats[(size_t)i]) {
                    const vb2_input& in = flats[(size_t)i]->input;
                    const long long M = in.num_marker, R = M > 0 ? in.read_off[M] - in.read_off[0] : 0;
                    need += 2 * R + 9 * (M + 1);                     // bases, qualities; offsets and alleles
                    if (!panel_counted) need += M * 8LL * (in.num_pc + 1);          // (the samples share the panel's arrays)
                    panel_counted = true;
                }
            size_t free_b = 0, total_b = 0;
            if (opt.device >= 0) (void)hipSetDevice(opt.device);
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (unsigned long long)need > free_b) {
                set_error("--CohortFitError: the raw inputs of samples " + std::to_string(c0) + ".." + std::to_string(c0 + n - 1) + " take " +
                          std::to_string(need) + " bytes on the device, " + std::to_string(free_b) + " of " + std::to_string(total_b) +
                          " are free");
                return VB2_ERR_NOMEM;
            }
        }
        std::vector<vb2_errfit> fits((size_t)S);
        vb2_errfit_pool pool{};
        int iters = 0, fitted = 0, bins = 0;
        double lrt_sum = 0.0;
        const double t0 = vb2::now_s();
        for (int c0 = 0; c0 < S; c0 += kMax) {
            const int n = std::min(kMax, S - c0);
            std::vector<const vb2_input*> in((size_t)n, nullptr);
            std::vector<int32_t> enter((size_t)n);
            for (int i = 0; i < n; ++i) {
                const size_t s = (size_t)(c0 + i);
                enter[(size_t)i] = e.status[s] != VB2_OK ? e.status[s] : flats[s] ? VB2_OK : VB2_ERR_INVALID;
                if (enter[(size_t)i] == VB2_OK) in[(size_t)i] = &flats[s]->input;
            }
            if (const int rc = vb2::errfit_cohort_inputs(in.data(), n, &opt, e.model, est.data() + c0, enter.data(), opts, pooled,
                                                         fits.data() + c0, &pool))
                return rc;
            iters = std::max(iters, (int)pool.num_iter);
            fitted += pool.num_fitted;
            bins = std::max(bins, (int)pool.num_bin);
            lrt_sum += pool.lrt_sum;
        }
        const auto folded = [](double a) { return a < 0.5 ? a : 1 - a; };
        const char* const* prefixes = e.a->output_prefixes;
        if (!pooled && prefixes)
            for (int s = 0; s < S; ++s)
                if (e.status[s] == VB2_OK && fits[(size_t)s].status == VB2_OK && flats[(size_t)s] && prefixes[s])
                    if (const int rc = vb2::write_errfit_files(prefixes[s], flats[(size_t)s]->viewer.SEQ_SM, folded(est[(size_t)s].alpha),
                                                               fits[(size_t)s]))
                        return rc;
        if (pooled && e.a->base.output_prefix) {
            const std::string prefix = e.a->base.output_prefix;
            if (const int rc = vb2::write_error_rates(prefix, pool.err, pool.n, pool.s)) return rc;
            const int rc = vb2::write_text_file(prefix + ".PooledFit", [&](std::ostream& fout) {
                fout << "#SEQ_ID\tFREEMIX\tFREEMIX_FIT\tLRT\tFREELK1_FIT\tFREELK1_NOMINAL\tSTATUS\n";
                for (int s = 0; s < S; ++s) {
                    const vb2_errfit& f = fits[(size_t)s];
                    fout << (flats[(size_t)s] ? flats[(size_t)s]->viewer.SEQ_SM : std::string(e.a->pileup_paths[s])) << "\t";
                    if (e.status[s] == VB2_OK) fout << folded(est[(size_t)s].alpha);
                    else fout << "NA";
                    if (f.status == VB2_OK) fout << "\t" << folded(f.est.alpha) << "\t" << f.lrt << "\t" << f.llk_fit << "\t" << f.llk_nominal;
                    else fout << "\tNA\tNA\tNA\tNA";
                    fout << "\t" << f.status << "\n";
                }
            });
            if (rc) return rc;
        }
        if (pooled)
            std::fprintf(stderr, "NOTICE - --PooledError: one error table for %d of %d samples, %d qualities fitted in %d iterations%s; "
                                 "summed LRT %g  [%.3f seconds]\n", fitted, S, bins, iters, pool.converged ? "" : ", not converged", lrt_sum,
                         vb2::now_s() - t0);
        else
            std::fprintf(stderr, "NOTICE - --CohortFitError: the error rates of %d of %d samples fitted, each on its own table, at most %d "
                                 "iterations; summed LRT %g  [%.3f seconds]\n", fitted, S, iters, lrt_sum, vb2::now_s() - t0);
        if (fits_out) std::memcpy(fits_out, fits.data(), sizeof(vb2_errfit) * (size_t)S);
        if (pool_out) *pool_out = pool;
        flats.clear();
        return VB2_OK;
    }
};

int check_args(const char* fn, const vb2_cohort_args* a, const vb2_run_result* out, const int32_t* status, bool rest_ok = true)
{
    if (a && out && status && a->num_sample >= 1 && a->pileup_paths && a->base.ud_path && a->base.mean_path && a->base.bed_path &&
        a->base.num_pc >= 1 && a->base.num_pc <= VB2_MAX_PC && rest_ok)
        return VB2_OK;
    set_error(std::string(fn) + ": invalid argument");
    return VB2_ERR_INVALID;
}

int refuse(bool when, const char* text)
{
    if (when) set_error(text);
    return when ? VB2_ERR_INVALID : VB2_OK;
}

int one_device(const vb2_cohort_args* a, const char* text) { return refuse(a->base.num_device > 1 || a->base.num_device < 0, text); }

int cohort_run_paired(const vb2_cohort_args* a, int32_t num_pair, const int32_t* tumour, const int32_t* normal, double hom_min,
                      vb2_run_result* out, int32_t* status, vb2_pair_fit* fits, bool interval, vb2_interval* ci)
{
    if (const int rc = check_args("vb2_cohort_run_paired", a, out, status, num_pair >= 1 && tumour && normal)) return rc;
    if (const int rc = one_device(a, "--MatchedNormal takes one device: the normals' rows and the refits given them are not spread over several --Devices"))
        return rc;
    if (const int rc = refuse(a->base.model.is_alpha_fixed,
                              "--MatchedNormal cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate"))
        return rc;
    if (const int rc = refuse(!(hom_min >= 0.0 && hom_min <= 1.0), "--NormalHomMin takes a probability within [0, 1]")) return rc;
    if (const int rc = vb2::check_pairs("vb2_cohort_run_paired", a->num_sample, num_pair, tumour, normal)) return rc;
    std::unique_ptr<PairedStage> pairs;
    const int rc = vb2::guarded([&] {
        pairs.reset(new PairedStage(a->num_sample, num_pair, tumour, normal, hom_min, fits, interval, ci));
        return VB2_OK;
    });
    return rc ? rc : vb2::cohort_run_with(a, out, status, {{pairs.get()}});
}

}  // namespace

extern "C" int vb2_cohort_run(const vb2_cohort_args* a, vb2_run_result* out, int32_t* status)
{
    if (const int rc = check_args("vb2_cohort_run", a, out, status, a && a->base.num_device >= 0 && a->base.num_device <= 64)) return rc;
    // (Tunables::cohort_dup_devices: a test switch -- the pipelines of a several-device run, their group
    // schedule and the readers' per-device look-ahead exercised on a machine with one GPU)
    const bool dup_ok = vb2::tunables().cohort_dup_devices != 0;
    for (int i = 0; i < a->base.num_device && !dup_ok; ++i)
        for (int j = 0; j < i; ++j)      // (two lock-step pipelines on one device would each launch device-filling grids)
            if (a->base.devices && a->base.devices[i] == a->base.devices[j]) return refuse(true, "vb2_cohort_run: a device is listed twice");
    return vb2::cohort_run_with(a, out, status, {});
}

extern "C" int vb2_cohort_run_sources(const vb2_cohort_args* a, int32_t top, vb2_run_result* out, int32_t* status, double* score,
                                      int32_t* shared)
{
    if (const int rc = check_args("vb2_cohort_run_sources", a, out, status, top >= 0)) return rc;
    if (const int rc = one_device(a, "--FindSource takes one device: a source set is not spread over several --Devices")) return rc;
    SourcesStage sources(top, score, shared);
    return vb2::cohort_run_with(a, out, status, {{&sources}});
}

extern "C" int vb2_cohort_run_related(const vb2_cohort_args* a, int32_t related_top, int32_t source_top, vb2_run_result* out,
                                      int32_t* status, double* llr, int32_t* shared)
{
    if (const int rc = check_args("vb2_cohort_run_related", a, out, status, related_top >= 0 && source_top >= 0)) return rc;
    if (const int rc = one_device(a, "--FindRelated takes one device: a set of samples is not spread over several --Devices")) return rc;
    SourcesStage sources(source_top, nullptr, nullptr);
    RelatedStage related(related_top, llr, shared);
    return vb2::cohort_run_with(a, out, status, {{source_top > 0 ? &sources : nullptr, &related}});
}

extern "C" int vb2_cohort_run_source_fits(const vb2_cohort_args* a, int32_t top, vb2_run_result* out, int32_t* status, double* score,
                                          int32_t* shared, vb2_source_fit* fit)
{
    if (const int rc = check_args("vb2_cohort_run_source_fits", a, out, status, top >= 0)) return rc;
    if (const int rc = one_device(a, "--RefitSource takes one device: a source set and the refits given it are not spread over several --Devices"))
        return rc;
    if (const int rc = refuse(a->base.model.is_alpha_fixed,
                              "--RefitSource cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate"))
        return rc;
    SourcesStage sources(top, score, shared);
    RefitStage refit(sources, fit);
    return vb2::cohort_run_with(a, out, status, {{&sources, &refit}});
}

extern "C" int vb2_cohort_run_intervals(const vb2_cohort_args* a, int32_t source_top, vb2_run_result* out, int32_t* status,
                                        vb2_interval* ci)
{
    if (const int rc = check_args("vb2_cohort_run_intervals", a, out, status, source_top >= 0)) return rc;
    if (const int rc = one_device(a, "--CohortInterval takes one device: the intervals of a cohort are not spread over several --Devices"))
        return rc;
    SourcesStage sources(source_top, nullptr, nullptr);
    return vb2::cohort_run_with(a, out, status, {{source_top > 0 ? &sources : nullptr}, true, ci});
}

extern "C" int vb2_cohort_run_errfit(const vb2_cohort_args* a, const vb2_errfit_opts* fit_opts, int32_t pooled, vb2_run_result* out,
                                     int32_t* status, vb2_errfit* fits, vb2_errfit_pool* pooled_out)
{
    if (const int rc = check_args("vb2_cohort_run_errfit", a, out, status)) return rc;
    if (const int rc = one_device(a, "--CohortFitError takes one device: the samples' raw inputs are fitted together on one device, not "
                                     "over several --Devices"))
        return rc;
    if (const int rc = refuse(a->base.model.is_alpha_fixed,
                              "--CohortFitError cannot be combined with --FixAlpha: a fixed alpha leaves the fit nothing to tell errors from"))
        return rc;
    if (const int rc = refuse(a->base.search.num_start > 1 || a->base.search.line_search,
                              "--CohortFitError cannot be combined with --NumStart / --LineSearch: every iteration's search is the "
                              "reference's own"))
        return rc;
    {   // the fit's options, before any file is read
        double kappa = 0.0, tol = 0.0;
        int max_iter = 0;
        if (const int rc = vb2::errfit_options(a->base.model, fit_opts, "vb2_cohort_run_errfit", &kappa, &tol, &max_iter)) return rc;
    }
    if (const int rc = refuse(pooled && a->num_sample > VB2_ERRSTAT_BATCH_MAX, "--PooledError: one pool holds at most 64 samples"))
        return rc;
    ErrFitStage fit(a->num_sample, fit_opts, pooled != 0, fits, pooled_out);
    return vb2::cohort_run_with(a, out, status, {{&fit}});
}

extern "C" int vb2_cohort_run_under_table(const vb2_cohort_args* a, const double* err_table, vb2_run_result* out, int32_t* status)
{
    if (const int rc = check_args("vb2_cohort_run_under_table", a, out, status, a && a->base.num_device >= 0 && a->base.num_device <= 64))
        return rc;
    if (!vb2::err_table_ok(err_table, "vb2_cohort_run_under_table")) return VB2_ERR_INVALID;
    return vb2::cohort_run_with(a, out, status, {{}, false, nullptr, err_table});
}

extern "C" int vb2_cohort_run_paired(const vb2_cohort_args* a, int32_t num_pair, const int32_t* tumour, const int32_t* normal,
                                     double hom_min, vb2_run_result* out, int32_t* status, vb2_pair_fit* fits)
{
    return cohort_run_paired(a, num_pair, tumour, normal, hom_min, out, status, fits, false, nullptr);
}

extern "C" int vb2_cohort_run_paired_intervals(const vb2_cohort_args* a, int32_t num_pair, const int32_t* tumour,
                                               const int32_t* normal, double hom_min, vb2_run_result* out, int32_t* status,
                                               vb2_pair_fit* fits, vb2_interval* ci)
{
    return cohort_run_paired(a, num_pair, tumour, normal, hom_min, out, status, fits, true, ci);
}
