// paired.cpp -- host side of the likelihood given priors on both components (marker_sum_kernels.hip: PairTerm; DESIGN.md
// section 16): what fills the planes of a set of pair hypotheses (the rest of the set: row_set.cpp), and the options of the
// refits with the intended sample's PCs held (refit.h).
#include "paired.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "context.h"
#include "deriv_kernels.h"
#include "device_util.h"
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

// ---- derivatives ----

Paired::~Paired()
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    delete deriv_stage_;                   // (its steps are synchronous: nothing of it is in flight)
    give_device(d_deriv_, d_deriv_bytes_, ctx->device);
}

const float* Paired::hyp_planes(int h) const { return planes() + (size_t)h * paired_hyp_floats(ctx->L); }

double* Paired::deriv_marker(int h) const { return d_deriv_ + (size_t)h * kDerivChunk * kDerivVals * (size_t)ctx->L.m_pad; }

int Paired::ensure_deriv_scratch()
{
    VB2_HIP(hipSetDevice(ctx->device));
    if (d_deriv_) return VB2_OK;
    const size_t bytes = sizeof(double) * (size_t)num_row * kDerivChunk * kDerivVals * (size_t)ctx->L.m_pad;
    void* p = nullptr;
    if (const int rc = take_device(std::max<size_t>(bytes, 256), ctx->device, &p, &d_deriv_bytes_, "vb2_paired_derivs")) return rc;
    d_deriv_ = static_cast<double*>(p);
    device_bytes += (int64_t)d_deriv_bytes_;
    return VB2_OK;
}

int PairDerivStage::create(int device, int num_job, int num_pc, PairDerivStage** out)
{
    *out = nullptr;
    std::unique_ptr<PairDerivStage> s(new PairDerivStage());
    const size_t J = (size_t)num_job, n = 2 * (size_t)num_pc + 1;
    s->device_ = device;
    s->num_job_ = num_job;
    s->k_ = num_pc;
    s->o_planes_ = up256(sizeof(DerivJob) * J);
    s->o_rows_ = up256(s->o_planes_ + sizeof(const float*) * J);
    s->o_res_ = up256(s->o_rows_ + sizeof(double) * J * kDerivChunk * n);
    s->total_ = s->o_res_ + sizeof(double) * J * kDerivChunk * (size_t)deriv_out_count(num_pc);
    VB2_HIP(hipSetDevice(device));
    if (const int rc = take_device(s->total_, device, &s->d_, &s->d_bytes_, "vb2_paired_derivs")) return rc;
    s->h_ = cached_pinned_slab(s->total_, device, &s->h_bytes_);
    if (!s->h_) {
        VB2_HIP(hipHostMalloc(&s->h_, s->total_, hipHostMallocMapped));
        s->h_bytes_ = s->total_;
    }
    *out = s.release();
    return VB2_OK;
}

PairDerivStage::~PairDerivStage()
{
    if (device_ < 0) return;
    (void)hipSetDevice(device_);
    give_device(d_, d_bytes_, device_);
    if (h_ && !recycle_pinned_slab(h_, h_bytes_, device_)) (void)hipHostFree(h_);
}

int paired_derivs(Paired* const* sets, int num_set, PairDerivStage* st, const int32_t* num_point, const double* pc1,
                  const double* pc2, const double* alpha, double* llk, double* grad, double* hess)
{
    const auto refuse = [](const char* what) {
        set_error(std::string("vb2_paired_derivs: ") + what);
        return VB2_ERR_INVALID;
    };
    if (!sets || num_set < 1 || !st || !num_point) return refuse("invalid argument");
    const int k = st->k_, n = 2 * k + 1, nout = deriv_out_count(k);
    struct Row { Paired* set; int h; };
    std::vector<Row> row;
    for (int s = 0; s < num_set; ++s) {
        Paired* p = sets[s];
        if (!p || !p->ctx) return refuse("invalid argument");
        if (p->ctx->num_pc != k) return refuse("the sets' contexts differ in the number of PCs");
        if (p->ctx->device != st->device_) return refuse("the sets' contexts are on several devices");
        if (p->ctx->resident_active) return refuse("not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        if (p->eval_pending()) return refuse("an evaluation step of the set is in flight");
        for (int h = 0; h < p->num_row; ++h) row.push_back(Row{p, h});
    }
    const int R = (int)row.size();
    if (R > st->num_job_) return refuse("more hypotheses than the stage has room for");
    std::vector<size_t> first((size_t)R + 1, 0);
    int most = 0;
    for (int r = 0; r < R; ++r) {
        if (num_point[r] < 0) return refuse("a negative point count");
        first[(size_t)r + 1] = first[(size_t)r] + (size_t)num_point[r];
        most = std::max(most, (int)num_point[r]);
    }
    if (most == 0) return VB2_OK;
    if (!pc1 || !pc2 || !alpha || !llk || !grad || !hess) return refuse("invalid argument");
    for (int s = 0; s < num_set; ++s)
        if (const int rc = sets[s]->ensure_deriv_scratch()) return rc;
    VB2_HIP(hipSetDevice(st->device_));
    hipStream_t stream = sets[0]->ctx->stream;
    char* const hp = static_cast<char*>(st->h_);
    char* const dp = static_cast<char*>(st->d_);
    DerivJob* const h_jobs = reinterpret_cast<DerivJob*>(hp);
    const float** const h_planes = reinterpret_cast<const float**>(hp + st->o_planes_);
    double* const h_rows = reinterpret_cast<double*>(hp + st->o_rows_);
    const double* const h_res = reinterpret_cast<const double*>(hp + st->o_res_);
    double* const d_rows = reinterpret_cast<double*>(dp + st->o_rows_);
    double* const d_res = reinterpret_cast<double*>(dp + st->o_res_);
    std::vector<int> who((size_t)R);
    for (int done = 0; done < most; done += kDerivChunk) {
        // this step's jobs: the probability-domain contexts' first (one marker launch per layout class)
        int nj = 0;
        for (int cls = 1; cls >= 0; --cls)
            for (int r = 0; r < R; ++r)
                if (num_point[r] > done && (row[(size_t)r].set->ctx->L.pd != 0) == (cls != 0)) who[(size_t)nj++] = r;
        for (int j = 0; j < nj; ++j) {
            const int r = who[(size_t)j];
            const Row& w = row[(size_t)r];
            const int cnt = std::min(kDerivChunk, num_point[r] - done);
            DerivJob& job = h_jobs[j];
            job.L = w.set->ctx->L;
            job.L.stamps = nullptr;
            job.points = d_rows + (size_t)j * kDerivChunk * n;
            job.marker = w.set->deriv_marker(w.h);
            job.out = d_res + (size_t)j * kDerivChunk * nout;
            job.num_point = cnt;
            job.reserved = 0;
            h_planes[j] = w.set->hyp_planes(w.h);
            for (int b = 0; b < cnt; ++b) {
                const size_t src = first[(size_t)r] + (size_t)done + (size_t)b;
                double* dst = h_rows + ((size_t)j * kDerivChunk + b) * n;
                std::memcpy(dst, pc1 + src * k, sizeof(double) * k);
                std::memcpy(dst + k, pc2 + src * k, sizeof(double) * k);
                dst[2 * k] = alpha[src];
            }
        }
        const size_t up = st->o_rows_ + sizeof(double) * (size_t)nj * kDerivChunk * n;
        VB2_HIP(hipMemcpyAsync(dp, hp, up, hipMemcpyHostToDevice, stream));
        if (nj == 1)
            // one job: the single-sample launch, its grid sized for that context alone (the same bits)
            VB2_HIP(launch_llk_pair_derivs(h_jobs[0].L, h_jobs[0].num_point, h_jobs[0].points, h_planes[0], h_jobs[0].marker,
                                           h_jobs[0].out, stream));
        else
            VB2_HIP(launch_llk_pair_derivs_multi(h_jobs, reinterpret_cast<const DerivJob*>(dp),
                                                 reinterpret_cast<const float* const*>(dp + st->o_planes_), nj, stream));
        VB2_HIP(hipMemcpyAsync(hp + st->o_res_, dp + st->o_res_, sizeof(double) * (size_t)nj * kDerivChunk * nout,
                                 hipMemcpyDeviceToHost, stream));
        VB2_HIP(hipStreamSynchronize(stream));
        ++st->num_step;
        for (int j = 0; j < nj; ++j) {
            const int r = who[(size_t)j];
            const int cnt = std::min(kDerivChunk, num_point[r] - done);
            for (int b = 0; b < cnt; ++b) {
                const size_t dst = first[(size_t)r] + (size_t)done + (size_t)b;
                const double* res = h_res + ((size_t)j * kDerivChunk + b) * nout;
                llk[dst] = res[0];
                std::memcpy(grad + dst * n, res + 1, sizeof(double) * n);
                double* hs = hess + dst * n * n;
                int e = 1 + n;
                for (int i = 0; i < n; ++i)
                    for (int jj = i; jj < n; ++jj, ++e) hs[(size_t)i * n + jj] = hs[(size_t)jj * n + i] = res[e];
            }
        }
    }
    return VB2_OK;
}

int Paired::derivs(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk, double* grad,
                   double* hess)
{
    if (!deriv_stage_) {
        if (const int rc = PairDerivStage::create(ctx->device, num_row, ctx->num_pc, &deriv_stage_)) return rc;
        device_bytes += (int64_t)deriv_stage_->device_bytes();
    }
    Paired* self = this;
    return paired_derivs(&self, 1, deriv_stage_, num_point, pc1, pc2, alpha, llk, grad, hess);
}

// ---- the interval of a paired refit ----

int paired_interval(Paired* const* sets, int num_set, const vb2_model& model, const double* pc2_fixed, const vb2_estimate* est,
                    vb2_interval* out, int32_t* status, int64_t* num_step, const char* const* labels)
{
    const auto refuse = [](const char* what) {
        set_error(std::string("vb2_paired_interval: ") + what);
        return VB2_ERR_INVALID;
    };
    if (num_step) *num_step = 0;
    if (!sets || num_set < 1 || !pc2_fixed || !est || !out || !status) return refuse("invalid argument");
    if (model.is_alpha_fixed) return refuse("a fixed alpha leaves the interval nothing to bound (--FixAlpha)");
    int R = 0;
    for (int s = 0; s < num_set; ++s) {
        if (!sets[s] || !sets[s]->ctx) return refuse("invalid argument");
        if (sets[s]->ctx->num_pc != sets[0]->ctx->num_pc) return refuse("the sets' contexts differ in the number of PCs");
        if (sets[s]->ctx->device != sets[0]->ctx->device) return refuse("the sets' contexts are on several devices");
        for (int t = 0; t < s; ++t)
            if (sets[t] == sets[s]) return refuse("a set is listed twice");
        R += sets[s]->num_row;
    }
    const int k = sets[0]->ctx->num_pc;
    // the hypotheses that walk a marker, in order: they are the gang's fibers
    std::vector<int> live;
    std::vector<IntervalOptions> opts;
    std::vector<int32_t> kaf;
    std::vector<vb2_estimate> est_l;
    std::vector<const char*> label_l;
    int r = 0;
    for (int s = 0; s < num_set; ++s)
        for (int h = 0; h < sets[s]->num_row; ++h, ++r) {
            std::memset(&out[r], 0, sizeof(out[r]));
            status[r] = VB2_OK;
            if (sets[s]->given[(size_t)h] == 0) {
                status[r] = VB2_ERR_INVALID;
                set_error("vb2_paired_interval: a hypothesis leaves the sample no marker");
                continue;
            }
            IntervalOptions o;
            o.held = IntervalOptions::kPc2;
            o.fixed = pc2_fixed + (size_t)s * k;
            o.fold = false;
            live.push_back(r);
            opts.push_back(o);
            kaf.push_back(sets[s]->ctx->L.known_af != nullptr);
            est_l.push_back(est[r]);
            label_l.push_back(labels ? labels[r] : nullptr);
        }
    const int F = (int)live.size();
    if (F == 0) return VB2_OK;
    // (scratch and staging before the first fiber runs: the fibers only park)
    for (int s = 0; s < num_set; ++s)
        if (const int rc = sets[s]->ensure_deriv_scratch()) return rc;
    PairDerivStage* stage = nullptr;
    if (const int rc = PairDerivStage::create(sets[0]->ctx->device, R, k, &stage)) return rc;
    const std::unique_ptr<PairDerivStage> hold(stage);
    std::vector<int32_t> np_all((size_t)R);
    const BatchDerivsFn fn = [&](int32_t, const int32_t* np, const double* p1, const double* p2, const double* a, double* llk,
                                 double* grad, double* hess) {
        std::fill(np_all.begin(), np_all.end(), 0);
        for (int i = 0; i < F; ++i) np_all[(size_t)live[(size_t)i]] = np[i];
        return paired_derivs(sets, num_set, stage, np_all.data(), p1, p2, a, llk, grad, hess);
    };
    std::vector<vb2_interval> out_l((size_t)F);
    std::vector<int32_t> status_l((size_t)F, VB2_OK);
    const int rc = intervals_lockstep(F, k, kaf.data(), &model, 1, est_l.data(), fn, out_l.data(), status_l.data(), num_step,
                                      labels ? label_l.data() : nullptr, opts.data());
    for (int i = 0; i < F; ++i) {
        out[live[(size_t)i]] = out_l[(size_t)i];
        status[live[(size_t)i]] = status_l[(size_t)i];
    }
    return rc;
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

int vb2_paired_derivs(vb2_paired* pair, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                      double* llk, double* grad, double* hess)
{
    if (!pair || !pair->impl) {
        set_error("null vb2_paired");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int { return pair->impl->derivs(num_point, pc1, pc2, alpha, llk, grad, hess); });
}

int vb2_paired_derivs_sets(vb2_paired* const* sets, int32_t num_set, const int32_t* num_point, const double* pc1,
                           const double* pc2, const double* alpha, double* llk, double* grad, double* hess)
{
    if (!sets || num_set < 1) {
        set_error("vb2_paired_derivs_sets: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        std::vector<vb2::Paired*> impl((size_t)num_set);
        int rows = 0;
        for (int s = 0; s < num_set; ++s) {
            if (!sets[s] || !sets[s]->impl) {
                set_error("null vb2_paired");
                return VB2_ERR_INVALID;
            }
            for (int t = 0; t < s; ++t)
                if (sets[t] == sets[s]) {
                    set_error("vb2_paired_derivs_sets: a set is listed twice");
                    return VB2_ERR_INVALID;
                }
            impl[(size_t)s] = sets[s]->impl;
            rows += impl[(size_t)s]->num_row;
        }
        vb2::PairDerivStage* stage = nullptr;           // (a call's own: the sets keep theirs for vb2_paired_derivs)
        if (const int rc = vb2::PairDerivStage::create(impl[0]->ctx->device, rows, impl[0]->ctx->num_pc, &stage)) return rc;
        const std::unique_ptr<vb2::PairDerivStage> hold(stage);
        return vb2::paired_derivs(impl.data(), num_set, stage, num_point, pc1, pc2, alpha, llk, grad, hess);
    });
}

int vb2_paired_interval(vb2_paired* const* sets, int32_t num_set, const vb2_model* model, const double* pc2_fixed,
                        const vb2_estimate* est, vb2_interval* out, int32_t* status, int64_t* num_step)
{
    if (!sets || num_set < 1 || !model) {
        set_error("vb2_paired_interval: invalid argument");
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
        return vb2::paired_interval(impl.data(), num_set, *model, pc2_fixed, est, out, status, num_step);
    });
}

int vb2_paired_intervals_lockstep(vb2_batch_derivs_fn fn, void* user, int32_t num_hyp, int32_t num_pc,
                                  const int32_t* data_has_known_af, const vb2_model* model, int32_t held, const double* fixed,
                                  const vb2_estimate* est, vb2_interval* out, int32_t* status, int64_t* num_step)
{
    if (num_step) *num_step = 0;
    if (!fn || !model || !est || !out || !status || num_hyp < 1 || num_pc < 1 || num_pc > VB2_MAX_PC || held < 0 || held > 2 ||
        (held != 0 && !fixed)) {
        set_error("vb2_paired_intervals_lockstep: invalid argument (held: 0 none, 1 pc1, 2 pc2, with its PCs)");
        return VB2_ERR_INVALID;
    }
    if (held != 0 && model->is_alpha_fixed) {
        set_error("vb2_paired_intervals_lockstep: a fixed alpha leaves the interval nothing to bound (--FixAlpha)");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        std::vector<vb2::IntervalOptions> opts((size_t)num_hyp);
        for (int h = 0; h < num_hyp && held != 0; ++h) {
            opts[(size_t)h].held = held;
            opts[(size_t)h].fixed = fixed + (size_t)h * num_pc;
            opts[(size_t)h].fold = false;
        }
        const vb2::BatchDerivsFn call = [fn, user](int32_t ns, const int32_t* np, const double* p1, const double* p2,
                                                   const double* a, double* llk, double* grad, double* hess) {
            const int rc = fn(user, ns, np, p1, p2, a, llk, grad, hess);
            if (rc) set_error("vb2_paired_intervals_lockstep: the evaluator failed");
            return rc;
        };
        return vb2::intervals_lockstep(num_hyp, num_pc, data_has_known_af, model, 1, est, call, out, status, num_step, nullptr,
                                       held != 0 ? opts.data() : nullptr);
    });
}

int vb2_debug_paired_time(vb2_paired* pair, int32_t num_point, int32_t warmup, int32_t reps, double* ms)
{
    if (!pair || !pair->impl) return VB2_ERR_INVALID;
    return pair->impl->time_launch(num_point, warmup, reps, ms);
}

// Measurement aid (tools/paired_interval_time.py; event-timed, milliseconds per repetition into ms[reps]): ONE single-sample
// launch pair of num_point <= kDerivChunk points (pc = 0.01, alpha = 0.03) -- given hypothesis hyp, or, hyp < 0, the anonymous
// pair of vb2_llk_derivs_batch on the set's context.
int vb2_debug_paired_derivs_time(vb2_paired* pair, int32_t hyp, int32_t num_point, int32_t warmup, int32_t reps, double* ms)
{
    if (!pair || !pair->impl || !ms || num_point < 1 || num_point > vb2::kDerivChunk || warmup < 0 || reps < 1 ||
        hyp >= pair->impl->num_row) {
        set_error("vb2_debug_paired_derivs_time: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Paired& c = *pair->impl;
        vb2::Context* ctx = c.ctx;
        if (ctx->resident_active || c.eval_pending()) {
            set_error("vb2_debug_paired_derivs_time: the context is busy");
            return VB2_ERR_INVALID;
        }
        if (const int rc = c.ensure_deriv_scratch()) return rc;
        if (const int rc = ctx->ensure_deriv_scratch()) return rc;
        const int k = ctx->num_pc, n = 2 * k + 1;
        // the context's own scratch holds the rows and the outputs of either launch ([chunk][vals][m_pad] | rows | outputs)
        double* const d_rows = ctx->d_deriv + (size_t)vb2::kDerivChunk * vb2::kDerivVals * (size_t)ctx->L.m_pad;
        double* const d_res = d_rows + (size_t)vb2::kDerivChunk * n;
        std::vector<double> rows((size_t)num_point * n, 0.01);
        for (int p = 0; p < num_point; ++p) rows[(size_t)p * n + 2 * k] = 0.03;
        hipStream_t s = ctx->stream;
        VB2_HIP(hipMemcpyAsync(d_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, s));
        VB2_HIP(hipStreamSynchronize(s));
        vb2::TimerEvents ev;
        VB2_HIP(hipEventCreate(&ev.a));
        VB2_HIP(hipEventCreate(&ev.b));
        for (int r = -warmup; r < reps; ++r) {
            VB2_HIP(hipEventRecord(ev.a, s));
            if (hyp < 0) VB2_HIP(vb2::launch_llk_derivs(ctx->L, num_point, d_rows, ctx->d_deriv, d_res, s));
            else VB2_HIP(vb2::launch_llk_pair_derivs(ctx->L, num_point, d_rows, c.hyp_planes(hyp), c.deriv_marker(hyp), d_res, s));
            VB2_HIP(hipEventRecord(ev.b, s));
            VB2_HIP(hipEventSynchronize(ev.b));
            float t = 0.0f;
            VB2_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
            if (r >= 0) ms[r] = (double)t;
        }
        return VB2_OK;
    });
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
