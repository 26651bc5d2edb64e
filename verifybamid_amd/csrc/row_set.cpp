// row_set.cpp -- see row_set.h
#include "row_set.h"

#include <algorithm>
#include <string>

#include "context.h"
#include "device_util.h"
#include "marker_sum_kernels.h"

namespace vb2 {

int RowSet::init(Context* c, int n, const char* who)
{
    if (!c || n < 1 || n > 65535) {
        set_error(std::string(who) + ": invalid argument (1..65535 " + kind_.rows_noun + ")");
        return VB2_ERR_INVALID;
    }
    if (c->resident_active) {
        set_error(std::string(who) + ": not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    ctx = c;
    num_row = n;
    const DeviceLayout& L = ctx->L;
    VB2_HIP(hipSetDevice(ctx->device));
    if (const int rc = ctx->ensure_pidx()) return rc;
    if (const int rc = take_device(std::max<size_t>(kind_.row_bytes(L) * (size_t)n, 256), ctx->device, &d_payload_, &d_payload_bytes_,
                                   kind_.nomem_who))
        return rc;
    if (const int rc = stage_.create(ctx, (size_t)n * VB2_BATCH_SLOTS,
                                     (size_t)kMaxPointsPerLaunch * (size_t)std::max(1, marker_sum_tile_groups(L)), kind_.nomem_who))
        return rc;
    device_bytes = (int64_t)(d_payload_bytes_ + stage_.device_bytes());
    launch_ = [this](int num_point, const double* d_rows, const int32_t* d_idx, double* d_partial, double* d_out, hipStream_t s) {
        return kind_.launch(ctx->L, num_point, d_rows, d_idx, d_payload_, d_partial, d_out, s);
    };
    return VB2_OK;
}

int RowSet::upload(const void* rows, size_t bytes, const char* what, const std::function<hipError_t(const void* d_panel)>& permute)
{
    void* d_panel = nullptr;
    size_t d_panel_bytes = 0;
    if (const int rc = take_device(std::max<size_t>(bytes, 256), ctx->device, &d_panel, &d_panel_bytes, kind_.nomem_who)) return rc;
    hipError_t e = hipMemcpyAsync(d_panel, rows, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = permute(d_panel);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    give_device(d_panel, d_panel_bytes, ctx->device);
    if (e != hipSuccess) {
        set_error(std::string(what) + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    return VB2_OK;
}

RowSet::~RowSet()
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // a begun evaluation reads the payload: it has to be over before the slab is given back, and the stage's own
    // destructor, which would wait for it as well, runs after this body
    (void)stage_.end(nullptr);
    give_device(d_payload_, d_payload_bytes_, ctx->device);
}

int RowSet::begin(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, bool have_llk)
{
    const auto refuse = [this](const std::string& what) {
        set_error(std::string(kind_.eval_who) + ": " + what);
        return VB2_ERR_INVALID;
    };
    if (!num_point || stage_.pending()) return refuse("invalid argument");
    size_t total = 0;
    if (!PointStage::count(num_row, num_point, &total))
        return refuse(std::string(kind_.count_noun) + " point count outside 0..VB2_BATCH_SLOTS");
    if (total == 0) return VB2_OK;
    if (!pc1 || !pc2 || !alpha || !have_llk) return refuse("invalid argument");
    if (ctx->resident_active) return refuse("not inside vb2_ctx_search_begin / vb2_ctx_search_end");
    // the synchronisation is end's
    return stage_.begin(num_row, num_point, total, pc1, pc2, alpha, launch_);
}

int RowSet::eval(const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk)
{
    const int rc = begin(num_point, pc1, pc2, alpha, llk || !kind_.llk_checked_first);
    if (rc) {
        (void)eval_end(nullptr);           // whatever reached the stream has left the stages when this returns
        return rc;
    }
    if (stage_.pending() && !llk) {
        (void)eval_end(nullptr);
        set_error(std::string(kind_.eval_who) + ": invalid argument");
        return VB2_ERR_INVALID;
    }
    return eval_end(llk);
}

namespace {
struct SetsStep {
    RowSet* const* sets;
    int num_set, k;
};
int sets_step(void* user, int32_t, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha, double* llk)
{
    const SetsStep* S = static_cast<const SetsStep*>(user);
    const int k = S->k;
    // begin every set with live points, then collect: sets on different contexts overlap on the device
    std::vector<size_t> at((size_t)S->num_set + 1, 0);
    int rc = VB2_OK, row = 0, begun = 0;
    for (int s = 0; s < S->num_set; ++s) {
        size_t n = 0;
        for (int h = 0; h < S->sets[s]->num_row; ++h) n += (size_t)num_point[row + h];
        at[(size_t)s + 1] = at[(size_t)s] + n;
        row += S->sets[s]->num_row;
    }
    row = 0;
    for (int s = 0; s < S->num_set && !rc; ++s) {
        const size_t o = at[(size_t)s];
        if (at[(size_t)s + 1] > o) rc = S->sets[s]->eval_begin(num_point + row, pc1 + o * k, pc2 + o * k, alpha + o);
        row += S->sets[s]->num_row;
        begun = s + 1;
    }
    for (int s = 0; s < begun; ++s) {
        const int re = S->sets[s]->eval_end(rc ? nullptr : llk + at[(size_t)s]);
        if (!rc) rc = re;
    }
    return rc;
}
}  // namespace

int optimize_row_sets(RowSet* const* sets, int num_set, Refit opt, const vb2_model& model, vb2_estimate* est, int32_t* status)
{
    const std::string who(opt.who);
    if (!sets || num_set < 1 || !opt.fixed || !est || !status) {
        set_error(who + ": invalid argument");
        return VB2_ERR_INVALID;
    }
    int R = 0;
    for (int s = 0; s < num_set; ++s) {
        if (!sets[s] || !sets[s]->ctx) {
            set_error(who + ": invalid argument");
            return VB2_ERR_INVALID;
        }
        if (sets[s]->ctx->num_pc != sets[0]->ctx->num_pc) {
            set_error(who + ": the sets' contexts differ in the number of PCs");
            return VB2_ERR_INVALID;
        }
        if (sets[s]->ctx->resident_active) {
            set_error(who + ": not inside vb2_ctx_search_begin / vb2_ctx_search_end");
            return VB2_ERR_INVALID;
        }
        for (int t = 0; t < s; ++t)
            if (sets[t] == sets[s]) {
                set_error(who + ": a set is listed twice");
                return VB2_ERR_INVALID;
            }
        R += sets[s]->num_row;
    }
    std::vector<uint8_t> kaf((size_t)R);
    std::vector<int32_t> fixed_row((size_t)R);
    int r = 0;
    for (int s = 0; s < num_set; ++s)
        for (int j = 0; j < sets[s]->num_row; ++j, ++r) {
            kaf[(size_t)r] = sets[s]->ctx->L.known_af != nullptr;
            fixed_row[(size_t)r] = s;
        }
    SetsStep S{sets, num_set, sets[0]->ctx->num_pc};
    opt.known_af = kaf.data();
    opt.fixed_row = fixed_row.data();
    return refit_lockstep(opt, sets_step, &S, R, S.k, model, est, status);
}

}  // namespace vb2
