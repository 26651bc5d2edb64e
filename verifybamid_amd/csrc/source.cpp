// source.cpp -- host side of --FindSource (source_kernels.hip) and --FindRelated (related_kernels.hip): Context::marginals,
// the set and its planes, its C entries and the <Output>.Sources / .Related / .SourceFit writers.
#include "source.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <new>

#include "device_util.h"
#include "related_kernels.h"
#include "source_kernels.h"

namespace vb2 {

int Context::ensure_pidx()
{
    if (d_pidx || L.num_active == 0) return VB2_OK;
    const size_t na = (size_t)L.num_active;
    if (h_perm.size() < na) {
        set_error("vb2_ctx_marginals: the context holds no marker order");
        return VB2_ERR_INVALID;
    }
    std::vector<int32_t> pidx(na);
    for (size_t m = 0; m < na; ++m) {
        const int64_t a = h_perm[m];
        pidx[m] = a >= 0 && (size_t)a < h_active.size() ? h_active[(size_t)a] : -1;
    }
    VB2_HIP(hipSetDevice(device));
    const size_t bytes = na * sizeof(int32_t);
    size_t got = 0;
    void* p = cached_device_slab(bytes, device, &got);
    if (!p) {
        VB2_HIP(hipMalloc(&p, bytes));
        got = bytes;
    }
    d_pidx = static_cast<int32_t*>(p);
    d_pidx_bytes = got;
    VB2_HIP(hipMemcpyAsync(d_pidx, pidx.data(), bytes, hipMemcpyHostToDevice, stream));
    VB2_HIP(hipStreamSynchronize(stream));          // (a pageable source: gone when this returns)
    return VB2_OK;
}

int Context::marginals(const double* pc1, const double* pc2, double alpha, double* contam_lik, double* geno_post, double* log_l,
                       float* d_row, double* own_lik, double* kin_post, const MarginalRelated* planes)
{
    if (!pc1 || !pc2) {
        set_error("vb2_ctx_marginals: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (resident_active) {
        set_error("vb2_ctx_marginals: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipSetDevice(device));
    const int k = num_pc;
    const size_t M = (size_t)num_marker;
    const bool want_host = contam_lik || geno_post || log_l;
    const bool want_rel = own_lik || kin_post;
    const bool related = want_rel || planes;          // the kernel's related instantiation (the caller zero-fills `planes`)
    if (d_row) VB2_HIP(hipMemsetAsync(d_row, 0, sizeof(float) * kSourceRowFloats * M, stream));
    // NaN parameters: no marker counts (context.h: params_hold_nan)
    const bool none = params_hold_nan(pc1, pc2, alpha, k, L.known_af != nullptr) || L.num_active == 0;
    double* d_c = nullptr;
    if (want_host && !none) {
        if (!d_marg) {
            const size_t bytes = 7 * M * sizeof(double);
            size_t got = 0;
            void* p = cached_device_slab(bytes, device, &got);
            if (!p) {
                VB2_HIP(hipMalloc(&p, bytes));
                got = bytes;
            }
            d_marg = p;
            d_marg_bytes = got;
        }
        d_c = static_cast<double*>(d_marg);
        VB2_HIP(hipMemsetAsync(d_c, 0, 7 * M * sizeof(double), stream));
    }
    double* d_r = nullptr;
    if (want_rel && !none) {
        if (!d_marg_rel) {
            const size_t bytes = 6 * M * sizeof(double);
            size_t got = 0;
            void* p = cached_device_slab(bytes, device, &got);
            if (!p) {
                VB2_HIP(hipMalloc(&p, bytes));
                got = bytes;
            }
            d_marg_rel = p;
            d_marg_rel_bytes = got;
        }
        d_r = static_cast<double*>(d_marg_rel);
        VB2_HIP(hipMemsetAsync(d_r, 0, 6 * M * sizeof(double), stream));
    }
    if (!none) {
        if (const int rc = ensure_pidx()) return rc;
        // the point travels through the context's mapped staging row (as eval_host's points do)
        std::memcpy(h_points, pc1, sizeof(double) * k);
        std::memcpy(h_points + k, pc2, sizeof(double) * k);
        h_points[2 * k] = alpha;
        if (related) {
            MarginalRelated rel;
            if (planes) rel = *planes;
            rel.own_lik = d_r;
            rel.kin_post = d_r ? d_r + 3 * M : nullptr;
            VB2_HIP(launch_related_marginals(L, num_marker, d_points, d_pidx, d_c, d_c ? d_c + 3 * M : nullptr,
                                               d_c ? d_c + 6 * M : nullptr, rel, stream));
        } else {
            VB2_HIP(launch_source_marginals(L, num_marker, d_points, d_pidx, d_c, d_c ? d_c + 3 * M : nullptr,
                                              d_c ? d_c + 6 * M : nullptr, d_row, stream));
        }
    }
    if (want_rel && !none) {
        if (own_lik) VB2_HIP(hipMemcpyAsync(own_lik, d_r, 3 * M * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (kin_post) VB2_HIP(hipMemcpyAsync(kin_post, d_r + 3 * M, 3 * M * sizeof(double), hipMemcpyDeviceToHost, stream));
    } else if (want_rel) {
        if (own_lik) std::memset(own_lik, 0, 3 * M * sizeof(double));
        if (kin_post) std::memset(kin_post, 0, 3 * M * sizeof(double));
    }
    if (want_host && !none) {
        if (contam_lik) VB2_HIP(hipMemcpyAsync(contam_lik, d_c, 3 * M * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (geno_post) VB2_HIP(hipMemcpyAsync(geno_post, d_c + 3 * M, 3 * M * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (log_l) VB2_HIP(hipMemcpyAsync(log_l, d_c + 6 * M, M * sizeof(double), hipMemcpyDeviceToHost, stream));
    } else if (want_host) {
        if (contam_lik) std::memset(contam_lik, 0, 3 * M * sizeof(double));
        if (geno_post) std::memset(geno_post, 0, 3 * M * sizeof(double));
        if (log_l) std::memset(log_l, 0, M * sizeof(double));
    }
    VB2_HIP(hipStreamSynchronize(stream));
    return VB2_OK;
}

int SourceSet::create(int num_marker, int capacity, int device, SourceSet** out, int planes)
{
    *out = nullptr;
    if (num_marker < 1 || capacity < 1 || planes < 1 || (planes & ~(VB2_SET_SOURCE | VB2_SET_RELATED))) {
        set_error("vb2_source_set_create: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (usable_device_count() < 1) {
        set_error("vb2_source_set_create: no usable gfx950 device");
        return VB2_ERR_NO_DEVICE;
    }
    std::unique_ptr<SourceSet> s(new SourceSet());
    if (device < 0) VB2_HIP(hipGetDevice(&device));
    VB2_HIP(hipSetDevice(device));
    s->device_ = device;
    s->num_marker_ = num_marker;
    s->capacity_ = capacity;
    s->rows_.assign((size_t)capacity, nullptr);
    // the planes a row holds, [num_marker][3] floats each, in the order c q h t: the source pair kernel finds c | q at the
    // row's start, the related one q | h | t from q_offset_ on
    s->planes_ = planes;
    const int num_plane = ((planes & VB2_SET_SOURCE) ? 2 : 1) + ((planes & VB2_SET_RELATED) ? 2 : 0);
    s->q_offset_ = (planes & VB2_SET_SOURCE) ? 3 * (size_t)num_marker : 0;
    s->row_floats_ = (size_t)num_plane * 3 * (size_t)num_marker;
    static_assert(kSourceRowFloats == 6, "a source-only row is c | q");
    const unsigned long long bytes = (unsigned long long)capacity * (unsigned long long)num_marker * (3ull * num_plane) * sizeof(float);
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (!known) (void)hipGetLastError();
    void* p = nullptr;
    if ((known && bytes > (unsigned long long)free_b) || hipMalloc(&p, (size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        char msg[256];
        std::snprintf(msg, sizeof(msg), "vb2_source_set_create: %d samples x %d markers need %llu bytes of device memory "
                      "(%llu free)", capacity, num_marker, bytes, (unsigned long long)free_b);
        set_error(msg);
        return VB2_ERR_NOMEM;
    }
    s->d_slab_ = static_cast<float*>(p);
    VB2_HIP(hipStreamCreateWithFlags(&s->stream_, hipStreamNonBlocking));
    *out = s.release();
    return VB2_OK;
}

SourceSet::~SourceSet()
{
    if (device_ >= 0) (void)hipSetDevice(device_);
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    if (d_slab_) (void)hipFree(d_slab_);
}

void SourceSet::set_count(int n)
{
    std::lock_guard<std::mutex> lk(mu_);
    n_ = std::max(n_, std::min(n, capacity_));
}

int SourceSet::count()
{
    std::lock_guard<std::mutex> lk(mu_);
    return n_;
}

int SourceSet::add(Context* ctx, const vb2_model& model, const vb2_estimate& est, int* index)
{
    int slot;
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (n_ >= capacity_) {
            set_error("vb2_source_set_add: the set is full");
            return VB2_ERR_INVALID;
        }
        slot = n_++;
    }
    if (index) *index = slot;
    return put(slot, ctx, model, est);
}

void search_point(const Context& ctx, const vb2_model& model, const vb2_estimate& est, std::vector<double>* p1,
                  std::vector<double>* p2, double* alpha)
{
    // the search's own point: the reported PCs with the reference's swap of indices 0, 1 undone (as interval.cpp) ...
    const int k = ctx.num_pc;
    const bool kaf = model.is_af_known != 0 || ctx.L.known_af != nullptr;
    const bool heter = model.is_heter && !kaf;
    p1->assign(est.pc, est.pc + k);
    p2->assign(est.pc2, est.pc2 + k);
    if (heter && est.alpha >= 0.5 && k >= 1) {
        std::swap((*p1)[0], (*p2)[0]);
        if (k >= 2) std::swap((*p1)[1], (*p2)[1]);
    }
    // ... mirrored when the fit put the larger share first: g1 is always the minor component
    if (est.alpha >= 0.5) p1->swap(*p2);
    if (alpha) *alpha = est.alpha >= 0.5 ? 1.0 - est.alpha : est.alpha;
}

int SourceSet::put(int slot, Context* ctx, const vb2_model& model, const vb2_estimate& est)
{
    if (slot < 0 || slot >= capacity_ || !ctx) {
        set_error("vb2_source_set_add: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (ctx->num_marker != num_marker_ || ctx->device != device_) {
        set_error("vb2_source_set_add: the context is of another panel size or on another device than the set");
        return VB2_ERR_INVALID;
    }
    std::vector<double> p1, p2;
    double alpha = 0;
    search_point(*ctx, model, est, &p1, &p2, &alpha);
    float* row = d_slab_ + (size_t)slot * row_floats_;
    if (planes_ == VB2_SET_SOURCE) {
        if (const int rc = ctx->marginals(p1.data(), p2.data(), alpha, nullptr, nullptr, nullptr, row)) return rc;
    } else {                // every plane the set has, from one launch
        VB2_HIP(hipSetDevice(device_));
        VB2_HIP(hipMemsetAsync(row, 0, sizeof(float) * row_floats_, ctx->stream));
        const MarginalRelated rel = planes_of(row);
        if (const int rc = ctx->marginals(p1.data(), p2.data(), alpha, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &rel))
            return rc;
    }
    std::lock_guard<std::mutex> lk(mu_);
    rows_[(size_t)slot] = row;
    n_ = std::max(n_, slot + 1);
    return VB2_OK;
}

MarginalRelated SourceSet::planes_of(float* row) const
{
    const size_t plane = 3 * (size_t)num_marker_;
    MarginalRelated rel;
    if (planes_ & VB2_SET_SOURCE) rel.c = row;
    rel.q = row + q_offset_;
    if (planes_ & VB2_SET_RELATED) {
        rel.h = row + q_offset_ + plane;
        rel.t = row + q_offset_ + 2 * plane;
    }
    return rel;
}

int SourceSet::relations(double* llr, int32_t* shared)
{
    if (!(planes_ & VB2_SET_RELATED)) {
        set_error("vb2_source_set_relations: the set was created without the related planes (VB2_SET_RELATED)");
        return VB2_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(mu_);
    const int n = n_;
    if (n == 0) return VB2_OK;
    VB2_HIP(hipSetDevice(device_));
    const size_t nn = (size_t)n * (size_t)n, np = related_partial_count(n, num_marker_);
    // [rows: n pointers][llr: 4 nn doubles][partial sums: 4 np doubles][shared: nn ints][partial counts: np ints]
    const size_t ptr_bytes = ((size_t)n * sizeof(float*) + 15) / 16 * 16;
    const size_t bytes = ptr_bytes + (nn + np) * kNumRelation * sizeof(double) + (nn + np) * sizeof(int32_t);
    char* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("vb2_source_set_relations: " + std::to_string(bytes) + " bytes of device scratch do not fit");
        return VB2_ERR_NOMEM;
    }
    const float** d_rows = reinterpret_cast<const float**>(d);
    double* d_llr = reinterpret_cast<double*>(d + ptr_bytes);
    double* d_pk = d_llr + nn * kNumRelation;
    int32_t* d_shared = reinterpret_cast<int32_t*>(d_pk + np * kNumRelation);
    int32_t* d_pn = d_shared + nn;
    hipError_t e = hipMemcpyAsync(d_rows, rows_.data(), (size_t)n * sizeof(float*), hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = launch_related_pairs(d_rows, q_offset_, n, num_marker_, d_pk, d_pn, d_llr, d_shared, stream_);
    if (e == hipSuccess && llr) e = hipMemcpyAsync(llr, d_llr, nn * kNumRelation * sizeof(double), hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess && shared) e = hipMemcpyAsync(shared, d_shared, nn * sizeof(int32_t), hipMemcpyDeviceToHost, stream_);
    const hipError_t es = hipStreamSynchronize(stream_);
    (void)hipFree(d);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        set_error(std::string("vb2_source_set_relations: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    return VB2_OK;
}

int SourceSet::scores(double* score, int32_t* shared)
{
    if (!(planes_ & VB2_SET_SOURCE)) {
        set_error("vb2_source_set_scores: the set was created without the source planes (VB2_SET_SOURCE)");
        return VB2_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(mu_);
    const int n = n_;
    if (n == 0) return VB2_OK;
    VB2_HIP(hipSetDevice(device_));
    const size_t nn = (size_t)n * (size_t)n, np = source_partial_count(n, num_marker_);
    // [rows: n pointers][score: nn doubles][partial sums: np doubles][shared: nn ints][partial counts: np ints]
    const size_t ptr_bytes = ((size_t)n * sizeof(float*) + 15) / 16 * 16;
    const size_t bytes = ptr_bytes + (nn + np) * sizeof(double) + (nn + np) * sizeof(int32_t);
    char* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("vb2_source_set_scores: " + std::to_string(bytes) + " bytes of device scratch do not fit");
        return VB2_ERR_NOMEM;
    }
    const float** d_rows = reinterpret_cast<const float**>(d);
    double* d_score = reinterpret_cast<double*>(d + ptr_bytes);
    double* d_ps = d_score + nn;
    int32_t* d_shared = reinterpret_cast<int32_t*>(d_ps + np);
    int32_t* d_pn = d_shared + nn;
    hipError_t e = hipMemcpyAsync(d_rows, rows_.data(), (size_t)n * sizeof(float*), hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) e = launch_source_pairs(d_rows, n, num_marker_, d_ps, d_pn, d_score, d_shared, stream_);
    if (e == hipSuccess && score) e = hipMemcpyAsync(score, d_score, nn * sizeof(double), hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess && shared) e = hipMemcpyAsync(shared, d_shared, nn * sizeof(int32_t), hipMemcpyDeviceToHost, stream_);
    const hipError_t es = hipStreamSynchronize(stream_);
    (void)hipFree(d);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        set_error(std::string("vb2_source_set_scores: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    return VB2_OK;
}

namespace {
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
}  // namespace

int SourceSet::time_pairs(int n, uint32_t seed, int warmup, int reps, double* ms, bool related)
{
    if (n < 1 || n > capacity_ || reps < 1 || warmup < 0 || !ms || !(planes_ & (related ? VB2_SET_RELATED : VB2_SET_SOURCE))) {
        set_error("time_pairs: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(mu_);
    VB2_HIP(hipSetDevice(device_));
    const size_t row_floats = row_floats_;
    // eight distinct rows, dealt to the slots in turn (the kernels' time does not depend on the values)
    std::vector<float> host(row_floats);
    uint32_t x = seed * 2654435761u + 1u;
    for (int v = 0; v < 8 && v < n; ++v) {
        for (size_t e = 0; e < row_floats; ++e) {
            x = x * 1664525u + 1013904223u;
            host[e] = (float)((x >> 8) & 0xffff) * (1.0f / 65536.0f) + 1e-3f;
        }
        VB2_HIP(hipMemcpy(d_slab_ + (size_t)v * row_floats, host.data(), row_floats * sizeof(float), hipMemcpyHostToDevice));
    }
    for (int sl = 8; sl < n; ++sl)
        VB2_HIP(hipMemcpy(d_slab_ + (size_t)sl * row_floats, d_slab_ + (size_t)(sl % 8) * row_floats, row_floats * sizeof(float),
                            hipMemcpyDeviceToDevice));
    for (int sl = 0; sl < n; ++sl) rows_[(size_t)sl] = d_slab_ + (size_t)sl * row_floats;
    n_ = std::max(n_, n);
    const size_t nn = (size_t)n * (size_t)n, np = source_partial_count(n, num_marker_);
    const size_t per = related ? kNumRelation : 1;          // doubles per pair
    const size_t ptr_bytes = ((size_t)n * sizeof(float*) + 15) / 16 * 16;
    const size_t bytes = ptr_bytes + (nn + np) * per * sizeof(double) + (nn + np) * sizeof(int32_t);
    char* d = nullptr;
    VB2_HIP(hipMalloc(reinterpret_cast<void**>(&d), bytes));
    const float** d_rows = reinterpret_cast<const float**>(d);
    double* d_score = reinterpret_cast<double*>(d + ptr_bytes);
    double* d_ps = d_score + nn * per;
    int32_t* d_shared = reinterpret_cast<int32_t*>(d_ps + np * per);
    int32_t* d_pn = d_shared + nn;
    EventPair ev;
    hipError_t e = hipMemcpy(d_rows, rows_.data(), (size_t)n * sizeof(float*), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&ev.a);
    if (e == hipSuccess) e = hipEventCreate(&ev.b);
    for (int r = -warmup; r < reps && e == hipSuccess; ++r) {
        e = hipEventRecord(ev.a, stream_);
        if (e == hipSuccess)
            e = related ? launch_related_pairs(d_rows, q_offset_, n, num_marker_, d_ps, d_pn, d_score, d_shared, stream_)
                        : launch_source_pairs(d_rows, n, num_marker_, d_ps, d_pn, d_score, d_shared, stream_);
        if (e == hipSuccess) e = hipEventRecord(ev.b, stream_);
        if (e == hipSuccess) e = hipEventSynchronize(ev.b);
        float t = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, ev.a, ev.b);
        if (r >= 0) ms[r] = (double)t;
    }
    (void)hipFree(d);
    if (e != hipSuccess) {
        set_error(std::string("time_pairs: ") + hipGetErrorString(e));
        return VB2_ERR_HIP;
    }
    return VB2_OK;
}

int SourceSet::time_marginals(Context* ctx, double alpha, int warmup, int reps, double* ms)
{
    if (!ctx || ctx->num_marker != num_marker_ || ctx->device != device_ || reps < 1 || warmup < 0 || !ms || ctx->resident_active) {
        set_error("time_marginals: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(mu_);      // (slot 0 is written: no add, no scores meanwhile; the row is not registered)
    VB2_HIP(hipSetDevice(device_));
    if (const int rc = ctx->ensure_pidx()) return rc;
    const int k = ctx->num_pc;
    for (int j = 0; j < 2 * k; ++j) ctx->h_points[j] = 0.01;
    ctx->h_points[2 * k] = alpha;
    EventPair ev;
    VB2_HIP(hipEventCreate(&ev.a));
    VB2_HIP(hipEventCreate(&ev.b));
    for (int r = -warmup; r < reps; ++r) {
        VB2_HIP(hipEventRecord(ev.a, ctx->stream));
        VB2_HIP(hipMemsetAsync(d_slab_, 0, sizeof(float) * row_floats_, ctx->stream));
        if (planes_ == VB2_SET_SOURCE)
            VB2_HIP(launch_source_marginals(ctx->L, num_marker_, ctx->d_points, ctx->d_pidx, nullptr, nullptr, nullptr, d_slab_,
                                              ctx->stream));
        else
            VB2_HIP(launch_related_marginals(ctx->L, num_marker_, ctx->d_points, ctx->d_pidx, nullptr, nullptr, nullptr,
                                               planes_of(d_slab_), ctx->stream));
        VB2_HIP(hipEventRecord(ev.b, ctx->stream));
        VB2_HIP(hipEventSynchronize(ev.b));
        float t = 0.0f;
        VB2_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
        if (r >= 0) ms[r] = (double)t;
    }
    return VB2_OK;
}

int write_sources(const std::string& prefix, int n, int top, const char* const* names, const vb2_run_result* res,
                  const int32_t* status, const double* score, const int32_t* shared)
{
    const std::string name(prefix + ".Sources");
    std::FILE* f = std::fopen(name.c_str(), "w");
    if (!f) {
        set_error("cannot write " + name);
        return VB2_ERR_IO;
    }
    std::fprintf(f, "#SAMPLE\tFREEMIX\tRANK\tCANDIDATE\tLLR\tMARKERS\n");
    std::vector<int> order;
    for (int i = 0; i < n; ++i) {
        if (status[i] != VB2_OK) {          // never searched: no estimate, no candidates
            std::fprintf(f, "%s\t%g\t%d\t%s\t%g\t%d\n", names[i], std::numeric_limits<double>::quiet_NaN(), 1, "NA",
                         std::numeric_limits<double>::quiet_NaN(), 0);
            continue;
        }
        const double a = res[i].est.alpha, freemix = a < 0.5 ? a : 1 - a;
        order.clear();
        for (int j = 0; j < n; ++j)
            if (j != i && !std::isnan(score[(size_t)i * n + j])) order.push_back(j);
        std::stable_sort(order.begin(), order.end(),
                         [&](int x, int y) { return score[(size_t)i * n + x] > score[(size_t)i * n + y]; });
        const int lim = std::min<int>(top, (int)order.size());
        for (int r = 0; r < lim; ++r) {
            const int j = order[(size_t)r];
            std::fprintf(f, "%s\t%g\t%d\t%s\t%g\t%d\n", names[i], freemix, r + 1, names[j], score[(size_t)i * n + j],
                         (int)shared[(size_t)i * n + j]);
        }
    }
    if (std::fclose(f) != 0) {
        set_error("cannot write " + name);
        return VB2_ERR_IO;
    }
    return VB2_OK;
}

int write_related(const std::string& prefix, int n, int top, const char* const* names, const int32_t* status, const double* llr,
                  const int32_t* shared)
{
    static const char* const kName[VB2_NUM_RELATION] = {"DUP", "PO", "FS", "D2"};
    const std::string name(prefix + ".Related");
    std::FILE* f = std::fopen(name.c_str(), "w");
    if (!f) {
        set_error("cannot write " + name);
        return VB2_ERR_IO;
    }
    std::fprintf(f, "#SAMPLE\tPARTNER\tRANK\tRELATION\tLLR\tLLR_DUP\tLLR_PO\tLLR_FS\tLLR_D2\tMARKERS\n");
    std::vector<int> order, best((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (status[i] != VB2_OK) continue;          // never searched: absent
        order.clear();
        for (int j = 0; j < n; ++j) {
            const double* k = llr + ((size_t)i * n + j) * VB2_NUM_RELATION;
            if (j == i || std::isnan(k[0])) continue;
            int b = 0;
            for (int r = 1; r < VB2_NUM_RELATION; ++r)
                if (k[r] > k[b]) b = r;
            best[(size_t)j] = b;
            order.push_back(j);
        }
        const auto top_of = [&](int j) { return llr[((size_t)i * n + j) * VB2_NUM_RELATION + best[(size_t)j]]; };
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return top_of(x) > top_of(y); });
        const int lim = std::min<int>(top, (int)order.size());
        for (int r = 0; r < lim; ++r) {
            const int j = order[(size_t)r];
            const double* k = llr + ((size_t)i * n + j) * VB2_NUM_RELATION;
            std::fprintf(f, "%s\t%s\t%d\t%s\t%g\t%g\t%g\t%g\t%g\t%d\n", names[i], names[j], r + 1,
                         top_of(j) > 0 ? kName[best[(size_t)j]] : "UN", top_of(j), k[0], k[1], k[2], k[3], (int)shared[(size_t)i * n + j]);
        }
    }
    if (std::fclose(f) != 0) {
        set_error("cannot write " + name);
        return VB2_ERR_IO;
    }
    return VB2_OK;
}

int write_source_fit(const std::string& prefix, int n, const char* const* names, const vb2_source_fit* fit)
{
    const std::string name(prefix + ".SourceFit");
    std::FILE* f = std::fopen(name.c_str(), "w");
    if (!f) {
        set_error("cannot write " + name);
        return VB2_ERR_IO;
    }
    std::fprintf(f, "#SAMPLE\tCANDIDATE\tLLR\tMARKERS\tFREEMIX\tFREELK1\tALPHA_GIVEN\tLK1_GIVEN\tLK0_GIVEN\tDELTA_LK\n");
    for (int i = 0; i < n; ++i) {
        const vb2_source_fit& s = fit[i];
        if (s.candidate < 0 || s.candidate >= n) continue;
        std::fprintf(f, "%s\t%s\t%g\t%d\t%g\t%g", names[i], names[s.candidate], s.llr, (int)s.markers, s.freemix, s.freelk1);
        if (s.status == VB2_OK) std::fprintf(f, "\t%g\t%g\t%g\t%g\n", s.alpha_given, s.lk1_given, s.lk0_given, s.delta_lk);
        else std::fprintf(f, "\tNA\tNA\tNA\tNA\n");
    }
    if (std::fclose(f) != 0) {
        set_error("cannot write " + name);
        return VB2_ERR_IO;
    }
    return VB2_OK;
}

}  // namespace vb2

using vb2::set_error;

extern "C" {

int vb2_ctx_marginals(vb2_ctx* ctx, const double* pc1, const double* pc2, double alpha, double* contam_lik, double* geno_post,
                      double* log_l)
{
    if (!ctx || !ctx->impl) {
        set_error("vb2_ctx_marginals: invalid context");
        return VB2_ERR_INVALID;
    }
    try {
        return ctx->impl->marginals(pc1, pc2, alpha, contam_lik, geno_post, log_l, nullptr);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

int vb2_source_set_create_ex(int32_t num_marker, int32_t capacity, int32_t device, int32_t planes, vb2_source_set** out)
{
    if (!out) {
        set_error("vb2_source_set_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    try {
        vb2::SourceSet* s = nullptr;
        if (const int rc = vb2::SourceSet::create(num_marker, capacity, device, &s, planes)) return rc;
        *out = new vb2_source_set{s};
        return VB2_OK;
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

int vb2_source_set_create(int32_t num_marker, int32_t capacity, int32_t device, vb2_source_set** out)
{
    return vb2_source_set_create_ex(num_marker, capacity, device, VB2_SET_SOURCE, out);
}

int vb2_source_set_relations(vb2_source_set* set, double* llr, int32_t* shared)
{
    if (!set || !set->impl) {
        set_error("vb2_source_set_relations: invalid argument");
        return VB2_ERR_INVALID;
    }
    try {
        return set->impl->relations(llr, shared);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

int vb2_ctx_marginals_related(vb2_ctx* ctx, const double* pc1, const double* pc2, double alpha, double* own_lik, double* kin_post)
{
    if (!ctx || !ctx->impl) {
        set_error("vb2_ctx_marginals_related: invalid context");
        return VB2_ERR_INVALID;
    }
    try {
        return ctx->impl->marginals(pc1, pc2, alpha, nullptr, nullptr, nullptr, nullptr, own_lik, kin_post);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

// measurement aid (not in vb2_abi.h): tools/related_time.py
int vb2_debug_related_time_pairs(vb2_source_set* set, int32_t n, uint32_t seed, int32_t warmup, int32_t reps, double* ms)
{
    if (!set || !set->impl) return VB2_ERR_INVALID;
    try {
        return set->impl->time_pairs(n, seed, warmup, reps, ms, true);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

int vb2_source_set_add(vb2_source_set* set, vb2_ctx* ctx, const vb2_model* model, const vb2_estimate* est, int32_t* index)
{
    if (!set || !set->impl || !ctx || !ctx->impl || !model || !est) {
        set_error("vb2_source_set_add: invalid argument");
        return VB2_ERR_INVALID;
    }
    try {
        int idx = -1;
        const int rc = set->impl->add(ctx->impl, *model, *est, &idx);
        if (index) *index = idx;
        return rc;
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

int vb2_source_set_scores(vb2_source_set* set, double* score, int32_t* shared)
{
    if (!set || !set->impl) {
        set_error("vb2_source_set_scores: invalid argument");
        return VB2_ERR_INVALID;
    }
    try {
        return set->impl->scores(score, shared);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

// measurement aids (not in vb2_abi.h): tools/source_time.py
int vb2_debug_source_time_pairs(vb2_source_set* set, int32_t n, uint32_t seed, int32_t warmup, int32_t reps, double* ms)
{
    if (!set || !set->impl) return VB2_ERR_INVALID;
    try {
        return set->impl->time_pairs(n, seed, warmup, reps, ms);
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    }
}

int vb2_debug_source_time_marginals(vb2_source_set* set, vb2_ctx* ctx, double alpha, int32_t warmup, int32_t reps, double* ms)
{
    if (!set || !set->impl || !ctx || !ctx->impl) return VB2_ERR_INVALID;
    return set->impl->time_marginals(ctx->impl, alpha, warmup, reps, ms);
}

int vb2_source_set_size(vb2_source_set* set, int32_t* n)
{
    if (!set || !set->impl || !n) {
        set_error("vb2_source_set_size: invalid argument");
        return VB2_ERR_INVALID;
    }
    *n = set->impl->count();
    return VB2_OK;
}

void vb2_source_set_destroy(vb2_source_set* set)
{
    if (!set) return;
    delete set->impl;
    delete set;
}

}  // extern "C"
