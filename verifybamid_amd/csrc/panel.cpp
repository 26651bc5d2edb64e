// panel.cpp -- the --RefVCF panel builder behind vb2_panel_* / vb2_vcf_* (include/vb2_abi.h section 4):
// SVDcalculator::ProcessRefVCF (SVDcalculator.cpp:363-400) and WriteSVD (:471-513) with the decomposition on the GPU.
//
// Flow: the reader (vcf_panel.cpp) hands kept markers over block by block; they collect in a pinned staging chunk of
// `chunk_markers` markers (marker-major), which is copied to the device and there transposed into its own
// sample-major slab chunk, summed per marker (mu) and multiplied into the exact int32 Gram S -- while the reader goes
// on.  The minimums (>= 5000 markers, >= 1000 samples) are settled before the first device call: markers stay on the
// host until 5000 are kept.  After the last chunk: c = G^T mu and tau = mu^T mu per chunk in a fixed order, the
// centred Gram C in FP64, rocSOLVER dsyevd (librocsolver bound with dlopen on first use, so ordinary runs never load
// it), the sign convention on the host, and UD = G V - mu (1^T V) from the resident slab.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <rocblas/rocblas.h>        // types only: the libraries are bound with dlopen below
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "context.h"
#include "guard.h"
#include "panel.h"

struct vb2_vcf {
    vb2::VcfMarkers mk;
    std::vector<int8_t> geno;
    std::vector<const char*> chr_ptrs, sample_ptrs;
};

struct vb2_panel {
    bool has_markers = false;
    vb2::VcfMarkers mk;
    int64_t M = 0;
    int32_t N = 0, k = 0;
    std::vector<double> ud, v, mu, sigma;
    std::vector<int32_t> gram, row_sum;
    double seconds[7] = {0, 0, 0, 0, 0, 0, 0};
    double seconds_total = 0;
};

namespace vb2 {

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

constexpr int64_t kMinMarkers = 5000;
constexpr int32_t kMinSamples = 1000;
constexpr int64_t kMaxExactMarkers = 500000000;   // 4 * M < 2^31: S stays exact in int32 (|g| <= 2)

enum Stage { kParse, kUpload, kGram, kCentre, kEig, kProject, kWrite };

// ---- rocSOLVER / rocBLAS, bound on first use ----
struct Solver {
    decltype(&rocblas_create_handle) create_handle = nullptr;
    decltype(&rocblas_destroy_handle) destroy_handle = nullptr;
    decltype(&rocblas_set_stream) set_stream = nullptr;
    decltype(&rocsolver_dsyevd) dsyevd = nullptr;
    bool ok = false;
    std::string why;
};

Solver& solver()
{
    static Solver s;
    static std::once_flag once;
    std::call_once(once, [] {
        // prefer the rocSOLVER that sits beside the HIP runtime this process already uses (a PyTorch wheel ships its
        // own runtime and its own rocSOLVER: one runtime per process), then the loader's search, then /opt/rocm
        std::vector<std::string> names;
        Dl_info di;
        if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &di) && di.dli_fname) {
            std::string dir(di.dli_fname);
            const size_t sl = dir.rfind('/');
            if (sl != std::string::npos) {
                dir.resize(sl);
                names.push_back(dir + "/librocsolver.so.0");
                names.push_back(dir + "/librocsolver.so");
            }
        }
        names.push_back("librocsolver.so.0");
        names.push_back("librocsolver.so");
        names.push_back("/opt/rocm/lib/librocsolver.so.0");
        void* h = nullptr;
        std::string last;
        for (const std::string& n : names) {
            h = dlopen(n.c_str(), RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
            const char* e = dlerror();
            last = e ? e : n;
        }
        if (!h) {
            s.why = "librocsolver not loadable (needed by the panel builder's eigensolver): " + last;
            return;
        }
#define VB2_SOLVER_SYM(field, sym)                                        \
    s.field = reinterpret_cast<decltype(s.field)>(dlsym(h, sym));         \
    if (!s.field) { s.why = std::string("librocsolver/rocblas lacks ") + sym; return; }
        VB2_SOLVER_SYM(create_handle, "rocblas_create_handle")
        VB2_SOLVER_SYM(destroy_handle, "rocblas_destroy_handle")
        VB2_SOLVER_SYM(set_stream, "rocblas_set_stream")
        VB2_SOLVER_SYM(dsyevd, "rocsolver_dsyevd")
#undef VB2_SOLVER_SYM
        s.ok = true;
    });
    return s;
}

struct HipFail {
    int code;
};

void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        set_error(std::string("panel builder: ") + what + ": " + hipGetErrorString(e));
        throw HipFail{VB2_ERR_HIP};
    }
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// the device half: chunks of the slab, S, the per-marker sums and means
class Builder {
public:
    Builder(int32_t n, int64_t chunk, int device) : n_(n), n_pad_((int32_t)round_up(n, kGramTile)), cw_(chunk), dev_(device) {}
    ~Builder() { release(); }

    // first device call of a build
    int start()
    {
        if (usable_device_count() < 1) {
            set_error("panel builder: no gfx950 device is visible; the decomposition runs on the GPU only "
                      "(there is no CPU fallback)");
            return VB2_ERR_NO_DEVICE;
        }
        if (dev_ >= 0) hip_check(hipSetDevice(dev_), "hipSetDevice");
        hip_check(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking), "hipStreamCreate");
        started_ = true;      // from here on release() has something to free
        const size_t sb = (size_t)n_pad_ * n_pad_ * sizeof(int32_t);
        if (hipMalloc(&d_S_, sb) != hipSuccess) {
            (void)hipGetLastError();
            set_error("panel builder: the " + std::to_string(n_) + " x " + std::to_string(n_) +
                      " Gram matrix does not fit in device memory");
            throw HipFail{VB2_ERR_NOMEM};
        }
        hip_check(hipMemsetAsync(d_S_, 0, sb, st_), "hipMemset(S)");
        hip_check(hipMalloc(&d_c_, (size_t)n_pad_ * sizeof(double)), "hipMalloc(c)");
        hip_check(hipMemsetAsync(d_c_, 0, (size_t)n_pad_ * sizeof(double), st_), "hipMemset(c)");
        hip_check(hipMalloc(&d_tau_, sizeof(double)), "hipMalloc(tau)");
        hip_check(hipMemsetAsync(d_tau_, 0, sizeof(double), st_), "hipMemset(tau)");
        hip_check(hipMalloc(&d_raw_, (size_t)cw_ * n_), "hipMalloc(staging)");
        for (int b = 0; b < 2; ++b) {
            hip_check(hipHostMalloc(&h_stage_[b], (size_t)cw_ * n_, hipHostMallocDefault), "hipHostMalloc");
            hip_check(hipEventCreate(&ev_stage_[b]), "hipEventCreate");
            hip_check(hipEventRecord(ev_stage_[b], st_), "hipEventRecord");   // "staging buffer free"
        }
        return VB2_OK;
    }

    bool started() const { return started_; }

    // append marker-major rows; full chunks go to the device
    void push(const int8_t* rows, int64_t count)
    {
        while (count > 0) {
            if (fill_ == 0) hip_check(hipEventSynchronize(ev_stage_[cur_]), "hipEventSynchronize");
            const int64_t take = std::min(count, cw_ - fill_);
            std::memcpy(h_stage_[cur_] + (size_t)fill_ * n_, rows, (size_t)take * n_);
            fill_ += take;
            rows += (size_t)take * n_;
            count -= take;
            if (fill_ == cw_) flush();
        }
    }

    void flush()
    {
        if (fill_ == 0) return;
        if (total_ + fill_ >= kMaxExactMarkers) {
            set_error("panel builder: more than 5e8 markers; the int32 Gram would no longer be exact");
            throw HipFail{VB2_ERR_INVALID};
        }
        Chunk ch;
        ch.count = fill_;
        const size_t slab_bytes = (size_t)n_pad_ * cw_;
        if (hipMalloc(&ch.slab, slab_bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("panel builder: the genotype slab (" + std::to_string(n_) + " samples x " +
                      std::to_string(total_ + fill_) + "+ markers, one byte each) does not fit in device memory; "
                      "panels larger than the device are not supported");
            throw HipFail{VB2_ERR_NOMEM};
        }
        chunks_.push_back(ch);
        Chunk& c = chunks_.back();
        hip_check(hipMalloc(&c.sums, (size_t)cw_ * sizeof(int32_t)), "hipMalloc(sums)");
        hip_check(hipMalloc(&c.mu, (size_t)cw_ * sizeof(double)), "hipMalloc(mu)");
        hip_check(hipMemsetAsync(c.slab, 0, slab_bytes, st_), "hipMemset(slab)");
        hip_check(hipMemsetAsync(c.sums, 0, (size_t)cw_ * sizeof(int32_t), st_), "hipMemset(sums)");
        hip_check(hipMemsetAsync(c.mu, 0, (size_t)cw_ * sizeof(double), st_), "hipMemset(mu)");
        Timed up = timed(kUpload);
        hip_check(hipMemcpyAsync(d_raw_, h_stage_[cur_], (size_t)fill_ * n_, hipMemcpyHostToDevice, st_), "upload");
        hip_check(hipEventRecord(ev_stage_[cur_], st_), "hipEventRecord");
        end(up);
        Timed gr = timed(kGram);
        hip_check(launch_transpose_chunk(d_raw_, fill_, n_, c.slab, cw_, st_), "transpose kernel");
        hip_check(launch_row_sums(d_raw_, fill_, n_, c.sums, st_), "row-sum kernel");
        hip_check(launch_gram_chunk(c.slab, cw_, cw_, n_pad_, d_S_, st_), "Gram kernel");
        end(gr);
        Timed ce = timed(kCentre);
        hip_check(launch_mu_from_sums(c.sums, fill_, n_, c.mu, st_), "mean kernel");
        hip_check(launch_sample_dot_mu(c.slab, cw_, cw_, n_, c.mu, d_c_, st_), "c kernel");
        hip_check(launch_sum_squares(c.mu, cw_, d_tau_, st_), "tau kernel");
        end(ce);
        total_ += fill_;
        fill_ = 0;
        cur_ ^= 1;
    }

    void finish(vb2_panel* p, int num_svd_pcs)
    {
        flush();
        const int64_t M = total_;
        const int32_t N = n_;
        p->M = M;
        p->N = N;
        // S (mirrored from its lower tiles) and the per-marker sums and means
        hip_check(hipStreamSynchronize(st_), "the Gram chunks");
        std::vector<int32_t> Sp((size_t)n_pad_ * n_pad_);
        hip_check(hipMemcpy(Sp.data(), d_S_, Sp.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "download S");
        p->gram.resize((size_t)N * N);
        for (int32_t i = 0; i < N; ++i)
            for (int32_t j = 0; j < N; ++j)
                p->gram[(size_t)i * N + j] = (i / kGramTile >= j / kGramTile) ? Sp[(size_t)i * n_pad_ + j] : Sp[(size_t)j * n_pad_ + i];
        p->row_sum.resize((size_t)M);
        p->mu.resize((size_t)M);
        int64_t off = 0;
        for (const Chunk& c : chunks_) {
            hip_check(hipMemcpy(p->row_sum.data() + off, c.sums, (size_t)c.count * sizeof(int32_t), hipMemcpyDeviceToHost), "download sums");
            hip_check(hipMemcpy(p->mu.data() + off, c.mu, (size_t)c.count * sizeof(double), hipMemcpyDeviceToHost), "download mu");
            off += c.count;
        }

        // centred Gram, eigendecomposition
        Timed ce = timed(kCentre);
        double* d_C = nullptr;
        hip_check(hipMalloc(&d_C, (size_t)N * N * sizeof(double)), "hipMalloc(C)");
        dev_ptrs_.push_back(d_C);
        hip_check(launch_centre_gram(d_S_, n_pad_, N, d_c_, d_tau_, d_C, st_), "centring kernel");
        end(ce);
        Solver& so = solver();
        if (!so.ok) {
            set_error(so.why);
            throw HipFail{VB2_ERR_NO_DEVICE};
        }
        Timed eg = timed(kEig);
        double *d_W = nullptr, *d_E = nullptr;
        int* d_info = nullptr;
        hip_check(hipMalloc(&d_W, (size_t)N * sizeof(double)), "hipMalloc(W)");
        dev_ptrs_.push_back(d_W);
        hip_check(hipMalloc(&d_E, (size_t)N * sizeof(double)), "hipMalloc(E)");
        dev_ptrs_.push_back(d_E);
        hip_check(hipMalloc(&d_info, sizeof(int)), "hipMalloc(info)");
        dev_ptrs_.push_back(d_info);
        rocblas_handle h = nullptr;
        if (so.create_handle(&h) != rocblas_status_success) {
            set_error("panel builder: rocblas_create_handle failed");
            throw HipFail{VB2_ERR_HIP};
        }
        so.set_stream(h, st_);
        const rocblas_status rs = so.dsyevd(h, rocblas_evect_original, rocblas_fill_lower, N, d_C, N, d_W, d_E, d_info);
        end(eg);
        hip_check(hipStreamSynchronize(st_), "eigensolver");
        so.destroy_handle(h);
        int info = 0;
        hip_check(hipMemcpy(&info, d_info, sizeof(int), hipMemcpyDeviceToHost), "download info");
        if (rs != rocblas_status_success || info != 0) {
            set_error("panel builder: Gram matrix eigendecomposition failed to converge (rocsolver_dsyevd status " +
                      std::to_string((int)rs) + ", info " + std::to_string(info) + ")");
            throw HipFail{VB2_ERR_HIP};
        }
        std::vector<double> W((size_t)N);
        hip_check(hipMemcpy(W.data(), d_W, (size_t)N * sizeof(double), hipMemcpyDeviceToHost), "download eigenvalues");
        p->sigma.resize((size_t)N);
        for (int32_t i = 0; i < N; ++i) p->sigma[i] = std::sqrt(std::max(W[(size_t)(N - 1 - i)], 0.0));

        const int64_t maxPCs = std::min<int64_t>(M, N);
        const int32_t k = (int32_t)(num_svd_pcs > 0 ? std::min<int64_t>(num_svd_pcs, maxPCs) : maxPCs);
        p->k = k;
        // the top k eigenvectors, descending; sign: the entry of largest magnitude positive, lowest index on ties
        std::vector<double> Vall((size_t)N * k);
        for (int32_t q = 0; q < k; ++q)
            hip_check(hipMemcpy(Vall.data() + (size_t)q * N, d_C + (size_t)(N - 1 - q) * N, (size_t)N * sizeof(double),
                                hipMemcpyDeviceToHost), "download eigenvectors");
        p->v.resize((size_t)N * k);
        for (int32_t q = 0; q < k; ++q) {
            const double* col = Vall.data() + (size_t)q * N;
            int32_t best = 0;
            for (int32_t j = 1; j < N; ++j)
                if (std::fabs(col[j]) > std::fabs(col[best])) best = j;
            const double sgn = col[best] < 0 ? -1.0 : 1.0;
            for (int32_t j = 0; j < N; ++j) p->v[(size_t)j * k + q] = sgn * col[j];
        }
        std::vector<double> vsum((size_t)k, 0.0);
        for (int32_t j = 0; j < N; ++j)
            for (int32_t q = 0; q < k; ++q) vsum[q] += p->v[(size_t)j * k + q];

        // projection from the resident slab
        double *d_V = nullptr, *d_vsum = nullptr, *d_UD = nullptr;
        hip_check(hipMalloc(&d_V, p->v.size() * sizeof(double)), "hipMalloc(V)");
        dev_ptrs_.push_back(d_V);
        hip_check(hipMalloc(&d_vsum, (size_t)k * sizeof(double)), "hipMalloc(vsum)");
        dev_ptrs_.push_back(d_vsum);
        hip_check(hipMalloc(&d_UD, (size_t)cw_ * k * sizeof(double)), "hipMalloc(UD)");
        dev_ptrs_.push_back(d_UD);
        hip_check(hipMemcpy(d_V, p->v.data(), p->v.size() * sizeof(double), hipMemcpyHostToDevice), "upload V");
        hip_check(hipMemcpy(d_vsum, vsum.data(), (size_t)k * sizeof(double), hipMemcpyHostToDevice), "upload vsum");
        p->ud.resize((size_t)M * k);
        off = 0;
        for (const Chunk& c : chunks_) {
            Timed pj = timed(kProject);
            hip_check(launch_project(c.slab, cw_, cw_, N, d_V, k, c.mu, d_vsum, d_UD, st_), "projection kernel");
            end(pj);
            hip_check(hipMemcpyAsync(p->ud.data() + (size_t)off * k, d_UD, (size_t)c.count * k * sizeof(double),
                                     hipMemcpyDeviceToHost, st_), "download UD");
            hip_check(hipStreamSynchronize(st_), "projection");
            off += c.count;
        }
        hip_check(hipStreamSynchronize(st_), "panel builder");
        for (const auto& t : timers_) {
            float ms = 0.f;
            hip_check(hipEventElapsedTime(&ms, t.a, t.b), "hipEventElapsedTime");
            p->seconds[t.stage] += ms * 1e-3;
        }
    }

    int64_t total() const { return total_ + fill_; }

private:
    struct Chunk {
        int8_t* slab = nullptr;
        int32_t* sums = nullptr;
        double* mu = nullptr;
        int64_t count = 0;
    };
    struct Timed {
        int stage;
        hipEvent_t a, b;
    };
    Timed timed(int stage)
    {
        Timed t{stage, nullptr, nullptr};
        hip_check(hipEventCreate(&t.a), "hipEventCreate");
        hip_check(hipEventCreate(&t.b), "hipEventCreate");
        hip_check(hipEventRecord(t.a, st_), "hipEventRecord");
        return t;
    }
    void end(const Timed& t)
    {
        hip_check(hipEventRecord(t.b, st_), "hipEventRecord");
        timers_.push_back(t);
    }
    void release()
    {
        if (!started_) return;
        (void)hipStreamSynchronize(st_);
        for (auto& t : timers_) {
            (void)hipEventDestroy(t.a);
            (void)hipEventDestroy(t.b);
        }
        for (Chunk& c : chunks_) {
            (void)hipFree(c.slab);
            (void)hipFree(c.sums);
            (void)hipFree(c.mu);
        }
        for (void* q : dev_ptrs_) (void)hipFree(q);
        (void)hipFree(d_S_);
        (void)hipFree(d_c_);
        (void)hipFree(d_tau_);
        (void)hipFree(d_raw_);
        for (int b = 0; b < 2; ++b) {
            if (h_stage_[b]) (void)hipHostFree(h_stage_[b]);
            if (ev_stage_[b]) (void)hipEventDestroy(ev_stage_[b]);
        }
        (void)hipStreamDestroy(st_);
        (void)hipGetLastError();
    }

    int32_t n_, n_pad_;
    int64_t cw_;
    int dev_;
    bool started_ = false;
    hipStream_t st_ = nullptr;
    int32_t* d_S_ = nullptr;
    double *d_c_ = nullptr, *d_tau_ = nullptr;
    int8_t* d_raw_ = nullptr;
    int8_t* h_stage_[2] = {nullptr, nullptr};
    hipEvent_t ev_stage_[2] = {nullptr, nullptr};
    int cur_ = 0;
    int64_t fill_ = 0, total_ = 0;
    std::vector<Chunk> chunks_;
    std::vector<void*> dev_ptrs_;
    std::vector<Timed> timers_;
};

// ProcessRefVCF :371-388
int check_minimums(int64_t M, int32_t N, bool skip, bool notices)
{
    if (M < kMinMarkers) {
        set_error("Insufficient number of markers (need >= 5000, have " + std::to_string(M) + ")");
        return VB2_ERR_INVALID;
    }
    if (N < kMinSamples) {
        if (skip) {
            if (notices)
                std::fprintf(stderr, "WARNING - Only %d individuals in reference panel (recommended minimum is 1000). "
                                     "Proceeding because --SkipMinSampleCountCheck is set. Contamination estimates may be "
                                     "unreliable if the panel does not adequately capture population structure.\n", (int)N);
        } else {
            set_error("Insufficient number of individuals (need >= 1000, have " + std::to_string(N) +
                      "). If your reference panel adequately captures population structure with fewer samples, rerun "
                      "with --SkipMinSampleCountCheck.");
            return VB2_ERR_INVALID;
        }
    }
    return VB2_OK;
}

// logVarianceExplained (:231-256) over the full spectrum
void log_variance_explained(const std::vector<double>& sv)
{
    double total = 0.0;
    const int n = (int)sv.size();
    for (int i = 0; i < n; ++i) total += sv[i] * sv[i];
    const int shown = std::min(n, 20);
    if (total <= 0.0) {
        std::fprintf(stderr, "WARNING - Total variance is zero; skipping variance-explained logging.\n");
        return;
    }
    double cum = 0.0;
    for (int i = 0; i < shown; ++i) {
        const double ve = sv[i] * sv[i] / total;
        cum += ve;
        std::fprintf(stderr, "NOTICE -   PC%d: singular_value=%.4f  variance_explained=%.4f (%.2f%%)  cumulative=%.4f (%.2f%%)\n",
                     i + 1, sv[i], ve, ve * 100.0, cum, cum * 100.0);
    }
    if (n > shown) std::fprintf(stderr, "NOTICE -   ... (%d more components not shown)\n", n - shown);
}

int64_t chunk_width(const vb2_panel_args* a)
{
    const int64_t c = a->chunk_markers > 0 ? a->chunk_markers : 16384;
    return round_up(c, kGramKStep);
}

// guard.h's clauses around a body that may also throw HipFail (its code; the message is set where it is thrown)
template <class F>
int entry(F&& f)
{
    return guarded([&]() -> int {
        try {
            return f();
        } catch (const HipFail& e) {
            return e.code;
        }
    });
}

}  // namespace

}  // namespace vb2

using vb2::set_error;

extern "C" {

int vb2_vcf_read(const vb2_panel_args* a, vb2_vcf** out)
{
    if (!a || !a->vcf_path || !out) {
        set_error("vb2_vcf_read: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return vb2::entry([&] {
        std::unique_ptr<vb2_vcf> v(new vb2_vcf);
        const auto inc = vb2::parse_include_chr(a->include_chr);
        const int rc = vb2::read_vcf(a->vcf_path, inc, a->num_thread, a->notices != 0, &v->mk, nullptr,
                                     [&](const int8_t* b, int64_t, int64_t n) {
                                         v->geno.insert(v->geno.end(), b, b + (size_t)n * v->mk.num_sample);
                                         return (int)VB2_OK;
                                     });
        if (rc != VB2_OK) return rc;
        for (const auto& s : v->mk.chr_names) v->chr_ptrs.push_back(s.c_str());
        for (const auto& s : v->mk.samples) v->sample_ptrs.push_back(s.c_str());
        *out = v.release();
        return (int)VB2_OK;
    });
}

int vb2_vcf_get_view(const vb2_vcf* v, vb2_vcf_view* o)
{
    if (!v || !o) {
        set_error("vb2_vcf_get_view: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::memset(o, 0, sizeof(*o));
    o->num_marker = v->mk.num_marker;
    o->num_sample = v->mk.num_sample;
    o->num_chr = (int32_t)v->mk.chr_names.size();
    o->genotypes = v->geno.data();
    o->pos = v->mk.pos.data();
    o->chr_index = v->mk.chr_index.data();
    o->ref = v->mk.ref.data();
    o->alt = v->mk.alt.data();
    o->chr_names = v->chr_ptrs.data();
    o->sample_ids = v->sample_ptrs.data();
    return VB2_OK;
}

void vb2_vcf_free(vb2_vcf* v) { delete v; }

int vb2_panel_build(const vb2_panel_args* a, vb2_panel** out)
{
    if (!a || !a->vcf_path || !out) {
        set_error("vb2_panel_build: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    const auto t0 = vb2::Clock::now();
    return vb2::entry([&] {
        std::unique_ptr<vb2_panel> p(new vb2_panel);
        p->has_markers = true;
        const bool notices = a->notices != 0;
        const bool skip = a->skip_min_sample_count_check != 0;
        const auto inc = vb2::parse_include_chr(a->include_chr);
        if (notices) std::fprintf(stderr, "NOTICE - --IncludeChr: filtering to %d chromosome name(s)\n", (int)inc.size());
        std::unique_ptr<vb2::Builder> b;
        std::vector<int8_t> held;     // markers kept before the minimums are settled
        int32_t N = 0;
        const int64_t cw = vb2::chunk_width(a);
        const auto tp = vb2::Clock::now();
        const int rc = vb2::read_vcf(
            a->vcf_path, inc, a->num_thread, notices, &p->mk, [&](int32_t n) { N = n; },
            [&](const int8_t* blk, int64_t first, int64_t n) {
                if (!b) {
                    held.insert(held.end(), blk, blk + (size_t)n * N);
                    // the device starts once the minimums can no longer fail
                    if (first + n < vb2::kMinMarkers || (N < vb2::kMinSamples && !skip)) return (int)VB2_OK;
                    b.reset(new vb2::Builder(N, cw, a->device));
                    const int r = b->start();
                    if (r != VB2_OK) return r;
                    b->push(held.data(), first + n);
                    std::vector<int8_t>().swap(held);
                    return (int)VB2_OK;
                }
                b->push(blk, n);
                return (int)VB2_OK;
            });
        if (rc != VB2_OK) return rc;
        p->seconds[vb2::kParse] = vb2::since(tp);
        const int64_t M = p->mk.num_marker;
        if (notices) {
            std::fprintf(stderr, "NOTICE - Number of Markers after filtering: %lld\n", (long long)M);
            std::fprintf(stderr, "NOTICE - Number of Individuals: %d\n", (int)N);
        }
        int r = vb2::check_minimums(M, N, skip, notices);
        if (r != VB2_OK) return r;
        if (!b) {   // cannot happen once the minimums hold; kept for clarity
            b.reset(new vb2::Builder(N, cw, a->device));
            if ((r = b->start()) != VB2_OK) return r;
            b->push(held.data(), M);
        }
        if (notices)
            std::fprintf(stderr, "NOTICE - Building genotype matrix (%lld markers x %d individuals) on the GPU...\n",
                         (long long)M, (int)N);
        b->finish(p.get(), a->num_svd_pcs);
        b.reset();
        if (notices) vb2::log_variance_explained(p->sigma);
        p->seconds_total = vb2::since(t0);
        *out = p.release();
        return (int)VB2_OK;
    });
}

int vb2_panel_build_genotypes(const vb2_panel_args* a, const int8_t* geno, int64_t M, int32_t N, vb2_panel** out)
{
    if (!a || !geno || !out || M < 1 || N < 1) {
        set_error("vb2_panel_build_genotypes: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    const auto t0 = vb2::Clock::now();
    return vb2::entry([&] {
        std::unique_ptr<vb2_panel> p(new vb2_panel);
        for (int64_t i = 0; i < M * (int64_t)N; ++i)
            if (geno[i] < -1 || geno[i] > 2) {
                set_error("vb2_panel_build_genotypes: genotypes must be -1, 0, 1 or 2");
                return (int)VB2_ERR_INVALID;
            }
        if (a->check_minimums) {
            const int r = vb2::check_minimums(M, N, a->skip_min_sample_count_check != 0, a->notices != 0);
            if (r != VB2_OK) return r;
        }
        vb2::Builder b(N, vb2::chunk_width(a), a->device);
        int r = b.start();
        if (r != VB2_OK) return r;
        b.push(geno, M);
        b.finish(p.get(), a->num_svd_pcs);
        if (a->notices) vb2::log_variance_explained(p->sigma);
        p->seconds_total = vb2::since(t0);
        *out = p.release();
        return (int)VB2_OK;
    });
}

int vb2_panel_get_view(const vb2_panel* p, vb2_panel_view* o)
{
    if (!p || !o) {
        set_error("vb2_panel_get_view: invalid argument");
        return VB2_ERR_INVALID;
    }
    std::memset(o, 0, sizeof(*o));
    o->num_marker = p->M;
    o->num_sample = p->N;
    o->num_pc = p->k;
    o->ud = p->ud.data();
    o->v = p->v.data();
    o->mu = p->mu.data();
    o->sigma = p->sigma.data();
    o->gram = p->gram.data();
    o->row_sum = p->row_sum.data();
    for (int i = 0; i < 7; ++i) o->seconds[i] = p->seconds[i];
    o->seconds_total = p->seconds_total;
    return VB2_OK;
}

int vb2_panel_write(vb2_panel* p, const char* prefix)
{
    if (!p || !prefix) {
        set_error("vb2_panel_write: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (!p->has_markers) {
        set_error("vb2_panel_write: a panel built from a genotype matrix has no marker names (.bed/.mu need them)");
        return VB2_ERR_INVALID;
    }
    return vb2::entry([&] {
        const auto t0 = vb2::Clock::now();
        const std::string pre(prefix);
        const int64_t M = p->M;
        const int32_t N = p->N, k = p->k;
        // chooseBed[chr][end] (:212) holds the LAST kept marker of a chr:pos, and the .bed line of every marker at
        // that chr:pos prints it
        std::unordered_map<uint64_t, int64_t> last;
        last.reserve((size_t)M);
        for (int64_t i = 0; i < M; ++i)
            last[((uint64_t)(uint32_t)p->mk.chr_index[i] << 32) | (uint32_t)p->mk.pos[i]] = i;
        std::ofstream fMu(pre + ".mu"), fUD(pre + ".UD"), fPC(pre + ".V"), fBed(pre + ".bed");
        if (!fMu || !fUD || !fPC || !fBed) {
            set_error("cannot write the panel files " + pre + ".UD/.mu/.bed/.V");
            return (int)VB2_ERR_IO;
        }
        for (int64_t i = 0; i < M; ++i) {
            const std::string& chr = p->mk.chr_names[p->mk.chr_index[i]];
            const int end = p->mk.pos[i], beg = end - 1;
            const int64_t li = last[((uint64_t)(uint32_t)p->mk.chr_index[i] << 32) | (uint32_t)end];
            fMu << chr + ":" + std::to_string(end) << "\t" << p->mu[i] << "\n";
            fBed << chr << "\t" << beg << "\t" << end << "\t" << p->mk.ref[li] << "\t" << p->mk.alt[li] << "\n";
            const double* row = p->ud.data() + (size_t)i * k;
            for (int32_t j = 0; j < k; ++j) fUD << row[j] << "\t";
            fUD << "\n";
        }
        for (int32_t s = 0; s < N; ++s) {
            fPC << p->mk.samples[s] << "\t";
            for (int32_t j = 0; j < k; ++j) fPC << p->v[(size_t)s * k + j] << "\t";
            fPC << "\n";
        }
        fMu.close();
        fUD.close();
        fPC.close();
        fBed.close();
        if (!fMu || !fUD || !fPC || !fBed) {
            set_error("writing the panel files " + pre + ".UD/.mu/.bed/.V failed");
            return (int)VB2_ERR_IO;
        }
        p->seconds[vb2::kWrite] = vb2::since(t0);
        return (int)VB2_OK;
    });
}

void vb2_panel_destroy(vb2_panel* p) { delete p; }

}  // extern "C"
