// errstat.cpp -- host side of the E-step of the error-rate fit (errstat.h): the raw sample goes up once into one slab; an
// evaluation uploads the table and the point, launches errstat_kernels.hip's two kernels and turns the fixed-point sums into
// doubles, each rounded once.  ErrStatBatch does the same for up to 64 samples through errstat_multi_kernels.hip.
#include "errstat.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "context.h"
#include "device_util.h"
#include "guard.h"
#include "tunables.h"

namespace vb2 {

bool err_table_ok(const double* err_table, const char* who)
{
    if (!err_table) {
        set_error(std::string(who) + ": the error table is NULL");
        return false;
    }
    for (int q = 0; q < kErrNumQual; ++q)
        if (!(err_table[q] >= 0.0 && err_table[q] <= 1.0)) {        // (false for a NaN)
            set_error(std::string(who) + ": the error rate of quality " + std::to_string(q) + " lies outside [0, 1]");
            return false;
        }
    return true;
}

namespace {

// the device of opt (or the current one) and its CU count; gfx950 only
int pick_device(const vb2_options* opt, const char* who, int* dev_out, int* num_cu)
{
    const std::string w(who);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        set_error(w + ": no HIP device visible (this library has no CPU fallback)");
        return VB2_ERR_NO_DEVICE;
    }
    int dev = opt ? opt->device : -1;
    if (dev < 0) VB2_HIP(hipGetDevice(&dev));
    if (dev >= ndev) {
        set_error(w + ": device ordinal out of range");
        return VB2_ERR_INVALID;
    }
    hipDeviceProp_t prop;
    VB2_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(w + ": device is " + prop.gcnArchName + ", kernels are built for gfx950 only");
        return VB2_ERR_NO_DEVICE;
    }
    *dev_out = dev;
    *num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    return VB2_OK;
}

// the shape of a raw input, as both sets need it
int check_input(const vb2_input* in, const char* who)
{
    const std::string w(who);
    if (!in || in->num_marker < 0 || in->num_pc < 1 || in->num_pc > VB2_MAX_PC || !in->read_off ||
        (!in->known_af && (!in->ud || !in->means))) {
        set_error(w + ": invalid input");
        return VB2_ERR_INVALID;
    }
    const int M = in->num_marker;
    for (int i = 0; i < M; ++i)
        if (in->read_off[i + 1] < in->read_off[i]) {
            set_error(w + ": read_off not monotone");
            return VB2_ERR_INVALID;
        }
    if (M > 0 && in->read_off[M] > in->read_off[0] && (!in->bases || !in->quals || !in->alt_base)) {
        set_error(w + ": reads without bases / quals / alt_base arrays");
        return VB2_ERR_INVALID;
    }
    return VB2_OK;
}

// a result's words as the caller's numbers: the reads, the expected errors rounded once, the log-likelihood's bits
void words_out(const unsigned long long* w, int64_t* n, double* s, double* llk)
{
    for (int q = 0; q < kErrNumQual; ++q) {
        if (n) n[q] = (int64_t)w[q];
        if (s) {
            // sum floor(r 2^32) 2^32 + sum (the next 32 bits): a 128-bit integer in units of 2^-64, through the 64-bit
            // mantissa of a long double to the nearest double (the same bits for the same integer)
            const unsigned __int128 t = ((unsigned __int128)w[kErrNumQual + q] << 32) + (unsigned __int128)w[2 * kErrNumQual + q];
            const uint64_t hi = (uint64_t)(t >> 64), lo = (uint64_t)t;
            s[q] = (double)((long double)hi + std::ldexp((long double)lo, -64));
        }
    }
    if (llk) std::memcpy(llk, &w[kErrBinWords], sizeof(double));
}

// one slab's pieces, every one 256-byte aligned
struct Carver {
    size_t total = 0;
    size_t operator()(size_t bytes)
    {
        const size_t off = total;
        total = up256(total + bytes);
        return off;
    }
};

}  // namespace

ErrStat::~ErrStat()
{
    if (device >= 0) (void)hipSetDevice(device);
    if (stream_) (void)hipStreamSynchronize(stream_);
    give_device(d_mem_, d_mem_bytes_, device);
    if (own_stream_ && stream_ && !recycle_stream(stream_, device)) (void)hipStreamDestroy(stream_);
}

int ErrStat::create(const vb2_input* in, const vb2_options* opt, ErrStat** out)
{
    *out = nullptr;
    if (const int rc = check_input(in, "vb2_errstat_create")) return rc;
    const int M = in->num_marker, k = in->num_pc;
    const int64_t base = M > 0 ? in->read_off[0] : 0, R = M > 0 ? in->read_off[M] - base : 0;
    int dev = -1, num_cu = 1;
    if (const int rc = pick_device(opt, "vb2_errstat_create", &dev, &num_cu)) return rc;
    VB2_HIP(hipSetDevice(dev));
    std::unique_ptr<ErrStat> e(new ErrStat());
    e->device = dev;
    e->num_cu = num_cu;
    e->num_marker = M;
    e->num_pc = k;
    e->num_read = R;
    if (opt && opt->stream) {
        e->stream_ = (hipStream_t)opt->stream;
    } else {
        e->stream_ = cached_stream(dev);
        if (!e->stream_) VB2_HIP(hipStreamCreateWithFlags(&e->stream_, hipStreamNonBlocking));
        e->own_stream_ = true;
    }
    // the launch shape: about four workgroups per CU (walk::stripe_grid), at most one per group of 256 markers
    const int ngrp = errstat_groups(M);
    e->max_grid_ = ngrp > 0 ? ngrp : 1;

    // one slab, every piece 256-byte aligned
    Carver carve;
    const bool kaf = in->known_af != nullptr;
    const size_t o_bases = carve((size_t)R), o_quals = carve((size_t)R), o_off = carve(sizeof(int64_t) * ((size_t)M + 1));
    const size_t o_alt = carve((size_t)M);
    const size_t o_ud = carve(kaf ? 0 : sizeof(double) * (size_t)M * (size_t)k), o_mu = carve(kaf ? 0 : sizeof(double) * (size_t)M);
    const size_t o_kaf = carve(kaf ? sizeof(double) * (size_t)M : 0);
    const size_t o_point = carve(sizeof(ErrStatPoint));
    const size_t o_slab = carve(sizeof(unsigned long long) * kErrBinWords * (size_t)e->max_grid_);
    const size_t o_partial = carve(sizeof(double) * (size_t)e->max_grid_);
    const size_t o_out = carve(sizeof(unsigned long long) * kErrOutWords);
    const size_t total = carve.total;
    if (const int rc = take_device(total, dev, &e->d_mem_, &e->d_mem_bytes_, "vb2_errstat_create")) return rc;
    e->device_bytes = (int64_t)total;
    char* d = static_cast<char*>(e->d_mem_);

    std::unique_ptr<int64_t[]> rel(new int64_t[(size_t)M + 1]);
    for (int i = 0; i <= M; ++i) rel[(size_t)i] = M > 0 ? in->read_off[i] - base : 0;
    hipStream_t s = e->stream_;
    hipError_t rc = hipMemcpyAsync(d + o_off, rel.get(), sizeof(int64_t) * ((size_t)M + 1), hipMemcpyHostToDevice, s);
    const auto up = [&](size_t off, const void* src, size_t bytes) {
        if (rc == hipSuccess && bytes > 0) rc = hipMemcpyAsync(d + off, src, bytes, hipMemcpyHostToDevice, s);
    };
    if (R > 0) {
        up(o_bases, in->bases + base, (size_t)R);
        up(o_quals, in->quals + base, (size_t)R);
    }
    if (M > 0 && in->alt_base) up(o_alt, in->alt_base, (size_t)M);
    else if (M > 0 && rc == hipSuccess) rc = hipMemsetAsync(d + o_alt, 0, (size_t)M, s);
    if (kaf) {
        up(o_kaf, in->known_af, sizeof(double) * (size_t)M);
    } else {
        up(o_ud, in->ud, sizeof(double) * (size_t)M * (size_t)k);
        up(o_mu, in->means, sizeof(double) * (size_t)M);
    }
    const hipError_t rs = hipStreamSynchronize(s);          // (the arrays are the caller's: read before this returns)
    if (rc == hipSuccess) rc = rs;
    if (rc != hipSuccess) {
        set_error(std::string("vb2_errstat_create: upload failed: ") + hipGetErrorString(rc));
        return VB2_ERR_HIP;
    }
    ErrStatInput& di = e->in_;
    di.num_marker = M;
    di.num_pc = k;
    di.bases = reinterpret_cast<const uint8_t*>(d + o_bases);
    di.quals = reinterpret_cast<const uint8_t*>(d + o_quals);
    di.read_off = reinterpret_cast<const int64_t*>(d + o_off);
    di.alt_base = reinterpret_cast<const uint8_t*>(d + o_alt);
    di.ud = kaf ? nullptr : reinterpret_cast<const double*>(d + o_ud);
    di.mu = kaf ? nullptr : reinterpret_cast<const double*>(d + o_mu);
    di.known_af = kaf ? reinterpret_cast<const double*>(d + o_kaf) : nullptr;
    di.avg_depth = in->avg_depth;
    di.sd_depth = in->sd_depth;
    di.sanity_disabled = in->sanity_disabled ? 1 : 0;
    e->d_point_ = reinterpret_cast<ErrStatPoint*>(d + o_point);
    e->d_slab_ = reinterpret_cast<unsigned long long*>(d + o_slab);
    e->d_partial_ = reinterpret_cast<double*>(d + o_partial);
    e->d_out_ = reinterpret_cast<unsigned long long*>(d + o_out);
    *out = e.release();
    return VB2_OK;
}

int ErrStat::eval(const double* err_table, const double* pc1, const double* pc2, double alpha, int64_t* n, double* s, double* llk)
{
    if (!err_table_ok(err_table, "vb2_errstat_eval")) return VB2_ERR_INVALID;
    const bool kaf = in_.known_af != nullptr;
    if (!kaf && (!pc1 || !pc2)) {
        set_error("vb2_errstat_eval: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (!(alpha >= 0.0 && alpha <= 1.0)) {
        set_error("vb2_errstat_eval: alpha lies outside [0, 1]");
        return VB2_ERR_INVALID;
    }
    VB2_HIP(hipSetDevice(device));
    ErrStatPoint pt;
    std::memset(&pt, 0, sizeof(pt));
    std::memcpy(pt.err, err_table, sizeof(pt.err));
    if (!kaf) {
        std::memcpy(pt.pc1, pc1, sizeof(double) * (size_t)num_pc);
        std::memcpy(pt.pc2, pc2, sizeof(double) * (size_t)num_pc);
    }
    pt.alpha = alpha;
    // about four workgroups per CU; the tunable errstat_groups sets the grid (the results do not depend on it)
    int grid = 4 * num_cu;
    if (tunables().errstat_groups > 0) grid = tunables().errstat_groups;
    grid = grid < max_grid_ ? grid : max_grid_;
    VB2_HIP(hipMemcpyAsync(d_point_, &pt, sizeof(pt), hipMemcpyHostToDevice, stream_));
    VB2_HIP(launch_errstat(in_, d_point_, grid, d_slab_, d_partial_, d_out_, stream_));
    num_launch += num_marker > 0 ? 2 : 0;
    unsigned long long w[kErrOutWords];
    VB2_HIP(hipMemcpyAsync(w, d_out_, sizeof(w), hipMemcpyDeviceToHost, stream_));
    VB2_HIP(hipStreamSynchronize(stream_));
    words_out(w, n, s, llk);
    return VB2_OK;
}

// ---- the batch ----
ErrStatBatch::~ErrStatBatch()
{
    if (device >= 0) (void)hipSetDevice(device);
    if (stream_) (void)hipStreamSynchronize(stream_);
    give_device(d_mem_, d_mem_bytes_, device);
    if (own_stream_ && stream_ && !recycle_stream(stream_, device)) (void)hipStreamDestroy(stream_);
    delete[] h_up_;
    delete[] h_out_;
}

int ErrStatBatch::create(const vb2_input* const* in, int num_sample, const vb2_options* opt, ErrStatBatch** out)
{
    const char* who = "vb2_errstat_batch_create";
    *out = nullptr;
    if (!in || num_sample < 1 || num_sample > kErrMultiMaxSample) {
        set_error(std::string(who) + ": 1.." + std::to_string(kErrMultiMaxSample) + " samples");
        return VB2_ERR_INVALID;
    }
    const int S = num_sample;
    for (int s = 0; s < S; ++s)
        if (in[s])
            if (const int rc = check_input(in[s], who)) return rc;
    int dev = -1, num_cu = 1;
    if (const int rc = pick_device(opt, who, &dev, &num_cu)) return rc;
    VB2_HIP(hipSetDevice(dev));
    std::unique_ptr<ErrStatBatch> e(new ErrStatBatch());
    e->device = dev;
    e->num_cu = num_cu;
    e->num_sample = S;
    if (opt && opt->stream) {
        e->stream_ = (hipStream_t)opt->stream;
    } else {
        e->stream_ = cached_stream(dev);
        if (!e->stream_) VB2_HIP(hipStreamCreateWithFlags(&e->stream_, hipStreamNonBlocking));
        e->own_stream_ = true;
    }

    // one slab.  A sample's reads, offsets and alleles are its own; a panel (ud and means, or known_af) is held once for
    // the samples that name the same arrays
    struct Piece {
        size_t bases = 0, quals = 0, off = 0, alt = 0;
        int panel = -1;
        int64_t base = 0, R = 0;
    } piece[kErrMultiMaxSample];
    struct Panel {
        const vb2_input* in;
        size_t ud = 0, mu = 0, kaf = 0;
    };
    std::vector<Panel> panels;
    Carver carve;
    int grp_total = 0, grid_total = 0;
    for (int s = 0; s < S; ++s) {
        if (!in[s]) continue;
        const vb2_input& i = *in[s];
        const int M = i.num_marker;
        Piece& p = piece[s];
        p.base = M > 0 ? i.read_off[0] : 0;
        p.R = M > 0 ? i.read_off[M] - p.base : 0;
        // (the kernel stages whole 16-byte loads: a piece ends on a multiple of 256 bytes)
        p.bases = carve((size_t)p.R);
        p.quals = carve((size_t)p.R);
        p.off = carve(sizeof(int64_t) * ((size_t)M + 1));
        p.alt = carve((size_t)M);
        for (size_t j = 0; j < panels.size() && p.panel < 0; ++j) {
            const vb2_input& o = *panels[j].in;
            if (o.num_marker == M && o.num_pc == i.num_pc && o.known_af == i.known_af &&
                (i.known_af || (o.ud == i.ud && o.means == i.means)))
                p.panel = (int)j;
        }
        if (p.panel < 0) {
            Panel np{&i};
            if (i.known_af) {
                np.kaf = carve(sizeof(double) * (size_t)M);
            } else {
                np.ud = carve(sizeof(double) * (size_t)M * (size_t)i.num_pc);
                np.mu = carve(sizeof(double) * (size_t)M);
            }
            p.panel = (int)panels.size();
            panels.push_back(np);
        }
        Sample& sm = e->sample_[s];
        sm.ngrp = errstat_groups(M);
        sm.grp_first = grp_total;
        grp_total += sm.ngrp;
        grid_total += sm.ngrp < kErrMultiMaxGrid ? sm.ngrp : kErrMultiMaxGrid;
        e->num_pc = i.num_pc > e->num_pc ? i.num_pc : e->num_pc;
        e->num_marker += M;
        e->num_read += p.R;
    }
    e->num_pc = e->num_pc > 0 ? e->num_pc : 1;
    e->num_panel = (int)panels.size();
    e->max_grid_ = grid_total > 0 ? grid_total : 1;
    e->o_jobs_ = up256(sizeof(ErrStatPoint) * (size_t)S);
    e->o_wg_ = e->o_jobs_ + up256(sizeof(ErrMultiJob) * (size_t)S);
    e->up_bytes_ = e->o_wg_ + up256(sizeof(int) * (size_t)e->max_grid_);
    const size_t o_up = carve(e->up_bytes_);
    const size_t o_slab = carve(sizeof(unsigned long long) * kErrBinWords * (size_t)e->max_grid_);
    const size_t o_partial = carve(sizeof(double) * (size_t)(grp_total > 0 ? grp_total : 1));
    const size_t o_out = carve(sizeof(unsigned long long) * kErrOutWords * (size_t)S);
    const size_t total = carve.total;
    if (const int rc = take_device(total, dev, &e->d_mem_, &e->d_mem_bytes_, who)) return rc;
    e->device_bytes = (int64_t)total;
    char* d = static_cast<char*>(e->d_mem_);
    e->h_up_ = new char[e->up_bytes_];
    e->h_out_ = new unsigned long long[(size_t)kErrOutWords * (size_t)S];

    hipStream_t st = e->stream_;
    hipError_t rc = hipSuccess;
    const auto up = [&](size_t off, const void* src, size_t bytes) {
        if (rc == hipSuccess && bytes > 0) rc = hipMemcpyAsync(d + off, src, bytes, hipMemcpyHostToDevice, st);
    };
    std::vector<std::unique_ptr<int64_t[]>> rels;           // (alive until the stream has read them)
    for (int s = 0; s < S; ++s) {
        if (!in[s]) continue;
        const vb2_input& i = *in[s];
        const Piece& p = piece[s];
        const int M = i.num_marker;
        rels.emplace_back(new int64_t[(size_t)M + 1]);
        int64_t* rel = rels.back().get();
        for (int m = 0; m <= M; ++m) rel[m] = M > 0 ? i.read_off[m] - p.base : 0;
        up(p.off, rel, sizeof(int64_t) * ((size_t)M + 1));
        if (p.R > 0) {
            up(p.bases, i.bases + p.base, (size_t)p.R);
            up(p.quals, i.quals + p.base, (size_t)p.R);
        }
        if (M > 0 && i.alt_base) up(p.alt, i.alt_base, (size_t)M);
        else if (M > 0 && rc == hipSuccess) rc = hipMemsetAsync(d + p.alt, 0, (size_t)M, st);
        const Panel& pn = panels[(size_t)p.panel];
        ErrStatInput& di = e->sample_[s].in;
        di.num_marker = M;
        di.num_pc = i.num_pc;
        di.bases = reinterpret_cast<const uint8_t*>(d + p.bases);
        di.quals = reinterpret_cast<const uint8_t*>(d + p.quals);
        di.read_off = reinterpret_cast<const int64_t*>(d + p.off);
        di.alt_base = reinterpret_cast<const uint8_t*>(d + p.alt);
        const bool kaf = i.known_af != nullptr;
        e->sample_[s].known_af = kaf;
        di.ud = kaf ? nullptr : reinterpret_cast<const double*>(d + pn.ud);
        di.mu = kaf ? nullptr : reinterpret_cast<const double*>(d + pn.mu);
        di.known_af = kaf ? reinterpret_cast<const double*>(d + pn.kaf) : nullptr;
        di.avg_depth = i.avg_depth;
        di.sd_depth = i.sd_depth;
        di.sanity_disabled = i.sanity_disabled ? 1 : 0;
    }
    for (const Panel& pn : panels) {
        const vb2_input& i = *pn.in;
        const size_t M = (size_t)i.num_marker;
        if (i.known_af) {
            up(pn.kaf, i.known_af, sizeof(double) * M);
        } else {
            up(pn.ud, i.ud, sizeof(double) * M * (size_t)i.num_pc);
            up(pn.mu, i.means, sizeof(double) * M);
        }
    }
    const hipError_t rs = hipStreamSynchronize(st);         // (the arrays are the caller's: read before this returns)
    if (rc == hipSuccess) rc = rs;
    if (rc != hipSuccess) {
        set_error(std::string(who) + ": upload failed: " + hipGetErrorString(rc));
        return VB2_ERR_HIP;
    }
    e->d_up_ = d + o_up;
    e->d_slab_ = reinterpret_cast<unsigned long long*>(d + o_slab);
    e->d_partial_ = reinterpret_cast<double*>(d + o_partial);
    e->d_out_ = reinterpret_cast<unsigned long long*>(d + o_out);
    *out = e.release();
    return VB2_OK;
}

int ErrStatBatch::eval(const int32_t* live, const double* err_tables, const double* pc1, const double* pc2, const double* alpha,
                       int64_t* n, double* s, double* llk)
{
    const char* who = "vb2_errstat_batch_eval";
    const int S = num_sample;
    if (!err_tables || !alpha) {
        set_error(std::string(who) + ": invalid argument");
        return VB2_ERR_INVALID;
    }
    // the jobs: the live samples that hold markers.  Every live sample's table and alpha are checked, as vb2_errstat_eval
    // checks them
    int job_of[kErrMultiMaxSample], num_job = 0;
    int64_t grp_live = 0;
    for (int i = 0; i < S; ++i) {
        if (live && !live[i]) continue;
        if (!err_table_ok(err_tables + (size_t)i * kErrNumQual, who)) return VB2_ERR_INVALID;
        if (!(alpha[i] >= 0.0 && alpha[i] <= 1.0)) {
            set_error(std::string(who) + ": alpha of sample " + std::to_string(i) + " lies outside [0, 1]");
            return VB2_ERR_INVALID;
        }
        if (sample_[i].ngrp <= 0) continue;
        if (!sample_[i].known_af && (!pc1 || !pc2)) {
            set_error(std::string(who) + ": invalid argument");
            return VB2_ERR_INVALID;
        }
        job_of[num_job++] = i;
        grp_live += sample_[i].ngrp;
    }
    VB2_HIP(hipSetDevice(device));
    // the workgroups are dealt in proportion to the marker groups, eight a CU over the launch, at most kErrMultiMaxGrid and
    // at least one a sample; the tunable errstat_multi_groups sets the number per sample (the results do not depend on it)
    ErrStatPoint* pts = reinterpret_cast<ErrStatPoint*>(h_up_);
    ErrMultiJob* jobs = reinterpret_cast<ErrMultiJob*>(h_up_ + o_jobs_);
    int* wg = reinterpret_cast<int*>(h_up_ + o_wg_);
    const ErrStatPoint* d_pts = reinterpret_cast<const ErrStatPoint*>(d_up_);
    const int64_t budget = 8 * (int64_t)num_cu;
    const int fixed = tunables().errstat_multi_groups;
    int grid = 0;
    std::memset(h_up_, 0, o_wg_);
    for (int j = 0; j < num_job; ++j) {
        const int i = job_of[j];
        const Sample& sm = sample_[i];
        const int cap = sm.ngrp < kErrMultiMaxGrid ? sm.ngrp : kErrMultiMaxGrid;
        int64_t g = fixed > 0 ? fixed : (budget * sm.ngrp + grp_live / 2) / grp_live;
        g = g < 1 ? 1 : g;
        g = g > cap ? cap : g;
        ErrStatPoint& pt = pts[i];
        std::memcpy(pt.err, err_tables + (size_t)i * kErrNumQual, sizeof(pt.err));
        if (!sm.known_af) {
            std::memcpy(pt.pc1, pc1 + (size_t)i * (size_t)num_pc, sizeof(double) * (size_t)sm.in.num_pc);
            std::memcpy(pt.pc2, pc2 + (size_t)i * (size_t)num_pc, sizeof(double) * (size_t)sm.in.num_pc);
        }
        pt.alpha = alpha[i];
        ErrMultiJob& job = jobs[j];
        job.in = sm.in;
        job.point = d_pts + i;
        job.sample = i;
        job.wg_first = grid;
        job.wg_count = (int)g;
        job.grp_first = sm.grp_first;
        for (int b = 0; b < (int)g; ++b) wg[grid + b] = j;
        grid += (int)g;
    }
    if (grid > max_grid_) {                     // (cannot be: every sample's share is capped as max_grid_ was summed)
        set_error(std::string(who) + ": internal: the grid exceeds the slab");
        return VB2_ERR_INVALID;
    }
    if (num_job > 0)
        VB2_HIP(hipMemcpyAsync(d_up_, h_up_, o_wg_ + sizeof(int) * (size_t)grid, hipMemcpyHostToDevice, stream_));
    VB2_HIP(launch_errstat_multi(reinterpret_cast<const ErrMultiJob*>(d_up_ + o_jobs_), num_job,
                                 reinterpret_cast<const int*>(d_up_ + o_wg_), grid, S, d_slab_, d_partial_, d_out_, stream_));
    num_launch += num_job > 0 ? 2 : 0;
    num_eval += 1;
    last_grid = grid;
    VB2_HIP(hipMemcpyAsync(h_out_, d_out_, sizeof(unsigned long long) * kErrOutWords * (size_t)S, hipMemcpyDeviceToHost, stream_));
    VB2_HIP(hipStreamSynchronize(stream_));
    for (int i = 0; i < S; ++i)
        words_out(h_out_ + (size_t)i * kErrOutWords, n ? n + (size_t)i * kErrNumQual : nullptr,
                  s ? s + (size_t)i * kErrNumQual : nullptr, llk ? llk + i : nullptr);
    return VB2_OK;
}

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

extern "C" {

int vb2_errstat_create(const vb2_input* in, const vb2_options* opt, vb2_errstat** out)
{
    if (!out) {
        set_error("vb2_errstat_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return guarded([&]() -> int {
        vb2::ErrStat* e = nullptr;
        if (const int rc = vb2::ErrStat::create(in, opt, &e)) return rc;
        *out = new vb2_errstat{e};
        return VB2_OK;
    });
}

void vb2_errstat_destroy(vb2_errstat* set)
{
    if (!set) return;
    delete set->impl;
    delete set;
}

int vb2_errstat_eval(vb2_errstat* set, const double* err_table, const double* pc1, const double* pc2, double alpha,
                     int64_t* n_out, double* s_out, double* llk_out)
{
    if (!set || !set->impl) {
        set_error("null vb2_errstat");
        return VB2_ERR_INVALID;
    }
    return guarded([&] { return set->impl->eval(err_table, pc1, pc2, alpha, n_out, s_out, llk_out); });
}

int vb2_errstat_info_get(const vb2_errstat* set, vb2_errstat_info* info)
{
    if (!set || !set->impl || !info) return VB2_ERR_INVALID;
    const vb2::ErrStat& e = *set->impl;
    info->num_marker = e.num_marker;
    info->num_pc = e.num_pc;
    info->num_read = e.num_read;
    info->device_bytes = e.device_bytes;
    info->num_launch = e.num_launch;
    return VB2_OK;
}

int vb2_errstat_batch_create(const vb2_input* const* in, int32_t num_sample, const vb2_options* opt, vb2_errstat_batch** out)
{
    if (!out) {
        set_error("vb2_errstat_batch_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    return guarded([&]() -> int {
        vb2::ErrStatBatch* e = nullptr;
        if (const int rc = vb2::ErrStatBatch::create(in, num_sample, opt, &e)) return rc;
        *out = new vb2_errstat_batch{e};
        return VB2_OK;
    });
}

void vb2_errstat_batch_destroy(vb2_errstat_batch* set)
{
    if (!set) return;
    delete set->impl;
    delete set;
}

int vb2_errstat_batch_eval(vb2_errstat_batch* set, const int32_t* live, const double* err_tables, const double* pc1,
                           const double* pc2, const double* alpha, int64_t* n_out, double* s_out, double* llk_out)
{
    if (!set || !set->impl) {
        set_error("null vb2_errstat_batch");
        return VB2_ERR_INVALID;
    }
    return guarded([&] { return set->impl->eval(live, err_tables, pc1, pc2, alpha, n_out, s_out, llk_out); });
}

int vb2_errstat_batch_info_get(const vb2_errstat_batch* set, vb2_errstat_batch_info* info)
{
    if (!set || !set->impl || !info) return VB2_ERR_INVALID;
    const vb2::ErrStatBatch& e = *set->impl;
    info->num_sample = e.num_sample;
    info->num_pc = e.num_pc;
    info->num_panel = e.num_panel;
    info->last_grid = e.last_grid;
    info->num_marker = e.num_marker;
    info->num_read = e.num_read;
    info->device_bytes = e.device_bytes;
    info->num_launch = e.num_launch;
    info->num_eval = e.num_eval;
    return VB2_OK;
}

}  // extern "C"
