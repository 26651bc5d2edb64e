// errstat.cpp -- host side of the E-step of the error-rate fit (errstat.h): the raw sample goes up once into one slab; an
// evaluation uploads the table and the point, launches errstat_kernels.hip's two kernels and turns the fixed-point sums into
// doubles, each rounded once.
#include "errstat.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <string>

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
    if (!in || in->num_marker < 0 || in->num_pc < 1 || in->num_pc > VB2_MAX_PC || !in->read_off ||
        (!in->known_af && (!in->ud || !in->means))) {
        set_error("vb2_errstat_create: invalid input");
        return VB2_ERR_INVALID;
    }
    const int M = in->num_marker, k = in->num_pc;
    for (int i = 0; i < M; ++i)
        if (in->read_off[i + 1] < in->read_off[i]) {
            set_error("vb2_errstat_create: read_off not monotone");
            return VB2_ERR_INVALID;
        }
    const int64_t base = M > 0 ? in->read_off[0] : 0, R = M > 0 ? in->read_off[M] - base : 0;
    if (R > 0 && (!in->bases || !in->quals || !in->alt_base)) {
        set_error("vb2_errstat_create: reads without bases / quals / alt_base arrays");
        return VB2_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        set_error("vb2_errstat_create: no HIP device visible (this library has no CPU fallback)");
        return VB2_ERR_NO_DEVICE;
    }
    int dev = opt ? opt->device : -1;
    if (dev < 0) VB2_HIP(hipGetDevice(&dev));
    if (dev >= ndev) {
        set_error("vb2_errstat_create: device ordinal out of range");
        return VB2_ERR_INVALID;
    }
    hipDeviceProp_t prop;
    VB2_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("vb2_errstat_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
        return VB2_ERR_NO_DEVICE;
    }
    VB2_HIP(hipSetDevice(dev));
    std::unique_ptr<ErrStat> e(new ErrStat());
    e->device = dev;
    e->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
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
    size_t total = 0;
    const auto carve = [&total](size_t bytes) {
        const size_t off = total;
        total = up256(total + bytes);
        return off;
    };
    const bool kaf = in->known_af != nullptr;
    const size_t o_bases = carve((size_t)R), o_quals = carve((size_t)R), o_off = carve(sizeof(int64_t) * ((size_t)M + 1));
    const size_t o_alt = carve((size_t)M);
    const size_t o_ud = carve(kaf ? 0 : sizeof(double) * (size_t)M * (size_t)k), o_mu = carve(kaf ? 0 : sizeof(double) * (size_t)M);
    const size_t o_kaf = carve(kaf ? sizeof(double) * (size_t)M : 0);
    const size_t o_point = carve(sizeof(ErrStatPoint));
    const size_t o_slab = carve(sizeof(unsigned long long) * kErrBinWords * (size_t)e->max_grid_);
    const size_t o_partial = carve(sizeof(double) * (size_t)e->max_grid_);
    const size_t o_out = carve(sizeof(unsigned long long) * kErrOutWords);
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

}  // extern "C"
