// replicates.cpp -- host side of the weighted-marker replicates (marker_sum_kernels.hip): what fills
// the weight rows of a replicate set (the rest of the set: row_set.cpp), the options of its lock-step searches (refit.h), the
// host-only helpers (chromosome and bootstrap weights, the delete-m_j jackknife) and the file flow behind --PerChromosome /
// --Bootstrap.
#include "replicates.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "context.h"
#include "guard.h"
#include "host_clock.h"
#include "hostio.h"
#include "marker_sum_kernels.h"
#include "run.h"

namespace vb2 {

namespace {
const RowSet::Kind kKind = {
    "vb2_replicates_eval", "a replicate's", "replicates", nullptr, true,
    [](const DeviceLayout& L) { return (size_t)L.m_pad; },
    [](const DeviceLayout& L, int num_point, const double* d_rows, const int32_t* d_row_of, const void* d_weights, double* d_partial,
       double* d_out, hipStream_t s) {
        return launch_llk_weighted(L, num_point, d_rows, d_row_of, static_cast<const uint8_t*>(d_weights), d_partial, d_out, s);
    }};
}  // namespace

Replicates::Replicates() : RowSet(kKind) {}

int Replicates::create(Context* ctx, int num_rep, const uint8_t* weight, Replicates** out)
{
    *out = nullptr;
    if (!weight) {
        set_error("vb2_replicates_create: invalid argument (1..65535 replicates)");
        return VB2_ERR_INVALID;
    }
    std::unique_ptr<Replicates> r(new Replicates());
    if (const int rc = r->init(ctx, num_rep, "vb2_replicates_create")) return rc;
    const size_t M = (size_t)ctx->num_marker, na = (size_t)ctx->L.num_active;
    // counted markers per replicate, on the host: the sorted positions' panel rows are h_active[h_perm[position]]
    r->counted.assign(num_rep, 0);
    if (na > 0 && ctx->h_perm.size() < na) {
        set_error("vb2_replicates_create: the context holds no marker order");
        return VB2_ERR_INVALID;
    }
    for (size_t pos = 0; pos < na; ++pos) {
        const int64_t a = ctx->h_perm[pos];
        if (a < 0 || (size_t)a >= ctx->h_active.size()) continue;
        const size_t i = (size_t)ctx->h_active[(size_t)a];
        if (i >= M) continue;
        for (int q = 0; q < num_rep; ++q) r->counted[q] += weight[(size_t)q * M + i] != 0;
    }
    if (const int rc = r->upload(weight, M * (size_t)num_rep, "vb2_replicates_create: weight upload failed: ", [&](const void* d_panel) {
            return launch_weights_permute(ctx->L, ctx->num_marker, num_rep, static_cast<const uint8_t*>(d_panel), ctx->d_pidx,
                                          static_cast<uint8_t*>(r->d_payload_), ctx->stream);
        }))
        return rc;
    *out = r.release();
    return VB2_OK;
}

int replicates_lockstep(vb2_replicates_eval_fn fn, void* user, int num_rep, int num_pc, bool data_has_known_af,
                        const vb2_model& model, vb2_estimate* est, int32_t* status, int64_t* num_step)
{
    const std::vector<uint8_t> known_af((size_t)std::max(num_rep, 0), data_has_known_af ? 1 : 0);
    Refit o;                                   // the model's own search from the reference start: no side is held
    o.who = "vb2_replicates_optimize_llk";
    o.empty_message = "vb2_replicates_optimize_llk: a replicate's weights select no counted marker";
    o.known_af = known_af.data();
    o.num_step = num_step;
    return refit_lockstep(o, fn, user, num_rep, num_pc, model, est, status);
}

namespace {
int replicates_eval_cb(void* user, int32_t, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                       double* llk)
{
    return static_cast<Replicates*>(user)->eval(num_point, pc1, pc2, alpha, llk);
}
}  // namespace

int Replicates::optimize(const vb2_model& model, vb2_estimate* est, int32_t* status)
{
    if (!est || !status) {
        set_error("vb2_replicates_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (ctx->resident_active) {
        set_error("vb2_replicates_optimize_llk: not inside vb2_ctx_search_begin / vb2_ctx_search_end");
        return VB2_ERR_INVALID;
    }
    return replicates_lockstep(replicates_eval_cb, this, num_row, ctx->num_pc, ctx->L.known_af != nullptr, model, est, status,
                               nullptr);
}

// ---------------------------------------------------------------------------
// host-only helpers
// ---------------------------------------------------------------------------
namespace {
struct Blocks {
    std::vector<std::string> names;
    std::vector<int32_t> block_of;           // per row
    std::vector<int32_t> size;               // distinct positions per block
};

// the chromosomes of a panel's rows in order of first appearance (rows beyond `rows` are not looked at)
void blocks_of_panel(const Panel& p, size_t rows, Blocks* b)
{
    rows = std::min(rows, p.rowSlot.size());
    std::vector<int32_t> block_of_chr(p.chrNames.size(), -1);
    std::vector<char> seen(p.num_slot(), 0);
    b->block_of.assign(rows, -1);
    for (size_t i = 0; i < rows; ++i) {
        const int32_t slot = p.rowSlot[i], chr = p.slotChr[slot];
        if (block_of_chr[chr] < 0) {
            block_of_chr[chr] = (int32_t)b->names.size();
            b->names.push_back(p.chrNames[chr]);
            b->size.push_back(0);
        }
        b->block_of[i] = block_of_chr[chr];
        if (!seen[slot]) {
            seen[slot] = 1;
            ++b->size[block_of_chr[chr]];
        }
    }
}

inline uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

double freemix_of(const vb2_estimate& e) { return e.alpha < 0.5 ? e.alpha : 1 - e.alpha; }
}  // namespace

}  // namespace vb2

using vb2::guarded;
using vb2::set_error;

extern "C" {

int vb2_replicates_create(vb2_ctx* ctx, int32_t num_rep, const uint8_t* weight, vb2_replicates** out)
{
    if (!out) {
        set_error("vb2_replicates_create: out is NULL");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (!ctx || !ctx->impl) {
        set_error("null vb2_ctx");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Replicates* r = nullptr;
        if (const int rc = vb2::Replicates::create(ctx->impl, num_rep, weight, &r)) return rc;
        *out = new vb2_replicates{r};
        return VB2_OK;
    });
}

void vb2_replicates_destroy(vb2_replicates* rep)
{
    if (!rep) return;
    delete rep->impl;
    delete rep;
}

int vb2_replicates_eval(vb2_replicates* rep, const int32_t* num_point, const double* pc1, const double* pc2, const double* alpha,
                        double* llk_out)
{
    if (!rep || !rep->impl) {
        set_error("null vb2_replicates");
        return VB2_ERR_INVALID;
    }
    return rep->impl->eval(num_point, pc1, pc2, alpha, llk_out);
}

int vb2_replicates_optimize_llk(vb2_replicates* rep, const vb2_model* model, vb2_estimate* est_out, int32_t* status)
{
    if (!rep || !rep->impl || !model) {
        set_error("vb2_replicates_optimize_llk: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&] { return rep->impl->optimize(*model, est_out, status); });
}

int vb2_debug_replicates_time(vb2_replicates* rep, int32_t num_point, int32_t warmup, int32_t reps, double* ms)
{
    if (!rep || !rep->impl) return VB2_ERR_INVALID;
    return rep->impl->time_launch(num_point, warmup, reps, ms);
}

int vb2_replicates_info_get(const vb2_replicates* rep, vb2_replicates_info* info, int64_t* counted)
{
    if (!rep || !rep->impl || !info) return VB2_ERR_INVALID;
    const vb2::Replicates& r = *rep->impl;
    info->num_rep = r.num_row;
    info->num_marker = r.ctx->num_marker;
    info->device_bytes = r.device_bytes;
    info->num_step = r.num_step();
    info->num_launch = r.num_launch();
    if (counted) std::memcpy(counted, r.counted.data(), sizeof(int64_t) * (size_t)r.num_row);
    return VB2_OK;
}

int vb2_replicates_lockstep(vb2_replicates_eval_fn fn, void* user, int32_t num_rep, int32_t num_pc, const vb2_model* model,
                            vb2_estimate* est_out, int32_t* status)
{
    if (!fn || !model || !est_out || !status || num_rep < 1 || num_pc < 1 || num_pc > VB2_MAX_PC) {
        set_error("vb2_replicates_lockstep: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&] { return vb2::replicates_lockstep(fn, user, num_rep, num_pc, false, *model, est_out, status, nullptr); });
}

int vb2_chromosome_weights(const char* bed_path, int32_t num_marker, int32_t max_block, int32_t* num_block, int32_t* block_of,
                           int32_t* block_size, char* names, uint8_t* only, uint8_t* without)
{
    if (!bed_path || num_marker < 1 || !num_block) {
        set_error("vb2_chromosome_weights: invalid argument");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        vb2::Panel panel;
        if (const int rc = vb2::read_bed(bed_path, &panel)) return rc;
        vb2::Blocks b;
        vb2::blocks_of_panel(panel, (size_t)num_marker, &b);
        const int32_t nb = (int32_t)b.names.size();
        *num_block = nb;
        if (b.block_of.size() < (size_t)num_marker) {
            set_error("vb2_chromosome_weights: the .bed has fewer rows than num_marker");
            return VB2_ERR_INVALID;
        }
        if ((block_size || names || only || without) && nb > max_block) {
            set_error("vb2_chromosome_weights: more chromosomes than max_block");
            return VB2_ERR_INVALID;
        }
        const size_t M = (size_t)num_marker;
        if (block_of) std::memcpy(block_of, b.block_of.data(), sizeof(int32_t) * M);
        for (int32_t j = 0; j < nb; ++j) {
            if (block_size) block_size[j] = b.size[j];
            if (names) {
                char* dst = names + (size_t)j * VB2_CHROM_NAME_LEN;
                std::memset(dst, 0, VB2_CHROM_NAME_LEN);
                std::strncpy(dst, b.names[j].c_str(), VB2_CHROM_NAME_LEN - 1);
            }
            for (size_t i = 0; i < M && (only || without); ++i) {
                const uint8_t in = b.block_of[i] == j ? 1 : 0;
                if (only) only[(size_t)j * M + i] = in;
                if (without) without[(size_t)j * M + i] = (uint8_t)(1 - in);
            }
        }
        return VB2_OK;
    });
}

int vb2_bootstrap_weights(int32_t num_marker, int32_t num_rep, uint32_t seed, uint8_t* out)
{
    if (num_marker < 1 || num_rep < 1 || !out) {
        set_error("vb2_bootstrap_weights: invalid argument");
        return VB2_ERR_INVALID;
    }
    const size_t M = (size_t)num_marker;
    std::memset(out, 0, M * (size_t)num_rep);
    for (int32_t r = 0; r < num_rep; ++r) {
        uint64_t s = ((uint64_t)seed << 32) ^ (0x5851f42d4c957f2dull * (uint64_t)(r + 1));
        uint8_t* row = out + (size_t)r * M;
        for (size_t d = 0; d < M; ++d) {
            const uint64_t x = vb2::splitmix64(s);
            const size_t i = (size_t)(((unsigned __int128)x * (unsigned __int128)M) >> 64);
            if (row[i] != 255) ++row[i];
        }
    }
    return VB2_OK;
}

int vb2_jackknife(int32_t num_block, const int64_t* m, double theta_hat, const double* theta_without, double* estimate, double* se)
{
    if (num_block < 1 || !m || !theta_without || !estimate || !se) {
        set_error("vb2_jackknife: invalid argument");
        return VB2_ERR_INVALID;
    }
    double n = 0;
    int g = 0;
    for (int32_t j = 0; j < num_block; ++j)
        if (m[j] > 0) {
            n += (double)m[j];
            ++g;
        }
    if (g < 2) {
        set_error("vb2_jackknife: fewer than two blocks with counted markers");
        return VB2_ERR_INVALID;
    }
    // the formulas of vb2_abi.h in the differences d_j = theta_hat - theta_without[j] (sum_j (1 - m_j / n) = g - 1):
    //   estimate = theta_hat + S,  S = sum_j (1 - m_j / n) d_j;   tau_j - estimate = (h_j - 1) d_j - S
    // -- the same numbers without the cancellation of g theta_hat against the sum: equal estimates give se = 0 exactly
    double S = 0;
    for (int32_t j = 0; j < num_block; ++j)
        if (m[j] > 0) S += (1.0 - (double)m[j] / n) * (theta_hat - theta_without[j]);
    const double est = theta_hat + S;
    double var = 0;
    for (int32_t j = 0; j < num_block; ++j) {
        if (m[j] <= 0) continue;
        const double h = n / (double)m[j];
        const double dev = (h - 1.0) * (theta_hat - theta_without[j]) - S;
        var += dev * dev / (h - 1.0);
    }
    *estimate = est;
    *se = std::sqrt(var / (double)g);
    return VB2_OK;
}

int vb2_run_replicates(const vb2_run_args* args, int32_t per_chromosome, int32_t bootstrap, vb2_run_result* out,
                       vb2_replicate_summary* summary)
{
    if (!args || !out || bootstrap < 0 || bootstrap > 1000 || (!per_chromosome && bootstrap == 0)) {
        set_error("vb2_run_replicates: invalid argument (--Bootstrap takes 1..1000 replicates)");
        return VB2_ERR_INVALID;
    }
    if (args->devices && args->num_device > 1) {
        set_error("--PerChromosome / --Bootstrap take one device: they cannot be combined with marker shards over several "
                  "--Devices");
        return VB2_ERR_INVALID;
    }
    vb2_replicate_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    sum.jack_estimate = sum.jack_se = sum.jack_lo = sum.jack_hi = NAN;
    sum.boot_mean = sum.boot_sd = sum.boot_p025 = sum.boot_p975 = NAN;
    vb2::RunStage stage;
    stage.on_context = [&](vb2_ctx* ctx, const vb2_flat& flat, const vb2_model& model, const vb2_estimate& whole) -> int {
        const double t0 = vb2::now_s();
        vb2::Context* c = ctx->impl;
        const size_t M = (size_t)c->num_marker;
        vb2::Blocks b;
        if (per_chromosome) vb2::blocks_of_panel(flat.panel, M, &b);
        const int C = (int)b.names.size(), N = bootstrap, R = 2 * C + N;
        if (R < 1) {
            set_error("vb2_run_replicates: the panel names no chromosome");
            return VB2_ERR_INVALID;
        }
        // rows: C "only", C "without", N bootstrap resamples
        std::vector<uint8_t> w((size_t)R * M, 0);
        for (size_t i = 0; i < M && C > 0; ++i) {
            const int32_t j = i < b.block_of.size() ? b.block_of[i] : -1;
            for (int q = 0; q < C; ++q) {
                w[(size_t)q * M + i] = q == j ? 1 : 0;
                w[(size_t)(C + q) * M + i] = q == j ? 0 : 1;
            }
        }
        if (N > 0)
            if (const int rc = vb2_bootstrap_weights((int32_t)M, N, args->search.seed, w.data() + (size_t)2 * C * M)) return rc;
        const bool notices = model.notices != 0;
        if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Likelihood replicates (%d searches in lock-step)\n", R);
        vb2::Replicates* rep = nullptr;
        if (const int rc = vb2::Replicates::create(c, R, w.data(), &rep)) return rc;
        std::unique_ptr<vb2::Replicates> holder(rep);
        std::vector<vb2_estimate> est(R);
        std::vector<int32_t> status(R, 0);
        if (const int rc = rep->optimize(model, est.data(), status.data())) return rc;
        sum.num_step = rep->num_step();
        const double theta = vb2::freemix_of(whole);
        if (C > 0) {
            std::vector<int64_t> m(C);
            std::vector<double> without(C, 0.0);
            for (int j = 0; j < C; ++j) {
                m[j] = status[j] == VB2_OK ? rep->counted[j] : 0;
                if (status[C + j] != VB2_OK) m[j] = 0;
                without[j] = vb2::freemix_of(est[C + j]);
            }
            double je = NAN, jse = NAN;
            if (vb2_jackknife(C, m.data(), theta, without.data(), &je, &jse) == VB2_OK) {
                sum.jack_estimate = je;
                sum.jack_se = jse;
                sum.jack_lo = std::min(0.5, std::max(0.0, theta - 1.96 * jse));
                sum.jack_hi = std::min(0.5, std::max(0.0, theta + 1.96 * jse));
            }
            sum.num_chrom = C;
            if (args->output_prefix) {
                const int rc = vb2::write_text_file(std::string(args->output_prefix) + ".Chrom", [&](std::ostream& fout) {
                    fout << "#CHROM\tMARKERS\tFREEMIX_ONLY\tFREELK1_ONLY\tFREELK0_ONLY\tFREEMIX_WITHOUT\tDELTA\n";
                    for (int j = 0; j < C; ++j) {
                        fout << b.names[j] << "\t" << rep->counted[j];
                        if (m[j] > 0) {
                            fout << "\t" << vb2::freemix_of(est[j]) << "\t" << -est[j].llk1 << "\t" << -est[j].llk0 << "\t" << without[j]
                                 << "\t" << without[j] - theta << "\n";
                        } else {
                            fout << "\tNA\tNA\tNA\tNA\tNA\n";
                        }
                    }
                    fout << "#JACKKNIFE\tFREEMIX\t" << sum.jack_estimate << "\tSE\t" << sum.jack_se << "\tLO\t" << sum.jack_lo << "\tHI\t"
                         << sum.jack_hi << "\n";
                });
                if (rc) return rc;
            }
        }
        if (N > 0) {
            std::vector<double> v;
            for (int q = 0; q < N; ++q)
                if (status[2 * C + q] == VB2_OK) v.push_back(vb2::freemix_of(est[2 * C + q]));
            sum.num_boot = (int32_t)v.size();
            if (!v.empty()) {
                double mean = 0, ss = 0;
                for (double x : v) mean += x;
                mean /= (double)v.size();
                for (double x : v) ss += (x - mean) * (x - mean);
                std::vector<double> sorted(v);
                std::sort(sorted.begin(), sorted.end());
                const double last = (double)(sorted.size() - 1);
                sum.boot_mean = mean;
                sum.boot_sd = v.size() > 1 ? std::sqrt(ss / (double)(v.size() - 1)) : 0.0;
                sum.boot_p025 = sorted[(size_t)std::floor(0.025 * last + 0.5)];
                sum.boot_p975 = sorted[(size_t)std::floor(0.975 * last + 0.5)];
            }
            if (args->output_prefix) {
                const int rc = vb2::write_text_file(std::string(args->output_prefix) + ".Boot", [&](std::ostream& fout) {
                    fout << "#REPLICATE\tFREEMIX\tFREELK1\n";
                    for (int q = 0; q < N; ++q) {
                        const vb2_estimate& e = est[2 * C + q];
                        if (status[2 * C + q] == VB2_OK) fout << q + 1 << "\t" << vb2::freemix_of(e) << "\t" << -e.llk1 << "\n";
                        else fout << q + 1 << "\tNA\tNA\n";
                    }
                    fout << "#BOOTSTRAP\tMEAN\t" << sum.boot_mean << "\tSD\t" << sum.boot_sd << "\tP2.5\t" << sum.boot_p025 << "\tP97.5\t"
                         << sum.boot_p975 << "\n";
                });
                if (rc) return rc;
            }
        }
        sum.seconds = vb2::now_s() - t0;
        if (notices)
            std::fprintf(stderr, "NOTICE - Finished phase: Likelihood replicates  [%.3f seconds, %lld lock-step steps]\n", sum.seconds,
                         (long long)sum.num_step);
        if (C > 0)
            std::fprintf(stderr, "NOTICE - FREEMIX jackknife over %d chromosomes: %g, SE %g, [%g, %g]\n", C, sum.jack_estimate,
                         sum.jack_se, sum.jack_lo, sum.jack_hi);
        if (N > 0)
            std::fprintf(stderr, "NOTICE - FREEMIX bootstrap over %d resamples: mean %g, SD %g, [%g, %g]\n", (int)sum.num_boot,
                         sum.boot_mean, sum.boot_sd, sum.boot_p025, sum.boot_p975);
        return VB2_OK;
    };
    return guarded([&] {
        const int rc = vb2::run_sample(args, out, stage);
        if (summary) *summary = sum;
        return rc;
    });
}

}  // extern "C"
