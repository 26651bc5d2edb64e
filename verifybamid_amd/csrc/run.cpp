// run.cpp -- see run.h.
#include "run.h"

#include <cstdio>
#include <memory>
#include <string>
#include <thread>

#include "context.h"
#include "device_util.h"
#include "guard.h"
#include "hostio.h"
#include "shard.h"
#include "tunables.h"

namespace vb2 {

namespace {

// Joins a helper thread on every path out of a scope: an exception on the main thread must not
// unwind past a joinable std::thread (that is std::terminate, not an error code).
struct JoinGuard {
    std::thread& t;
    explicit JoinGuard(std::thread& th) : t(th) {}
    ~JoinGuard() { if (t.joinable()) t.join(); }
};

// The run's context and shard group, destroyed on every path out of the run
struct CtxDestroy {
    void operator()(vb2_ctx* c) const { vb2_ctx_destroy(c); }
};
struct ShardGroupDestroy {
    void operator()(vb2_shard_group* g) const { vb2_shard_group_destroy(g); }
};

// The panel files of a run, read on three threads: the constructor starts .UD and .mu on two helpers and reads the .bed,
// then the AF file, on the caller's (the pileup reader needs the .bed, and may run between the constructor and finish()).
class PanelLoad {
public:
    PanelLoad(const vb2_run_args* a, Panel* panel) : panel_(panel)
    {
        try {
            t_ud_ = std::thread([this, a] { parse(read_ud, a->ud_path, &rc_ud_, &err_ud_); });
            t_mu_ = std::thread([this, a] { parse(read_mean, a->mean_path, &rc_mu_, &err_mu_); });
            rc_ = read_bed(a->bed_path, panel_);
            if (!rc_ && a->known_af_path) rc_ = read_known_af(a->known_af_path, panel_);
            if (!rc_) panel_->finish();
            else err_ = g_last_error;
        } catch (...) {
            join();
            throw;
        }
    }
    PanelLoad(const PanelLoad&) = delete;
    PanelLoad& operator=(const PanelLoad&) = delete;
    ~PanelLoad() { join(); }

    bool bed_ok() const { return rc_ == VB2_OK; }

    // waits for .UD and .mu; the first error in the reference's reading order (.bed, AF, .UD, .mu), then the row counts
    int finish()
    {
        join();
        if (rc_) { set_error(err_); return rc_; }
        if (rc_ud_) { set_error(err_ud_); return rc_ud_; }
        if (rc_mu_) { set_error(err_mu_); return rc_mu_; }
        if (panel_->means.size() < panel_->NumMarker || panel_->PosVec.size() < panel_->NumMarker) {
            set_error(".UD has more rows than .mu/.bed");
            return VB2_ERR_INVALID;
        }
        return VB2_OK;
    }

private:
    void parse(int (*read)(const std::string&, Panel*), const char* path, int* rc, std::string* err)
    {
        try { *rc = read(path, panel_); if (*rc) *err = g_last_error; }
        catch (const std::exception& e) { *rc = VB2_ERR_NOMEM; *err = e.what(); }
    }
    void join()
    {
        if (t_ud_.joinable()) t_ud_.join();
        if (t_mu_.joinable()) t_mu_.join();
    }

    Panel* panel_;
    int rc_ = VB2_OK, rc_ud_ = VB2_OK, rc_mu_ = VB2_OK;
    std::string err_, err_ud_, err_mu_;
    std::thread t_ud_, t_mu_;
};

// the sample's pileup, or its BAM (with groups: every read group beside the whole sample)
int read_sample(const vb2_run_args* a, vb2_flat* f, vb2_flat_groups* groups)
{
    BamReadHow how;
    how.bam_adjust = a->bam_adjust;
    how.baq_stats = &f->baq_stats;
    const std::string ref_path = a->reference_path ? a->reference_path : "";
    const int rc = a->pileup_path ? read_pileup(a->pileup_path, f->panel, &f->viewer)
                   : groups       ? read_bam_groups(a->bam_path, f->panel_ptr, &f->viewer, &a->mpileup, a->device, &f->bam_stats, groups,
                                                    ref_path, &how)
                                  : read_bam(a->bam_path, ref_path, f->panel, &f->viewer, &a->mpileup, a->device, &f->bam_stats, &how);
    f->from_bam = !a->pileup_path && !rc;
    f->with_baq = f->from_bam && a->bam_adjust == 1;
    return rc;
}

// A group's own sanity check (unless disabled), BuildResolvedMarkers and status, once the panel is complete.
void finish_group(const vb2_run_args* a, size_t g, vb2_flat_groups* groups)
{
    vb2_flat& f = *groups->flat[g];
    vb2_flat_groups::Info& gi = groups->info[g];
    f.sanity_disabled = a->disable_sanity != 0;
    f.from_bam = false;
    gi.status = VB2_OK;
    if (!f.sanity_disabled) {
        std::fprintf(stderr, "NOTICE - Marker sanity check of read group %s:\n", gi.id.c_str());
        if (!sanity_check(f.panel, &f.viewer)) gi.status = VB2_ERR_SANITY;
    }
    f.resolve();
    if (gi.status == VB2_OK && (f.read_off.empty() || f.read_off.back() == 0)) gi.status = VB2_GROUP_NO_BASE;
}

// which "Estimation from ..." header the reference prints (ContaminationEstimator.cpp:98-150)
const char* estimation_title(const vb2_model& model)
{
    const bool heter = model.is_heter && !model.is_af_known;
    const bool pcfix = (model.is_pc_fixed && model.fix_pc) || model.is_af_known;
    const bool afix = !pcfix && model.is_alpha_fixed;
    if (!heter) return pcfix ? "Estimation from OptimizeHomoFixedPC:" : afix ? nullptr : "Estimation from OptimizeHomo:";
    return pcfix ? "Estimation from OptimizeHeterFixedPC:"
                 : afix ? "Estimation from OptimizeHeterFixedAlpha:" : "Estimation from OptimizeHeter:";
}

// the run's clocks: its start, and the start of "Flatten + upload"
struct RunClock {
    double t0, t_flat0;
};

// One search between the reference's "Optimize likelihood" notices (main.cpp:382); fills seconds_optimize.
template <class F>
int timed_search(bool notices, vb2_run_result* out, F&& search)
{
    const double t1 = now_s();
    if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Optimize likelihood\n");
    const int rc = search();
    out->seconds_optimize = now_s() - t1;
    if (notices) std::fprintf(stderr, "NOTICE - Finished phase: Optimize likelihood  [%.3f seconds]\n", out->seconds_optimize);
    return rc;
}

// --Devices a,b,...: the sample's markers sharded over the devices (vb2_shard_group_*)
int search_on_shards(const vb2_run_args* a, const vb2_flat& flat, const vb2_model& model, const RunClock& clock, vb2_run_result* out)
{
    if (a->search.num_start > 1 || a->search.line_search) {      // (never silently ignored)
        set_error("--NumStart / --LineSearch are single-device options: they cannot be combined with marker "
                  "shards over several --Devices");
        return VB2_ERR_INVALID;
    }
    const bool notices = model.notices != 0;
    vb2_shard_group* created = nullptr;
    if (const int rc = vb2_shard_group_create(&flat.input, a->devices, a->num_device, &created)) return rc;
    std::unique_ptr<vb2_shard_group, ShardGroupDestroy> grp(created);
    out->seconds_load = now_s() - clock.t0;
    if (notices)
        std::fprintf(stderr, "NOTICE - Finished phase: Flatten + upload to %d devices (marker shards, %s)  "
                             "[%.3f seconds]\n", (int)a->num_device,
                     grp->impl->use_rccl ? "RCCL all-reduce" : "host sum", now_s() - clock.t_flat0);
    return timed_search(notices, out, [&] { return vb2_shard_group_optimize_llk(grp.get(), &model, &out->est, nullptr); });
}

// one context, and the stage's work on it after a successful search
int search_on_context(const vb2_run_args* a, const vb2_flat& flat, const vb2_model& model, const RunClock& clock, const RunStage& stage,
                      vb2_run_result* out)
{
    const bool notices = model.notices != 0;
    vb2_options opt{};
    opt.device = (a->devices && a->num_device == 1) ? a->devices[0] : a->device;
    vb2_ctx* created = nullptr;
    if (const int rc = stage.err_table ? vb2_ctx_create_ex(&flat.input, &opt, stage.err_table, &created)
                                       : vb2_ctx_create(&flat.input, &opt, &created))
        return rc;
    std::unique_ptr<vb2_ctx, CtxDestroy> ctx(created);
    out->seconds_load = now_s() - clock.t0;
    if (notices)
        std::fprintf(stderr, "NOTICE - Finished phase: Flatten + upload to %s  [%.3f seconds]\n", ctx->impl->device_name,
                     now_s() - clock.t_flat0);
    const int rc = timed_search(notices, out, [&] {
        return (a->search.num_start > 1 || a->search.line_search) ? vb2_ctx_optimize_llk_ex(ctx.get(), &model, &a->search, &out->est, nullptr)
                                                                   : vb2_ctx_optimize_llk(ctx.get(), &model, &out->est, nullptr);
    });
    if (rc || !stage.on_context) return rc;
    return stage.on_context(ctx.get(), flat, model, out->est);
}

}  // namespace

int load_panel(const vb2_run_args* a, Panel* panel)
{
    PanelLoad load(a, panel);
    return load.finish();
}

int flat_load(const vb2_run_args* a, vb2_flat** out, vb2_flat_groups* groups)
{
    if (!a || !out || !a->ud_path || !a->mean_path || !a->bed_path || (!a->pileup_path && !a->bam_path) ||
        a->num_pc < 1 || a->num_pc > VB2_MAX_PC || (groups && (a->pileup_path || !a->bam_path))) {
        set_error(groups ? "vb2_flat_load_groups: invalid argument (read groups are read from bam_path alone)" : "vb2_flat_load: invalid argument");
        return VB2_ERR_INVALID;
    }
    *out = nullptr;
    if (a->bam_adjust != 0 && a->bam_adjust != 1) {
        set_error("vb2_flat_load: bam_adjust is " + std::to_string(a->bam_adjust) + "; it is 0 (BAM records as they are) or 1 (--ApplyBAQ)");
        return VB2_ERR_INVALID;
    }
    if (a->bam_adjust == 1 && a->bam_path && !a->pileup_path && !a->reference_path) {
        set_error("vb2_flat_load: bam_adjust = 1 (--ApplyBAQ) needs reference_path, the FASTA the BAM was aligned to");
        return VB2_ERR_INVALID;
    }
    return guarded([&]() -> int {
        std::unique_ptr<vb2_flat> f(new vb2_flat());
        f->panel.numPC = a->num_pc;
        // constructor reads the .bed (ContaminationEstimator.cpp:47), then ReadSVDMatrix
        // The four files are independent until the markers are resolved: .UD and .mu are parsed
        // on two helper threads while this one reads the .bed (the pileup reader needs it) and
        // the pileup.  Errors are reported in the reference's reading order (.bed, AF, .UD, .mu).
        const bool timing = tunables().debug_timing != 0;
        const double tl0 = now_s();
        PanelLoad load(a, &f->panel);
        const double tl_bed = now_s();
        int rc_pile = VB2_OK;
        std::string err_pile;
        if (load.bed_ok() && (rc_pile = read_sample(a, f.get(), groups))) err_pile = g_last_error;
        const double tl_pile = now_s();
        if (const int rc = load.finish()) return rc;
        const double tl_join = now_s();
        if (rc_pile) { set_error(err_pile); return rc_pile; }
        f->sanity_disabled = a->disable_sanity != 0;
        if (!f->sanity_disabled && !sanity_check(f->panel, &f->viewer)) {
            if (groups)
                for (size_t g = 0; g < groups->flat.size(); ++g) finish_group(a, g, groups);
            set_error("Insufficient Available markers, check input bam depth distribution in "
                      "output pileup file after specifying --OutputPileup");
            f->resolve();
            *out = f.release();
            return VB2_ERR_SANITY;
        }
        const double tl_san = now_s();
        f->resolve();
        if (groups)
            for (size_t g = 0; g < groups->flat.size(); ++g) finish_group(a, g, groups);
        if (timing)
            std::fprintf(stderr, "vb2_flat_load: .bed %.1f ms, pileup %.1f ms, wait for .UD/.mu %.1f ms, "
                         "sanity %.1f ms, resolve %.1f ms\n", 1e3 * (tl_bed - tl0), 1e3 * (tl_pile - tl_bed),
                         1e3 * (tl_join - tl_pile), 1e3 * (tl_san - tl_join), 1e3 * (now_s() - tl_san));
        *out = f.release();
        return VB2_OK;
    });
}

int run_sample(const vb2_run_args* a, vb2_run_result* out, const RunStage& stage, vb2_flat_groups* groups)
{
    if (!a || !out) {
        set_error("vb2_run: invalid argument");
        return VB2_ERR_INVALID;
    }
    RunClock clock;
    clock.t0 = now_s();
    // HIP runtime start-up on a helper thread, while this one reads the input files
    std::thread warm(warm_device, (int)a->device);
    JoinGuard j_warm(warm);
    vb2_flat* loaded = nullptr;
    const bool notices = a->model.notices != 0;
    // main.cpp:321-378: the reference times "Load SVD reference data", "Read pileup" and "Marker
    // sanity check" one after the other; here the panel files and the pileup are read
    // concurrently, so the three are one phase
    if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Load SVD reference data + Read pileup + Marker sanity check\n");
    int rc = flat_load(a, &loaded, groups);
    std::unique_ptr<vb2_flat> flat(loaded);
    warm.join();
    if (notices) {
        std::fprintf(stderr, "NOTICE - Finished phase: Load SVD reference data + Read pileup + Marker sanity check  "
                             "[%.3f seconds]\n", now_s() - clock.t0);
        if (!rc && !a->disable_sanity) std::fprintf(stderr, "NOTICE - Passing Marker Sanity Check...\n");
    }
    if (rc == VB2_ERR_SANITY && flat && a->output_pileup && a->output_prefix) write_pileup(a->output_prefix, *flat);
    if (rc) return rc;
    vb2_flat_stats(flat.get(), out);
    if (a->output_pileup && a->output_prefix && (rc = write_pileup(a->output_prefix, *flat))) return rc;

    vb2_model model = a->model;
    if (flat->panel.isAFknown) model.is_af_known = 1;
    clock.t_flat0 = now_s();
    rc = a->devices && a->num_device > 1 ? search_on_shards(a, *flat, model, clock, out)
                                         : search_on_context(a, *flat, model, clock, stage, out);
    if (rc) return rc;

    print_summary(estimation_title(model), a->num_pc, out->est);
    if (a->output_prefix) {
        if ((rc = write_ancestry(a->output_prefix, a->num_pc, out->est.pc, out->est.pc2))) return rc;
        // main.cpp:398-400: #READS is viewer.numBases for BAM input, "NA" for pileup input
        if ((rc = write_selfsm(a->output_prefix, *flat, out->est, a->pileup_path != nullptr))) return rc;
    }
    return stage.after_writers ? stage.after_writers(*a) : VB2_OK;
}

}  // namespace vb2
