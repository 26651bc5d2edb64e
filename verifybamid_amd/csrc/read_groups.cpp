// read_groups.cpp -- FREEMIX per read group of one BAM (read_groups.h): every group is a small
// sample over the whole sample's panel, and many small samples searched at once is what the lock-step batch does.
#include "read_groups.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"   // set_error
#include "host_clock.h"

namespace vb2 {
namespace {

struct CtxList {         // every exit path destroys what was created
    std::vector<vb2_ctx*> v;
    ~CtxList() { for (vb2_ctx* c : v) vb2_ctx_destroy(c); }
};
struct BatchHolder {
    vb2_batch* b = nullptr;
    ~BatchHolder() { if (b) vb2_batch_destroy(b); }
};

}  // namespace

int run_read_groups_stage(const vb2_run_args* a, vb2_flat_groups* groups, int32_t capacity, vb2_group_result* results,
                          int32_t* num_group)
{
    const size_t G = groups->flat.size();
    *num_group = (int32_t)G;
    const bool notices = a->model.notices != 0;
    vb2_model model = a->model;
    if (G > 0 && groups->flat[0]->panel.isAFknown) model.is_af_known = 1;
    std::vector<vb2_estimate> est(G);
    std::vector<uint8_t> searched(G, 0);
    std::vector<double> seconds(G, 0.0);
    if (G > 0) std::memset(est.data(), 0, G * sizeof(vb2_estimate));
    const double t0 = now_s();
    if (notices) std::fprintf(stderr, "NOTICE - Starting phase: Optimize likelihood of %zu read groups\n", G);
    std::vector<size_t> todo;
    for (size_t g = 0; g < G; ++g)
        if (groups->info[g].status == VB2_OK) todo.push_back(g);
    vb2_options opt{};
    opt.device = (a->devices && a->num_device == 1) ? a->devices[0] : a->device;
    opt.flags = VB2_OPT_COHORT_LAYOUT;       // the lock-step search streams the 16-bit run lists
    for (size_t b0 = 0; b0 < todo.size(); b0 += (size_t)kReadGroupBatch) {
        const size_t b1 = std::min(todo.size(), b0 + (size_t)kReadGroupBatch);
        const double tb = now_s();
        CtxList ctxs;
        for (size_t k = b0; k < b1; ++k) {
            vb2_ctx* c = nullptr;
            if (int rc = vb2_ctx_create(&groups->flat[todo[k]]->input, &opt, &c)) return rc;
            ctxs.v.push_back(c);
        }
        BatchHolder batch;
        std::vector<vb2_estimate> got(b1 - b0);
        if (int rc = vb2_batch_create(ctxs.v.data(), (int32_t)ctxs.v.size(), &batch.b)) return rc;
        if (int rc = vb2_batch_optimize_llk(batch.b, &model, 1, got.data())) return rc;
        const double dt = (now_s() - tb) / (double)(b1 - b0);
        for (size_t k = b0; k < b1; ++k) {
            est[todo[k]] = got[k - b0];
            searched[todo[k]] = 1;
            seconds[todo[k]] = dt;
        }
    }
    if (notices)
        std::fprintf(stderr, "NOTICE - Finished phase: Optimize likelihood of %zu read groups (%zu searched)  [%.3f seconds]\n", G,
                     todo.size(), now_s() - t0);
    for (size_t g = 0; g < G && g < (size_t)capacity; ++g) {
        vb2_group_result& r = results[g];
        std::memset(&r, 0, sizeof(r));
        vb2_flat_stats(groups->flat[g].get(), &r.run);
        r.run.est = est[g];
        r.run.seconds_optimize = seconds[g];
        r.status = groups->info[g].status;
        r.header_index = (int32_t)g;
        r.records = groups->info[g].records;
    }
    if (a->output_prefix) {
        if (int rc = write_selfrg(a->output_prefix, *groups, est.data(), searched.data())) return rc;
        if (a->output_pileup)
            for (size_t g = 0; g < G; ++g)
                if (int rc = write_pileup(std::string(a->output_prefix) + ".RG" + std::to_string(g), *groups->flat[g])) return rc;
    }
    if (notices)
        for (size_t g = 0; g < G; ++g) {
            const vb2_flat_groups::Info& gi = groups->info[g];
            if (searched[g])
                std::fprintf(stderr, "NOTICE - read group %s: FREEMIX %g over %d bases\n", gi.id.c_str(),
                             est[g].alpha < 0.5 ? est[g].alpha : 1 - est[g].alpha, groups->flat[g]->viewer.numBases);
            else
                std::fprintf(stderr, "NOTICE - read group %s: not searched (%s)\n", gi.id.c_str(),
                             gi.status == VB2_GROUP_NO_BASE ? "no base at any marker" : "its marker sanity check failed");
        }
    return VB2_OK;
}

}  // namespace vb2
