// run.h -- the file flow of ONE sample (--SVDPrefix with --PileupFile or --BamFile; run.cpp): the panel loader, the load
// of a sample's files, and the run itself -- load, context or marker shards, search, the reference's summary and files.
// What a feature does with the searched sample is a RunStage; the extern "C" entries (abi.cpp, abi_input.cpp,
// interval.cpp, replicates.cpp, refbias.cpp) check their arguments and forward here.
#ifndef VB2_RUN_H_
#define VB2_RUN_H_

#include <functional>

#include "../../include/vb2_abi.h"

struct vb2_flat;
struct vb2_flat_groups;

namespace vb2 {

struct Panel;

// The panel files of a run: .UD and .mu parsed on helper threads while the caller's thread reads the .bed (and the AF
// file); errors in the reference's reading order (.bed, AF, .UD, .mu), then the check of .UD's rows against the others'.
int load_panel(const vb2_run_args* a, Panel* panel);

// vb2_flat_load, and with groups != nullptr vb2_flat_load_groups: the panel as load_panel reads it, the pileup or BAM
// read behind the .bed while .UD and .mu are still being parsed (its error is reported after the panel's), the sanity
// check and BuildResolvedMarkers.  VB2_ERR_SANITY leaves *out set.  Catches what its body throws.
int flat_load(const vb2_run_args* a, vb2_flat** out, vb2_flat_groups* groups);

// What a run does with its searched sample beyond vb2_run, in the two places a feature has work to do.  A non-zero return
// fails the run; either may be empty.
struct RunStage {
    // on the run's context (one device) after a successful search, before the summary and .Ancestry / .selfSM
    std::function<int(vb2_ctx* ctx, const vb2_flat& flat, const vb2_model& model, const vb2_estimate& est)> on_context;
    // after the run's own writers
    std::function<int(const vb2_run_args& args)> after_writers;
    // [VB2_ERR_NUM_QUAL] or null: the run's context is made under this error table (vb2_ctx_create_ex; one device)
    const double* err_table = nullptr;
};

// vb2_run with a stage; groups (may be null): loaded beside the whole sample (vb2_run_read_groups searches them afterwards).
// May throw what a stage or a writer throws: callers sit inside vb2::guarded.
int run_sample(const vb2_run_args* a, vb2_run_result* out, const RunStage& stage = RunStage(), vb2_flat_groups* groups = nullptr);

}  // namespace vb2
#endif
