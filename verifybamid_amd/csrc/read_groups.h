// read_groups.h -- the search of a BAM's read groups behind the whole sample's run (--PerReadGroup, vb2_run_read_groups;
// DESIGN.md section 19).  The groups' pileups come from the load (bam_flatten.cpp, vb2_flat_load_groups).
#ifndef VB2_READ_GROUPS_H_
#define VB2_READ_GROUPS_H_

#include "hostio.h"

namespace vb2 {

constexpr int kReadGroupBatch = 64;      // groups searched in lock-step at a time

// A context per group with status VB2_OK, batches of at most kReadGroupBatch searched with vb2_batch_optimize_llk under the
// run's model; <output_prefix>.selfRG and, with output_pileup, <output_prefix>.RG<index>.Pileup; results [capacity].
int run_read_groups_stage(const vb2_run_args* args, vb2_flat_groups* groups, int32_t capacity, vb2_group_result* results,
                          int32_t* num_group);

}  // namespace vb2

#endif
