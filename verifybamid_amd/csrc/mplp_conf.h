// mplp_conf.h -- the reference's mpileup configuration as both BAM readers apply it (bam_flatten.cpp, bam_htslib.cpp).
#ifndef VB2_MPLP_CONF_H_
#define VB2_MPLP_CONF_H_

#include <cstdint>

#include "../../include/vb2_abi.h"

namespace vb2 {

// the reference's mode bits of mplp.flag (SimplePileupViewer.h:14-24) -- `--incl-flags` stores its value THERE
// (main.cpp:185-186), not in a required-read-flags mask: kept
constexpr int kMplpNoOrphan = 1 << 3, kMplpRealn = 1 << 4, kMplpIllumina13 = 1 << 7, kMplpRedoBaq = 1 << 6,
              kMplpSmartOverlaps = 1 << 10;

struct MplpConf {                      // main.cpp:81-96
    int min_mq = 2, min_baseQ = 13, capQ_thres = 40, max_depth = 8000;
    int flag = kMplpRealn | kMplpSmartOverlaps;
    uint32_t rflag_filter = 4 | 256 | 512 | 1024;      // UNMAP | SECONDARY | QCFAIL | DUP
    void apply(const vb2_mpileup_opts* mp)      // main.cpp:176-187, 208-211
    {
        if (!mp || !mp->given) return;
        min_baseQ = mp->min_bq;
        min_mq = mp->min_mq;
        capQ_thres = mp->adjust_mq;
        max_depth = mp->max_depth;
        flag = mp->incl_flags;
        if (mp->no_orphans) flag |= kMplpNoOrphan;
        else flag &= ~kMplpNoOrphan;
        rflag_filter = (uint32_t)mp->excl_flags;
    }
};

}  // namespace vb2

#endif
