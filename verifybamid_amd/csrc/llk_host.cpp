// llk_host.cpp -- what the evaluation launches need from the host that touches no kernel symbol: the static deal's
// schedule and the test for a profiler in the process.  (resident_state_doubles and resident_cache_rows share their
// layout rules with resident_kernel.inc and stay with it in llk_kernels.hip.)
#include "llk_kernels.h"

#include <link.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace vb2 {

bool build_schedule(const uint32_t* rows, int num_mt, int nblk, int nwave, int tpu, int ngrp,
                    std::vector<uint32_t>* off, std::vector<uint16_t>* item, int own_shift)
{
    off->clear();
    item->clear();
    if (num_mt <= 0 || nblk <= 0 || nwave <= 0) return false;
    const uint32_t max_tiles = owned_most(own_shift, (uint32_t)num_mt, (uint32_t)nblk);
    if ((size_t)((max_tiles + tpu - 1) / tpu) * ngrp > 65535) return false;
    off->reserve((size_t)nblk * nwave + 1);
    std::vector<uint64_t> load(nwave);
    std::vector<std::vector<uint16_t>> mine(nwave);
    // cost model (VALU instructions per lane): 28 per row of two runs x two points, ~370 for the
    // per-marker epilogue and the item's fixed work; only the ratio matters
    constexpr uint64_t kRowCost = 28, kFixCost = 370;
    for (int b = 0; b < nblk; ++b) {
        const uint32_t ntile = owned_count(own_shift, (uint32_t)num_mt, (uint32_t)b, (uint32_t)nblk);
        const uint32_t nunit = (ntile + tpu - 1) / tpu;
        std::fill(load.begin(), load.end(), 0);
        for (auto& v : mine) v.clear();
        // the workgroup's tiles b, b + nblk, ... are in descending row order, so walking the units
        // in index order IS longest-first
        for (uint32_t u = 0; u < nunit; ++u) {
            uint32_t r = 0;
            for (int h = 0; h < tpu; ++h) {
                const uint32_t it = (uint32_t)tpu * u + h;
                if (it < ntile) r = std::max(r, rows[owned_tile(own_shift, (uint32_t)b, (uint32_t)nblk, it)]);
            }
            const uint64_t cost = kRowCost * r + kFixCost;
            for (int g = 0; g < ngrp; ++g) {
                int best = 0;
                for (int w = 1; w < nwave; ++w)
                    if (load[w] < load[best]) best = w;
                load[best] += cost;
                mine[best].push_back((uint16_t)((uint32_t)g * nunit + u));
            }
        }
        for (int w = 0; w < nwave; ++w) {
            std::sort(mine[w].begin(), mine[w].end());       // by (group, unit): few group changes per wave
            off->push_back((uint32_t)item->size());
            item->insert(item->end(), mine[w].begin(), mine[w].end());
        }
    }
    off->push_back((uint32_t)item->size());
    return true;
}

// A profiler's tool library in the process (rocprofv3 preloads librocprofiler-sdk-tool.so; rocprof v1/v2 their own)?
bool profiler_attached()
{
    static const bool attached = [] {
        bool found = false;
        dl_iterate_phdr(
            [](struct dl_phdr_info* info, size_t, void* data) -> int {
                const char* n = info->dlpi_name;
                if (n && (std::strstr(n, "rocprofiler-sdk-tool") || std::strstr(n, "librocprofiler64") ||
                          std::strstr(n, "libroctracer") || std::strstr(n, "rocprofv3"))) {
                    *static_cast<bool*>(data) = true;
                    return 1;
                }
                return 0;
            },
            &found);
        return found;
    }();
    return attached;
}

}  // namespace vb2
