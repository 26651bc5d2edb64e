// panel.h -- the --RefVCF reference-panel builder (SVDcalculator::ProcessRefVCF, SVDcalculator.cpp:363-400):
// the VCF reader (vcf_panel.cpp, host only), the device pipeline (panel.cpp + panel_kernels.hip).
#ifndef VB2_PANEL_H_
#define VB2_PANEL_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/vb2_abi.h"

namespace vb2 {

// what ReadVcf keeps of each marker (BedVec + chooseBed, SVDcalculator.cpp:211-213) and the sample names (:108)
struct VcfMarkers {
    std::vector<std::string> chr_names;   // distinct chromosome names in order of first appearance
    std::vector<int32_t> chr_index;       // [M] into chr_names
    std::vector<int32_t> pos;             // [M] 1-based POS
    std::vector<char> ref, alt;           // [M] upper-cased single bases
    std::vector<std::string> samples;     // [N]
    int32_t num_sample = 0;
    int64_t num_marker = 0;
};

// Receives the kept markers' genotypes in file order, marker-major (count x num_sample int8, -1 = missing), in
// blocks of any size; first = index of the block's first marker.  Called on the reading thread.
// Returns VB2_OK to go on; anything else stops the reader, which returns that code (the sink set the error).
using GenotypeSink = std::function<int(const int8_t* block, int64_t first, int64_t count)>;
// Called once the header has been read (num_sample known), before any block.
using HeaderSink = std::function<void(int32_t num_sample)>;

// SVDcalculator::ReadVcf rule for rule.  includeChr empty = no chromosome filter.  One inflating thread,
// num_thread parsers over blocks of lines, marker order kept.  Returns VB2_OK or a VB2_ERR_* with set_error()
// (the reference's fatal errors are VB2_ERR_INVALID, unreadable files VB2_ERR_IO).
int read_vcf(const std::string& path, const std::unordered_set<std::string>& includeChr, int num_thread,
             bool notices, VcfMarkers* markers, const HeaderSink& on_header, const GenotypeSink& sink);

// main.cpp:69-73: the 44 autosome names, with and without "chr"
std::unordered_set<std::string> parse_include_chr(const char* list /* NULL = the default */);

// kernels (panel_kernels.hip)
// tiles: the slab is N_pad rows (samples) x K columns (markers) int8, row pitch = ld bytes.
constexpr int kGramTile = 64;      // output tile edge (samples); N is padded to it
constexpr int kGramKStep = 128;    // markers per LDS stage; chunk widths are multiples of it
hipError_t launch_transpose_chunk(const int8_t* src /* count x N marker-major */, int64_t count, int32_t n,
                                  int8_t* dst /* n_pad x ld sample-major */, int64_t ld, hipStream_t s);
hipError_t launch_row_sums(const int8_t* src /* count x N marker-major */, int64_t count, int32_t n,
                           int32_t* sums, hipStream_t s);
hipError_t launch_mu_from_sums(const int32_t* sums, int64_t count, int32_t n, double* mu, hipStream_t s);
hipError_t launch_gram_chunk(const int8_t* slab, int64_t ld, int64_t k_len, int32_t n_pad, int32_t* S /* n_pad^2 */,
                             hipStream_t s);
hipError_t launch_sample_dot_mu(const int8_t* slab, int64_t ld, int64_t k_len, int32_t n, const double* mu,
                                double* c /* [n], accumulated */, hipStream_t s);
hipError_t launch_centre_gram(const int32_t* S, int32_t n_pad, int32_t n, const double* c, const double* tau,
                              double* C /* n x n */, hipStream_t s);
hipError_t launch_sum_squares(const double* mu, int64_t m, double* tau, hipStream_t s);
hipError_t launch_project(const int8_t* slab, int64_t ld, int64_t k_len, int32_t n, const double* V /* n x k */,
                          int32_t k, const double* mu, const double* vsum, double* UD /* k_len x k */, hipStream_t s);

}  // namespace vb2

#endif  // VB2_PANEL_H_
