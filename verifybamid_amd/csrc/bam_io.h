// bam_io.h -- the host stage of the built-in BAM reader: BGZF, the BAM header, the .bai index and
// the record chain, with nothing but C++17 and zlib.  No HIP header and nothing of context.h, so that the unit compiles
// stand-alone (tests/bam_io_check_main.cpp links it with -lz alone and runs it under the host sanitizers).
//
// What it hands on is what the device stage (bam_pileup_kernels.hip) may trust without looking again: every record of a
// chunk has a 32-byte descriptor whose variable part -- name, CIGAR, packed bases, qualities -- lies inside the chunk's
// inflated bytes.  Every malformed input ends in an error code with a message, never in an out-of-range read.
#ifndef VB2_BAM_IO_H_
#define VB2_BAM_IO_H_

#include <cstdint>
#include <string>
#include <vector>

namespace vb2 {
namespace bamio {

// the C-ABI's codes (include/vb2_abi.h), restated so that this header stands alone
constexpr int kOk = 0, kErrInvalid = -1, kErrIo = -4, kErrNoMem = -5;

// One record, as the cover kernel reads it.  `data` is the byte offset of the record's variable part (the read name)
// within its chunk's bytes on the host and within the batch's bytes on the device.
struct RecordDesc {
    uint32_t data;
    int32_t tid;
    int32_t pos;
    uint16_t flag;
    uint8_t mapq;
    uint8_t l_read_name;
    uint16_t n_cigar;
    uint16_t mate_same;      // mtid == tid (all the pileup asks of mtid; the field itself would make the descriptor 36 bytes)
    int32_t l_seq;
    int32_t mpos;
    uint32_t order;          // file-order number: ascending with the record's virtual offset
};
static_assert(sizeof(RecordDesc) == 32, "descriptors are 32 bytes");

// One @RG line of the header.  Only the ID is needed downstream; SM, LB and PU are there for whoever writes a report.
struct ReadGroup {
    std::string id, sm, lb, pu;
};
constexpr uint16_t kNoGroup = 0xFFFF;        // a record without an RG:Z field, or with an ID the header lacks
constexpr size_t kMaxGroups = 0xFFFF;

struct Chunk {               // one merged run of the index's chunks, inflated
    int32_t tid = -1;
    uint64_t beg = 0, end = 0;               // virtual offsets
    std::vector<uint8_t> bytes;              // inflated blocks back to back, from beg's block on
    std::vector<RecordDesc> recs;            // the records that start in [beg, end) on `tid` and may reach a marker
    std::vector<uint64_t> voffset;           // ... and their virtual offsets
    std::vector<uint16_t> group;             // ... and, when the scan was asked for groups, their index into Scan::groups
};

struct Stats {
    int64_t blocks = 0, bytes_inflated = 0, records_seen = 0, records_kept = 0, long_cigar_skipped = 0, chunks = 0;
    int64_t records_unassigned = 0;          // kept records of no group (0 when groups were not asked for)
    double seconds_index = 0, seconds_inflate = 0;
};

// The markers of one reference sequence: sorted distinct 1-based positions.
struct SeqMarkers {
    std::string name;
    std::vector<int32_t> pos;
};

struct Scan {
    std::string sample = "DefaultSampleName";
    std::vector<std::string> ref_name;
    std::vector<int64_t> ref_len;
    std::vector<int32_t> tid_of_seq;         // per entry of the markers passed in: its tid in the header, -1 = absent
    std::vector<Chunk> chunks;               // ascending by (tid, beg)
    std::vector<ReadGroup> groups;           // the header's @RG lines in header order (filled only when asked for)
    Stats stats;
};

// Opens bam_path and its index (<bam>.bai, else <stem>.bai), plans the chunks that can hold a record over one of the
// markers, inflates every block once on a pool of `threads` threads (<= 16) and walks the records.  kErrIo / kErrInvalid
// with *err set otherwise.
// want_groups: also parse the header's @RG lines into out->groups (two lines with one ID, a line without ID or more than
// 65 535 lines: kErrInvalid) and walk every kept record's auxiliary fields for its RG:Z, into Chunk::group.  Without it the
// auxiliary bytes are not looked at.
int scan(const std::string& bam_path, const std::vector<SeqMarkers>& markers, int threads, Scan* out, std::string* err,
         bool want_groups = false);

}  // namespace bamio
}  // namespace vb2

#endif
