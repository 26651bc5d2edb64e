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
    // with a BlockInflater: the blocks it was given, those of them it refused (inflated again by zlib), and the host pool's
    // wall-clock over CRC32 and those fallbacks (a block whose bytes missed the CRC32 counts as refused)
    int64_t inflater_blocks = 0, inflater_refused = 0;
    double seconds_inflater = 0, seconds_crc = 0;
};

// The hook for inflating the planned blocks somewhere else than on the host pool.  An item is one
// BGZF block: its deflate payload, and where its ISIZE bytes belong.  run() fills status[i] for every item: 0 = dst holds
// the isize inflated bytes; any other value = the block is the host's (zlib inflates it again, and zlib's verdict stands,
// so a corrupt file ends in the same code and message with and without an inflater).  The host checks the CRC32 of every
// block the inflater accepted; one whose bytes miss it is the host's again as well.  The return value is kOk, or a code
// of this header with *err set for a failure that is no block's own (the scan ends with it).
struct InflateItem {
    const uint8_t* raw;
    uint32_t raw_len;
    uint8_t* dst;
    uint32_t isize;
};
class BlockInflater {
public:
    virtual ~BlockInflater() {}
    virtual int run(const InflateItem* items, size_t n, int32_t* status, std::string* err) = 0;
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
// inflater (may be null): the planned blocks of all chunks go through it (above); the header's blocks and the tail blocks a
// straddling record pulls in stay on zlib.  Without one the scan is what it was before the hook existed.
int scan(const std::string& bam_path, const std::vector<SeqMarkers>& markers, int threads, Scan* out, std::string* err,
         bool want_groups = false, BlockInflater* inflater = nullptr);

// The BGZF blocks of a buffer, back to back from offset 0 to its end, with the scan's own header checks: per block the
// offset and length of its deflate payload, its ISIZE and its CRC32 field.  kErrIo / kErrInvalid with *err otherwise
// (`name` stands for the file in the messages).
struct BlockSpan {
    uint64_t raw_off;
    uint32_t raw_len, isize, crc;
};
int list_bgzf_blocks(const uint8_t* bytes, uint64_t n, const std::string& name, std::vector<BlockSpan>* out, std::string* err);

}  // namespace bamio
}  // namespace vb2

#endif
