// bam_io.cpp -- BGZF blocks, the BAM header, the .bai index and the record chain (bam_io.h).
//
// Formats as in the SAM/BAM specification (SAMv1, sections 4.1, 4.2 and 5.2): a BGZF block is a gzip member whose extra
// field carries the subfield 'B' 'C' with BSIZE = block size - 1; a virtual offset is (offset of the block in the file)
// << 16 | (offset within the inflated block); a record is block_size followed by 32 bytes of fixed fields and the name,
// CIGAR, packed bases and qualities; the index has, per reference sequence, the chunks of every bin and the linear index
// of 16 kb windows.
#include "bam_io.h"
#include "host_clock.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

namespace vb2 {
namespace bamio {
namespace {

constexpr uint32_t kMaxRecord = 64u << 20;       // a record larger than this is taken for a corrupt block_size
constexpr int kBinPseudo = 37450;

struct Fail {
    int code;
    std::string msg;
};

uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

struct File {
    int fd = -1;
    uint64_t size = 0;
    std::string path;
    ~File() { if (fd >= 0) ::close(fd); }
    bool open(const std::string& p)
    {
        path = p;
        fd = ::open(p.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return false;
        size = (uint64_t)st.st_size;
        return true;
    }
    // exactly n bytes at off, or Fail
    void read(uint64_t off, size_t n, uint8_t* dst) const
    {
        if (off > size || n > size - off) throw Fail{kErrIo, path + ": truncated (a read of " + std::to_string(n) + " bytes at " + std::to_string(off) + " passes the end of the file)"};
        size_t got = 0;
        while (got < n) {
            const ssize_t r = ::pread(fd, dst + got, n - got, (off_t)(off + got));
            if (r <= 0) throw Fail{kErrIo, path + ": read error at offset " + std::to_string(off + got)};
            got += (size_t)r;
        }
    }
};

struct BlockHead {
    uint32_t size;      // whole block in the file
    uint32_t data_off;  // compressed data within it
    uint32_t data_len;
};

// The gzip member header at `p` (`avail` bytes of the file from there on): magic, FEXTRA, the BC subfield, BSIZE.
BlockHead parse_block_head(const File& f, uint64_t off, const uint8_t* p, uint64_t avail)
{
    const std::string at = f.path + ": BGZF block at " + std::to_string(off) + ": ";
    if (avail < 18) throw Fail{kErrIo, at + "truncated header"};
    if (p[0] != 31 || p[1] != 139 || p[2] != 8) throw Fail{kErrInvalid, at + "not a gzip member (bad magic)"};
    if (!(p[3] & 4)) throw Fail{kErrInvalid, at + "no extra field (not BGZF)"};
    const uint32_t xlen = le16(p + 10);
    if (12ull + xlen > avail) throw Fail{kErrIo, at + "truncated extra field"};
    int64_t bsize = -1;
    for (uint32_t i = 0; i + 4 <= xlen;) {
        const uint8_t* s = p + 12 + i;
        const uint32_t slen = le16(s + 2);
        if (i + 4 + slen > xlen) throw Fail{kErrInvalid, at + "extra subfield passes the extra field"};
        if (s[0] == 'B' && s[1] == 'C') {
            if (slen != 2) throw Fail{kErrInvalid, at + "BC subfield of length " + std::to_string(slen)};
            bsize = le16(s + 4);
        }
        i += 4 + slen;
    }
    if (bsize < 0) throw Fail{kErrInvalid, at + "no BC subfield in the extra field (gzip, but not BGZF)"};
    BlockHead h;
    h.size = (uint32_t)bsize + 1;
    h.data_off = 12 + xlen;
    if (h.size < h.data_off + 8) throw Fail{kErrInvalid, at + "BSIZE " + std::to_string(bsize) + " is smaller than the block's own header"};
    if (h.size > avail) throw Fail{kErrIo, at + "BSIZE " + std::to_string(bsize) + " passes the end of the file"};
    h.data_len = h.size - h.data_off - 8;
    return h;
}

// Inflates the block whose `h.size` bytes are at p into dst (ISIZE bytes, which the caller reserved), checking CRC32 and ISIZE.
void inflate_block(const File& f, uint64_t off, const uint8_t* p, const BlockHead& h, uint8_t* dst, uint32_t isize)
{
    const std::string at = f.path + ": BGZF block at " + std::to_string(off) + ": ";
    const uint32_t crc = le32(p + h.size - 8);
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) throw Fail{kErrNoMem, "zlib: inflateInit2 failed"};
    uint8_t dummy = 0;                                   // an empty block (the end-of-file marker) still needs somewhere to write
    zs.next_in = const_cast<uint8_t*>(p + h.data_off);
    zs.avail_in = h.data_len;
    zs.next_out = isize ? dst : &dummy;
    zs.avail_out = isize ? isize : 1;
    const int rc = inflate(&zs, Z_FINISH);
    const uint64_t produced = zs.total_out;
    inflateEnd(&zs);
    if (rc != Z_STREAM_END) {
        if (rc == Z_BUF_ERROR || rc == Z_OK) throw Fail{kErrInvalid, at + "the data inflates to more than its ISIZE " + std::to_string(isize) + " (or is cut short)"};
        throw Fail{kErrInvalid, at + "inflate failed (corrupt deflate stream)"};
    }
    if (produced != isize) throw Fail{kErrInvalid, at + "inflated to " + std::to_string(produced) + " bytes, ISIZE says " + std::to_string(isize)};
    const uint32_t got = (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, isize);
    if (got != crc) throw Fail{kErrInvalid, at + "CRC32 mismatch"};
}

// Whether dst holds the bytes the block's CRC32 field names (a block that something else than inflate_block inflated).
bool crc_matches(const uint8_t* p, const BlockHead& h, const uint8_t* dst, uint32_t isize)
{
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, isize) == le32(p + h.size - 8);
}

// A run of blocks read and inflated one after the other: the header, and the tail of a chunk whose last record straddles.
struct Stream {
    const File& f;
    uint64_t next;                          // file offset of the next block
    std::vector<uint8_t>* out;
    std::vector<std::pair<uint64_t, uint64_t>>* blocks;   // (file offset, offset in *out) of every block appended
    int64_t* nblocks;
    // appends one block; false at the end of the file (or at the empty end-of-file block when nothing follows)
    bool more()
    {
        if (next >= f.size) return false;
        uint8_t head[18 + 256];
        const uint64_t avail = f.size - next;
        const size_t nh = (size_t)std::min<uint64_t>(avail, sizeof(head));
        f.read(next, nh, head);
        // (an extra field longer than what `head` holds is re-read below with the whole block)
        uint32_t xlen = nh >= 12 ? le16(head + 10) : 0;
        std::vector<uint8_t> raw;
        const uint8_t* p = head;
        if (12ull + xlen > nh && 12ull + xlen <= avail) {
            raw.resize(12 + xlen);
            f.read(next, raw.size(), raw.data());
            p = raw.data();
        }
        BlockHead h = parse_block_head(f, next, p, avail);
        std::vector<uint8_t> whole(h.size);
        f.read(next, h.size, whole.data());
        const uint32_t isize = le32(whole.data() + h.size - 4);
        if (isize > 65536) throw Fail{kErrInvalid, f.path + ": BGZF block at " + std::to_string(next) + ": ISIZE " + std::to_string(isize) + " exceeds 65536"};
        const size_t at = out->size();
        out->resize(at + isize);
        inflate_block(f, next, whole.data(), h, out->data() + at, isize);
        if (blocks) blocks->emplace_back(next, (uint64_t)at);
        if (nblocks) ++*nblocks;
        next += h.size;
        return true;
    }
};

std::string sample_of(const std::string& text, bool* several)      // @RG SM: (SimplePileupViewer.cpp:296-314)
{
    std::string sm;
    *several = false;
    size_t line = 0;
    while (line < text.size()) {
        size_t eol = text.find('\n', line);
        if (eol == std::string::npos) eol = text.size();
        if (eol - line >= 3 && text.compare(line, 3, "@RG") == 0) {
            size_t t = text.find("\tSM:", line);
            if (t != std::string::npos && t < eol) {
                t += 4;
                size_t e = t;
                while (e < eol && text[e] != '\t' && text[e] != '\r' && text[e] != '\0') ++e;
                const std::string one = text.substr(t, e - t);
                if (sm.empty()) sm = one;
                else if (sm != one) *several = true;
            }
        }
        line = eol + 1;
    }
    return sm.empty() ? std::string("DefaultSampleName") : sm;
}

// The header's @RG lines in header order: the tab-separated fields ID:, SM:, LB: and PU:, wherever they stand in the line.
void read_groups_of(const std::string& path, const std::string& text, std::vector<ReadGroup>* out)
{
    std::map<std::string, size_t> seen;
    size_t line = 0;
    while (line < text.size()) {
        size_t eol = text.find('\n', line);
        if (eol == std::string::npos) eol = text.size();
        size_t end = eol;
        while (end > line && (text[end - 1] == '\r' || text[end - 1] == '\0')) --end;
        if (end - line >= 3 && text.compare(line, 3, "@RG") == 0 && (end - line == 3 || text[line + 3] == '\t')) {
            ReadGroup g;
            bool has_id = false;
            size_t f = line + 3;
            while (f < end) {
                ++f;                                             // the tab
                size_t e = text.find('\t', f);
                if (e == std::string::npos || e > end) e = end;
                if (e - f >= 3 && text[f + 2] == ':') {
                    const std::string val = text.substr(f + 3, e - f - 3);
                    if (text.compare(f, 2, "ID") == 0) { g.id = val; has_id = true; }
                    else if (text.compare(f, 2, "SM") == 0) g.sm = val;
                    else if (text.compare(f, 2, "LB") == 0) g.lb = val;
                    else if (text.compare(f, 2, "PU") == 0) g.pu = val;
                }
                f = e;
            }
            const std::string nth = "@RG line " + std::to_string(out->size() + 1) + " of the header";
            if (!has_id) throw Fail{kErrInvalid, path + ": " + nth + " has no ID: field"};
            if (seen.count(g.id))
                throw Fail{kErrInvalid, path + ": " + nth + " repeats the ID \"" + g.id + "\" of line " + std::to_string(seen[g.id] + 1)};
            if (out->size() >= kMaxGroups)
                throw Fail{kErrInvalid, path + ": more than " + std::to_string(kMaxGroups) + " @RG lines in the header"};
            seen[g.id] = out->size();
            out->push_back(std::move(g));
        }
        line = eol + 1;
    }
}

// The group of one record: its auxiliary fields [p, end) walked once (SAMv1 4.2.4), every field's length checked against
// the record's end.  The first RG field of type Z names the group; an RG of another type, or an ID the header lacks, none.
uint16_t group_of_record(const uint8_t* p, const uint8_t* end, const std::map<std::string, uint16_t>& group_of,
                         const std::string& path, uint64_t voff)
{
    auto fail = [&](const std::string& what) -> Fail {
        return Fail{kErrInvalid, path + ": record at virtual offset " + std::to_string(voff) + ": " + what};
    };
    auto width = [](uint8_t t) -> size_t {
        switch (t) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
        }
    };
    uint16_t group = kNoGroup;
    bool found = false;
    while (p < end) {
        const size_t left = (size_t)(end - p);
        if (left < 3) throw fail(std::to_string(left) + " stray byte(s) behind its last auxiliary field");
        const uint8_t t0 = p[0], t1 = p[1], type = p[2];
        const std::string tag{(char)t0, (char)t1};
        p += 3;
        const size_t avail = (size_t)(end - p);
        size_t len = 0;
        if (type == 'Z' || type == 'H') {
            const void* nul = avail ? std::memchr(p, 0, avail) : nullptr;
            if (!nul) throw fail("auxiliary field " + tag + " of type " + std::string(1, (char)type) + " has no terminator before the record's end");
            len = (size_t)((const uint8_t*)nul - p) + 1;
            if (!found && t0 == 'R' && t1 == 'G') {
                found = true;
                if (type == 'Z') {
                    auto it = group_of.find(std::string((const char*)p, len - 1));
                    if (it != group_of.end()) group = it->second;
                }
            }
        } else if (type == 'B') {
            if (avail < 5) throw fail("auxiliary array " + tag + " passes the end of the record");
            const size_t w = width(p[0]);
            if (w == 0 || p[0] == 'A') throw fail("auxiliary array " + tag + " has the unknown subtype byte " + std::to_string((int)p[0]));
            const uint64_t count = le32(p + 1);
            if (count > (avail - 5) / w) throw fail("auxiliary array " + tag + " of " + std::to_string(count) + " elements passes the end of the record");
            len = 5 + (size_t)count * w;
        } else {
            len = width(type);
            if (len == 0) throw fail("auxiliary field " + tag + " has the unknown type byte " + std::to_string((int)type));
            if (len > avail) throw fail("auxiliary field " + tag + " passes the end of the record");
            if (t0 == 'R' && t1 == 'G') found = true;           // an RG that is no string: the record has no group
        }
        p += len;
    }
    return group;
}

struct Header {
    std::vector<std::string> name;
    std::vector<int64_t> len;
    std::string text;
};

void read_header(const File& f, Header* h, int64_t* nblocks)
{
    std::vector<uint8_t> buf;
    Stream s{f, 0, &buf, nullptr, nblocks};
    size_t o = 0;
    auto need = [&](uint64_t n) {
        while (buf.size() - o < n)
            if (!s.more()) throw Fail{kErrIo, f.path + ": the BAM header is truncated"};
    };
    need(4);
    if (std::memcmp(buf.data(), "BAM\1", 4) != 0) throw Fail{kErrInvalid, f.path + ": not a BAM file (bad magic after inflating the first block)"};
    o = 4;
    need(4);
    const int32_t l_text = (int32_t)le32(buf.data() + o);
    o += 4;
    if (l_text < 0) throw Fail{kErrInvalid, f.path + ": negative l_text in the BAM header"};
    need((uint64_t)l_text);
    h->text.assign((const char*)buf.data() + o, (size_t)l_text);
    o += (size_t)l_text;
    need(4);
    const int32_t n_ref = (int32_t)le32(buf.data() + o);
    o += 4;
    if (n_ref < 0) throw Fail{kErrInvalid, f.path + ": negative n_ref in the BAM header"};
    for (int32_t r = 0; r < n_ref; ++r) {
        need(4);
        const int32_t l_name = (int32_t)le32(buf.data() + o);
        o += 4;
        if (l_name < 1 || l_name > 65536) throw Fail{kErrInvalid, f.path + ": reference name of length " + std::to_string(l_name) + " in the BAM header"};
        need((uint64_t)l_name + 4);
        size_t n = (size_t)l_name;
        while (n > 0 && buf[o + n - 1] == 0) --n;
        h->name.emplace_back((const char*)buf.data() + o, n);
        o += (size_t)l_name;
        h->len.push_back((int32_t)le32(buf.data() + o));
        o += 4;
    }
}

// ---- the index ----
struct IdxChunk {
    uint64_t beg, end;
};
struct RefIndex {
    std::map<uint32_t, std::vector<IdxChunk>> bins;
    std::vector<uint64_t> linear;
};

struct Cursor {
    const std::vector<uint8_t>& b;
    size_t o = 0;
    const std::string& path;
    void need(uint64_t n) const
    {
        if (n > b.size() - o) throw Fail{kErrIo, path + ": the index is truncated"};
    }
    uint32_t u32() { need(4); const uint32_t v = le32(b.data() + o); o += 4; return v; }
    uint64_t u64() { need(8); const uint64_t v = le64(b.data() + o); o += 8; return v; }
    void skip(uint64_t n) { need(n); o += (size_t)n; }
};

// keeps the bins and windows of the sequences in `want` (by tid), skips the others
void read_bai(const std::string& path, size_t n_ref_bam, const std::vector<char>& want, std::vector<RefIndex>* idx)
{
    File f;
    if (!f.open(path)) throw Fail{kErrIo, "fail to load index for " + path};
    if (f.size > (4ull << 30)) throw Fail{kErrInvalid, path + ": index larger than 4 GiB"};
    std::vector<uint8_t> b((size_t)f.size);
    if (!b.empty()) f.read(0, b.size(), b.data());
    Cursor c{b, 0, path};
    c.need(8);
    if (std::memcmp(b.data(), "BAI\1", 4) != 0) throw Fail{kErrInvalid, path + ": not a BAI index (bad magic; .csi is not supported)"};
    c.o = 4;
    const int32_t n_ref = (int32_t)c.u32();
    if (n_ref < 0 || (size_t)n_ref != n_ref_bam)
        throw Fail{kErrInvalid, path + ": the index has " + std::to_string(n_ref) + " reference sequences, the BAM header " + std::to_string(n_ref_bam)};
    idx->assign((size_t)n_ref, RefIndex());
    for (int32_t r = 0; r < n_ref; ++r) {
        const int32_t n_bin = (int32_t)c.u32();
        if (n_bin < 0) throw Fail{kErrInvalid, path + ": negative bin count"};
        for (int32_t i = 0; i < n_bin; ++i) {
            const uint32_t bin = c.u32();
            const int32_t n_chunk = (int32_t)c.u32();
            if (n_chunk < 0) throw Fail{kErrInvalid, path + ": negative chunk count"};
            c.need(16ull * (uint64_t)n_chunk);
            if (!want[(size_t)r] || bin >= (uint32_t)kBinPseudo) {
                c.skip(16ull * (uint64_t)n_chunk);
                continue;
            }
            std::vector<IdxChunk>& v = (*idx)[(size_t)r].bins[bin];
            for (int32_t k = 0; k < n_chunk; ++k) {
                IdxChunk ch;
                ch.beg = c.u64();
                ch.end = c.u64();
                v.push_back(ch);
            }
        }
        const int32_t n_intv = (int32_t)c.u32();
        if (n_intv < 0) throw Fail{kErrInvalid, path + ": negative interval count"};
        c.need(8ull * (uint64_t)n_intv);
        if (!want[(size_t)r]) {
            c.skip(8ull * (uint64_t)n_intv);
            continue;
        }
        std::vector<uint64_t>& lin = (*idx)[(size_t)r].linear;
        lin.resize((size_t)n_intv);
        for (int32_t k = 0; k < n_intv; ++k) lin[(size_t)k] = c.u64();
    }
}

// The merged chunks that can hold a record over one of `pos` (sorted, 1-based): the bins of [p - 1, p), filtered by the
// linear index's minimum offset, sorted and merged where they touch the same block.
std::vector<IdxChunk> plan(const File& bam, const RefIndex& ri, const std::vector<int32_t>& pos)
{
    std::map<uint32_t, uint64_t> bin_min;           // bin -> smallest minimum offset among the markers that look into it
    for (int32_t p1 : pos) {
        if (p1 < 1 || p1 > (1 << 29)) continue;      // outside what a .bai can index: no record can be found there
        const uint32_t b = (uint32_t)(p1 - 1);
        uint64_t min_off = 0;
        if (!ri.linear.empty()) min_off = ri.linear[std::min<size_t>(b >> 14, ri.linear.size() - 1)];
        const uint32_t bins[6] = {0, 1 + (b >> 26), 9 + (b >> 23), 73 + (b >> 20), 585 + (b >> 17), 4681 + (b >> 14)};
        for (uint32_t bin : bins) {
            if (ri.bins.find(bin) == ri.bins.end()) continue;
            auto it = bin_min.find(bin);
            if (it == bin_min.end()) bin_min[bin] = min_off;
            else if (min_off < it->second) it->second = min_off;
        }
    }
    std::vector<IdxChunk> all;
    for (const auto& bm : bin_min)
        for (const IdxChunk& ch : ri.bins.at(bm.first)) {
            if (ch.end <= bm.second) continue;
            if (ch.beg >= ch.end) continue;                      // empty
            // (a chunk that only ENDS behind the file is found out while its blocks are listed: the file is truncated)
            if ((ch.beg >> 16) >= bam.size)
                throw Fail{kErrInvalid, bam.path + ": the index names a chunk beyond the end of the file (offset " + std::to_string(ch.beg >> 16) + ")"};
            all.push_back(ch);
        }
    std::sort(all.begin(), all.end(), [](const IdxChunk& a, const IdxChunk& b) { return a.beg < b.beg || (a.beg == b.beg && a.end < b.end); });
    std::vector<IdxChunk> merged;
    for (const IdxChunk& ch : all) {
        if (!merged.empty() && (ch.beg >> 16) <= (merged.back().end >> 16)) merged.back().end = std::max(merged.back().end, ch.end);
        else merged.push_back(ch);
    }
    return merged;
}

struct BlockRef {
    uint32_t chunk;
    uint64_t file_off;
    BlockHead head;
    uint32_t isize;
    uint64_t out_off;
    uint64_t raw_off;      // within the chunk's compressed bytes
};

struct Work {
    std::vector<uint8_t> raw;                                   // compressed bytes of the chunk's blocks
    std::vector<std::pair<uint64_t, uint64_t>> blocks;          // (file offset, offset in Chunk::bytes)
    uint64_t next_off = 0;                                      // file offset behind the chunk's last planned block
};

// the blocks from beg's to end's (inclusive where end points into one), their sizes from the headers and trailers
void list_blocks(const File& f, uint32_t ci, const Chunk& ch, Work* w, std::vector<BlockRef>* refs)
{
    const uint64_t c0 = ch.beg >> 16, c1 = ch.end >> 16;
    const uint64_t span_end = std::min<uint64_t>(f.size, c1 + 65536 + 18 + 65536);
    w->raw.resize((size_t)(span_end - c0));
    f.read(c0, w->raw.size(), w->raw.data());
    uint64_t off = c0, out = 0;
    while (off <= c1 && off < f.size) {
        if ((off == c1) && (ch.end & 0xffff) == 0 && off != c0) break;      // the chunk ends exactly at this block's start
        const uint64_t avail_buf = span_end - off;
        BlockHead h = parse_block_head(f, off, w->raw.data() + (off - c0), std::min<uint64_t>(avail_buf, f.size - off));
        const uint32_t isize = le32(w->raw.data() + (off - c0) + h.size - 4);
        if (isize > 65536) throw Fail{kErrInvalid, f.path + ": BGZF block at " + std::to_string(off) + ": ISIZE " + std::to_string(isize) + " exceeds 65536"};
        refs->push_back(BlockRef{ci, off, h, isize, out, off - c0});
        w->blocks.emplace_back(off, out);
        out += isize;
        off += h.size;
    }
    if (w->blocks.empty()) throw Fail{kErrInvalid, f.path + ": a chunk of the index holds no block"};
    w->next_off = off;
    if (out > 0xfff00000ull) throw Fail{kErrInvalid, f.path + ": a chunk of more than 4 GiB"};
}

inline bool consumes_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// Walks the record chain of one chunk whose planned blocks are inflated; inflates further blocks where its last record
// straddles.  Keeps the records on the chunk's sequence that can reach one of `pos`.
// group_of (may be null): the header's group IDs; then every kept record's auxiliary fields are walked for its group.
void walk_chunk(const File& f, Chunk* ch, Work* w, const std::vector<int32_t>& pos, int32_t n_ref, Stats* st,
                const std::map<std::string, uint16_t>* group_of)
{
    std::vector<uint8_t>& b = ch->bytes;
    Stream s{f, w->next_off, &b, &w->blocks, &st->blocks};
    const uint64_t u0 = ch->beg & 0xffff;
    if (u0 > b.size() || (w->blocks.size() > 1 && u0 > w->blocks[1].second))
        throw Fail{kErrInvalid, f.path + ": the index points past the end of the block at " + std::to_string(ch->beg >> 16)};
    uint64_t o = u0;
    size_t bi = 0;                                    // block that holds offset o
    auto need = [&](uint64_t n) -> bool {             // false: the file ends before offset o + n
        while (b.size() - o < n) {
            if (b.size() > 0xfff00000ull) throw Fail{kErrInvalid, f.path + ": a chunk of more than 4 GiB"};
            if (!s.more()) return false;
        }
        return true;
    };
    const int32_t last_marker = pos.empty() ? 0 : pos.back();
    for (;;) {
        if (o == b.size() && !need(1)) break;                                   // clean end of the file
        while (bi + 1 < w->blocks.size() && w->blocks[bi + 1].second <= o) ++bi;
        const uint64_t voff = (w->blocks[bi].first << 16) | (o - w->blocks[bi].second);
        if (voff >= ch->end) break;
        if (!need(4)) throw Fail{kErrIo, f.path + ": truncated inside a record's block_size (virtual offset " + std::to_string(voff) + ")"};
        const int32_t block_size = (int32_t)le32(b.data() + o);
        if (block_size < 32 || (uint32_t)block_size > kMaxRecord)
            throw Fail{kErrInvalid, f.path + ": record at virtual offset " + std::to_string(voff) + " has block_size " + std::to_string(block_size)};
        if (!need(4ull + (uint64_t)block_size))
            throw Fail{kErrIo, f.path + ": the record at virtual offset " + std::to_string(voff) + " runs past the end of the file"};
        const uint8_t* r = b.data() + o + 4;
        RecordDesc d;
        d.tid = (int32_t)le32(r);
        d.pos = (int32_t)le32(r + 4);
        d.l_read_name = r[8];
        d.mapq = r[9];
        d.n_cigar = le16(r + 12);
        d.flag = le16(r + 14);
        d.l_seq = (int32_t)le32(r + 16);
        d.mate_same = (int32_t)le32(r + 20) == d.tid ? 1 : 0;
        d.mpos = (int32_t)le32(r + 24);
        d.order = 0;
        d.data = (uint32_t)(o + 36);
        const std::string at = f.path + ": record at virtual offset " + std::to_string(voff) + ": ";
        if (d.l_read_name < 1) throw Fail{kErrInvalid, at + "l_read_name is 0"};
        if (d.l_seq < 0) throw Fail{kErrInvalid, at + "negative l_seq"};
        if ((uint64_t)d.l_read_name + 4ull * d.n_cigar + ((uint64_t)d.l_seq + 1) / 2 + (uint64_t)d.l_seq > (uint64_t)block_size - 32)
            throw Fail{kErrInvalid, at + "its name, CIGAR, bases and qualities exceed block_size"};
        if (d.tid < -1 || d.tid >= n_ref) throw Fail{kErrInvalid, at + "reference id " + std::to_string(d.tid) + " is not in the header"};
        ++st->records_seen;
        o += 4ull + (uint64_t)block_size;
        if (d.tid != ch->tid) {
            if (d.tid < 0 || d.tid > ch->tid) break;          // sorted input: the sequence is over
            continue;
        }
        if (d.pos < 0) continue;
        if (d.pos >= last_marker) break;                      // (1-based markers: pos + 1 > the last one) sorted: nothing more here
        const uint8_t* cg = b.data() + d.data + d.l_read_name;
        int64_t rlen = 0;
        for (uint32_t k = 0; k < d.n_cigar; ++k) {
            const uint32_t c = le32(cg + 4 * k);
            if (consumes_ref(c & 15)) rlen += c >> 4;
        }
        // the long-CIGAR convention (SAMv1 4.2.2): "<l_seq>S<reference length>N" stands in for a CIGAR of more than
        // 65 535 operations, which is in the CG tag
        if (d.n_cigar == 2 && (le32(cg) & 15) == 4 && (int64_t)(le32(cg) >> 4) == d.l_seq && (le32(cg + 4) & 15) == 3) {
            ++st->long_cigar_skipped;
            continue;
        }
        if (rlen < 1) rlen = 1;
        auto it = std::lower_bound(pos.begin(), pos.end(), d.pos + 1);
        if (it == pos.end() || (int64_t)*it > (int64_t)d.pos + rlen) continue;
        ch->recs.push_back(d);
        ch->voffset.push_back(voff);
        if (group_of) {
            // from the end of the qualities to the end of the record's block (o is behind it; the check above keeps the
            // start inside)
            const uint64_t var = (uint64_t)d.l_read_name + 4ull * d.n_cigar + ((uint64_t)d.l_seq + 1) / 2 + (uint64_t)d.l_seq;
            const uint16_t g = group_of_record(b.data() + d.data + var, b.data() + o, *group_of, f.path, voff);
            ch->group.push_back(g);
            if (g == kNoGroup) ++st->records_unassigned;
        }
    }
}

// fn(i) for i in [0, n) on `threads` threads; the first Fail wins
template <class F> void parallel(size_t n, int threads, F fn)
{
    std::atomic<size_t> next{0};
    std::mutex mu;
    bool failed = false;
    Fail first{0, ""};
    auto body = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) return;
            try {
                fn(i);
            } catch (const Fail& e) {
                std::lock_guard<std::mutex> g(mu);
                if (!failed) { failed = true; first = e; }
                next.store(n);
                return;
            } catch (const std::exception& e) {
                std::lock_guard<std::mutex> g(mu);
                if (!failed) { failed = true; first = Fail{kErrNoMem, e.what()}; }
                next.store(n);
                return;
            }
        }
    };
    const int t = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n));
    std::vector<std::thread> pool;
    for (int k = 1; k < t; ++k) pool.emplace_back(body);
    body();
    for (std::thread& th : pool) th.join();
    if (failed) throw first;
}

void scan_impl(const std::string& bam_path, const std::vector<SeqMarkers>& markers, int threads, Scan* out, bool want_groups,
               BlockInflater* inflater)
{
    threads = std::max(1, std::min(threads, 16));
    const double t0 = now_s();
    File bam;
    if (!bam.open(bam_path))
        throw Fail{kErrIo, "cannot open " + bam_path + " (built-in BAM reader; this build has no htslib: no CRAM, no BAQ, no mapQ cap)"};
    uint8_t magic[4] = {0, 0, 0, 0};
    if (bam.size >= 4) bam.read(0, 4, magic);
    if (std::memcmp(magic, "CRAM", 4) == 0)
        throw Fail{kErrInvalid, bam_path + " is a CRAM file: the built-in reader reads BAM only (this build has no htslib); convert it with `samtools view -b`"};
    Header hd;
    read_header(bam, &hd, &out->stats.blocks);
    bool several = false;
    out->sample = sample_of(hd.text, &several);
    if (several) throw Fail{kErrInvalid, "This BAM or CRAM file contains more than 1 sample, please demultiplex or separate first!"};
    out->ref_name = hd.name;
    out->ref_len = hd.len;
    std::map<std::string, uint16_t> group_of;
    if (want_groups) {
        read_groups_of(bam_path, hd.text, &out->groups);
        for (size_t g = 0; g < out->groups.size(); ++g) group_of[out->groups[g].id] = (uint16_t)g;
    }
    const int32_t n_ref = (int32_t)hd.name.size();
    std::map<std::string, int32_t> tid_of;
    for (int32_t t = n_ref - 1; t >= 0; --t) tid_of[hd.name[(size_t)t]] = t;
    std::vector<char> want((size_t)n_ref, 0);
    std::vector<const std::vector<int32_t>*> pos_of((size_t)n_ref, nullptr);
    out->tid_of_seq.assign(markers.size(), -1);
    for (size_t m = 0; m < markers.size(); ++m) {
        auto it = tid_of.find(markers[m].name);
        if (it == tid_of.end() || markers[m].pos.empty() || pos_of[(size_t)it->second]) continue;
        out->tid_of_seq[m] = it->second;
        want[(size_t)it->second] = 1;
        pos_of[(size_t)it->second] = &markers[m].pos;
    }
    // the index: <bam>.bai, else <stem>.bai
    std::string bai = bam_path + ".bai";
    {
        File probe;
        if (!probe.open(bai)) {
            std::string stem = bam_path;
            if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".bam") == 0) stem.resize(stem.size() - 4);
            bai = stem + ".bai";
            File probe2;
            if (!probe2.open(bai)) throw Fail{kErrIo, "fail to load index for " + bam_path};
        }
    }
    std::vector<RefIndex> idx;
    read_bai(bai, (size_t)n_ref, want, &idx);
    for (int32_t t = 0; t < n_ref; ++t) {
        if (!want[(size_t)t]) continue;
        for (const IdxChunk& c : plan(bam, idx[(size_t)t], *pos_of[(size_t)t])) {
            Chunk ch;
            ch.tid = t;
            ch.beg = c.beg;
            ch.end = c.end;
            out->chunks.push_back(std::move(ch));
        }
    }
    idx.clear();
    out->stats.chunks = (int64_t)out->chunks.size();
    const double t1 = now_s();
    out->stats.seconds_index = t1 - t0;
    // inflate: list every chunk's blocks, then every block on its own
    const size_t nc = out->chunks.size();
    std::vector<Work> work(nc);
    std::vector<std::vector<BlockRef>> refs_of(nc);
    parallel(nc, threads, [&](size_t i) { list_blocks(bam, (uint32_t)i, out->chunks[i], &work[i], &refs_of[i]); });
    std::vector<BlockRef> refs;
    for (size_t i = 0; i < nc; ++i) {
        uint64_t total = 0;
        for (const BlockRef& r : refs_of[i]) total += r.isize;
        out->chunks[i].bytes.resize((size_t)total);
        refs.insert(refs.end(), refs_of[i].begin(), refs_of[i].end());
    }
    if (!inflater) {
        parallel(refs.size(), threads, [&](size_t k) {
            const BlockRef& r = refs[k];
            inflate_block(bam, r.file_off, work[r.chunk].raw.data() + r.raw_off, r.head, out->chunks[r.chunk].bytes.data() + r.out_off, r.isize);
        });
    } else {
        // every planned block to the inflater; then, on the pool, the CRC32 of what it inflated, and zlib for what it refused or
        // got wrong
        const double ti = now_s();
        std::vector<InflateItem> items(refs.size());
        std::vector<int32_t> status(refs.size(), -1);
        for (size_t k = 0; k < refs.size(); ++k) {
            const BlockRef& r = refs[k];
            items[k] = InflateItem{work[r.chunk].raw.data() + r.raw_off + r.head.data_off, r.head.data_len,
                                   out->chunks[r.chunk].bytes.data() + r.out_off, r.isize};
        }
        std::string ierr;
        if (const int rc = inflater->run(items.data(), items.size(), status.data(), &ierr)) throw Fail{rc, ierr};
        const double tc = now_s();
        std::atomic<int64_t> refused{0};
        parallel(refs.size(), threads, [&](size_t k) {
            const BlockRef& r = refs[k];
            const uint8_t* p = work[r.chunk].raw.data() + r.raw_off;
            uint8_t* dst = out->chunks[r.chunk].bytes.data() + r.out_off;
            if (status[k] != 0) {
                refused.fetch_add(1);
                inflate_block(bam, r.file_off, p, r.head, dst, r.isize);
                return;
            }
            // bytes that miss the CRC32: zlib inflates the block again and ITS verdict stands -- a stream zlib refuses ends in
            // zlib's message although the inflater made something of it, and a wrong CRC32 field in inflate_block's own
            if (!crc_matches(p, r.head, dst, r.isize)) {
                refused.fetch_add(1);
                inflate_block(bam, r.file_off, p, r.head, dst, r.isize);
            }
        });
        out->stats.inflater_blocks = (int64_t)refs.size();
        out->stats.inflater_refused = refused.load();
        out->stats.seconds_inflater = tc - ti;
        out->stats.seconds_crc = now_s() - tc;
    }
    out->stats.blocks += (int64_t)refs.size();
    std::vector<Stats> st(nc);
    parallel(nc, threads, [&](size_t i) {
        work[i].raw.clear();
        work[i].raw.shrink_to_fit();
        walk_chunk(bam, &out->chunks[i], &work[i], *pos_of[(size_t)out->chunks[i].tid], n_ref, &st[i], want_groups ? &group_of : nullptr);
    });
    uint64_t order = 0;
    for (size_t i = 0; i < nc; ++i) {
        out->stats.blocks += st[i].blocks;
        out->stats.records_seen += st[i].records_seen;
        out->stats.long_cigar_skipped += st[i].long_cigar_skipped;
        out->stats.records_unassigned += st[i].records_unassigned;
        out->stats.bytes_inflated += (int64_t)out->chunks[i].bytes.size();
        out->stats.records_kept += (int64_t)out->chunks[i].recs.size();
        for (RecordDesc& d : out->chunks[i].recs) d.order = (uint32_t)order++;
        if (order > 0xffffffffull) throw Fail{kErrInvalid, bam_path + ": more than 2^32 records over the panel's markers"};
    }
    out->stats.seconds_inflate = now_s() - t1;
}

}  // namespace

int scan(const std::string& bam_path, const std::vector<SeqMarkers>& markers, int threads, Scan* out, std::string* err,
         bool want_groups, BlockInflater* inflater)
{
    try {
        scan_impl(bam_path, markers, threads, out, want_groups, inflater);
        return kOk;
    } catch (const Fail& e) {
        if (err) *err = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        if (err) *err = bam_path + ": out of memory while reading";
        return kErrNoMem;
    } catch (const std::exception& e) {
        if (err) *err = bam_path + ": " + e.what();
        return kErrInvalid;
    }
}

int list_bgzf_blocks(const uint8_t* bytes, uint64_t n, const std::string& name, std::vector<BlockSpan>* out, std::string* err)
{
    try {
        File f;                                   // (never opened: it carries the name and the size for the messages and checks)
        f.path = name;
        f.size = n;
        out->clear();
        for (uint64_t off = 0; off < n;) {
            const BlockHead h = parse_block_head(f, off, bytes + off, n - off);
            const uint32_t isize = le32(bytes + off + h.size - 4);
            if (isize > 65536) throw Fail{kErrInvalid, name + ": BGZF block at " + std::to_string(off) + ": ISIZE " + std::to_string(isize) + " exceeds 65536"};
            out->push_back(BlockSpan{off + h.data_off, h.data_len, isize, le32(bytes + off + h.size - 8)});
            off += h.size;
        }
        return kOk;
    } catch (const Fail& e) {
        if (err) *err = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        if (err) *err = name + ": out of memory while listing its blocks";
        return kErrNoMem;
    }
}

}  // namespace bamio
}  // namespace vb2
