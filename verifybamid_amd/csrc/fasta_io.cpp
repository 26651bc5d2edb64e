// fasta_io.cpp -- see fasta_io.h.
#include "fasta_io.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace vb2 {
namespace fasta {

namespace {

struct File {
    FILE* f = nullptr;
    ~File() { if (f) std::fclose(f); }
};

bool file_size(FILE* f, int64_t* n)
{
    if (fseeko(f, 0, SEEK_END) != 0) return false;
    const off_t e = ftello(f);
    if (e < 0) return false;
    *n = (int64_t)e;
    return fseeko(f, 0, SEEK_SET) == 0;
}

bool parse_i64(const std::string& s, int64_t* v)
{
    if (s.empty() || s.size() > 18) return false;
    int64_t x = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    *v = x;
    return true;
}

}  // namespace

int Index::find(const std::string& name) const
{
    for (size_t i = 0; i < seqs.size(); ++i)
        if (seqs[i].name == name) return (int)i;
    return -1;
}

namespace {
struct Nt16Table {
    uint8_t code[256];
    Nt16Table()
    {
        static const char kCodes[] = "=ACMGRSVTWYHKDBN";
        for (int c = 0; c < 256; ++c) {
            int u = c >= 'a' && c <= 'z' ? c - 32 : c;
            code[c] = 15;
            for (int i = 0; i < 16; ++i)
                if ((unsigned char)kCodes[i] == u) code[c] = (uint8_t)i;
        }
    }
};
}  // namespace

uint8_t nt16_of(unsigned char c)
{
    static const Nt16Table t;
    return t.code[c];
}

int open_index(const std::string& fasta_path, Index* out, std::string* err)
{
    out->path = fasta_path;
    out->seqs.clear();
    File fa;
    fa.f = std::fopen(fasta_path.c_str(), "rb");
    if (!fa.f) {
        *err = "--Reference: cannot open " + fasta_path + ": " + std::strerror(errno);
        return kErrIo;
    }
    if (!file_size(fa.f, &out->file_size)) {
        *err = "--Reference: cannot seek in " + fasta_path;
        return kErrIo;
    }
    unsigned char magic[2] = {0, 0};
    if (std::fread(magic, 1, 2, fa.f) == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
        *err = "--Reference: " + fasta_path + " is compressed (gzip or bgzip); --ApplyBAQ reads a plain FASTA with its .fai";
        return kErrInvalid;
    }
    const std::string fai_path = fasta_path + ".fai";
    File fi;
    fi.f = std::fopen(fai_path.c_str(), "rb");
    if (!fi.f) {
        *err = "--Reference: cannot open the index " + fai_path + " (" + std::strerror(errno) + "); build it with `samtools faidx " +
               fasta_path + "`";
        return kErrIo;
    }
    std::string text;
    {
        char buf[1 << 16];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), fi.f)) > 0) text.append(buf, n);
    }
    size_t at = 0;
    int line_no = 0;
    while (at < text.size()) {
        size_t eol = text.find('\n', at);
        const bool terminated = eol != std::string::npos;
        if (!terminated) eol = text.size();
        std::string line = text.substr(at, eol - at);
        at = eol + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const std::string where = fai_path + " line " + std::to_string(line_no) + ": ";
        std::vector<std::string> col;
        size_t p = 0;
        for (;;) {
            const size_t t = line.find('\t', p);
            col.push_back(line.substr(p, t == std::string::npos ? std::string::npos : t - p));
            if (t == std::string::npos) break;
            p = t + 1;
        }
        if (col.size() < 5 || !terminated) {
            *err = where + (col.size() < 5 ? "fewer than five columns" : "the line does not end") + " (a truncated index?)";
            return kErrInvalid;
        }
        Sequence s;
        s.name = col[0];
        if (s.name.empty() || !parse_i64(col[1], &s.length) || !parse_i64(col[2], &s.offset) || !parse_i64(col[3], &s.line_bases) ||
            !parse_i64(col[4], &s.line_width)) {
            *err = where + "a column is not a number";
            return kErrInvalid;
        }
        if (s.line_bases < 1 || s.line_width < s.line_bases) {
            if (s.length > 0) {
                *err = where + "line bases " + col[3] + " and line width " + col[4] + " cannot be";
                return kErrInvalid;
            }
            s.line_bases = s.line_width = 1;
        }
        // the last base's byte must lie inside the file
        if (s.length > 0) {
            const int64_t last = s.length - 1;
            const int64_t lines = last / s.line_bases;
            if (s.offset > out->file_size || lines > (out->file_size - s.offset) / s.line_width ||
                s.offset + lines * s.line_width + last % s.line_bases >= out->file_size) {
                *err = where + "sequence " + s.name + " (offset " + col[2] + ", length " + col[1] + ") passes the end of " + fasta_path +
                       " (" + std::to_string(out->file_size) + " bytes)";
                return kErrInvalid;
            }
        } else if (s.offset > out->file_size) {
            *err = where + "offset " + col[2] + " passes the end of " + fasta_path;
            return kErrInvalid;
        }
        out->seqs.push_back(std::move(s));
    }
    return kOk;
}

int fetch_nt16(const Index& idx, int seq, int64_t beg, int64_t end, uint8_t* out, std::string* err)
{
    Reader r(idx);
    return r.fetch_nt16(seq, beg, end, out, err);
}

Reader::~Reader()
{
    if (file_) std::fclose(static_cast<FILE*>(file_));
}

int Reader::fetch_nt16(int seq, int64_t beg, int64_t end, uint8_t* out, std::string* err)
{
    const Index& idx = idx_;
    if (seq < 0 || (size_t)seq >= idx.seqs.size()) {
        *err = "--Reference: internal error: sequence number out of range";
        return kErrInvalid;
    }
    const Sequence& s = idx.seqs[(size_t)seq];
    if (beg < 0 || end < beg || end > s.length) {
        *err = "--Reference: internal error: span outside sequence " + s.name;
        return kErrInvalid;
    }
    if (beg == end) return kOk;
    if (!file_) {
        file_ = std::fopen(idx.path.c_str(), "rb");
        if (!file_) {
            *err = "--Reference: cannot open " + idx.path + ": " + std::strerror(errno);
            return kErrIo;
        }
    }
    FILE* const f = static_cast<FILE*>(file_);
    // bytes [b0, b1] hold the span: open_index has checked that the sequence's last byte lies inside the file
    const int64_t b0 = s.offset + beg / s.line_bases * s.line_width + beg % s.line_bases;
    const int64_t b1 = s.offset + (end - 1) / s.line_bases * s.line_width + (end - 1) % s.line_bases;
    raw_.resize((size_t)(b1 - b0 + 1));
    if (fseeko(f, (off_t)b0, SEEK_SET) != 0 || std::fread(raw_.data(), 1, raw_.size(), f) != raw_.size()) {
        *err = "--Reference: short read from " + idx.path + " (sequence " + s.name + ")";
        return kErrIo;
    }
    int64_t col = beg % s.line_bases, n = 0;
    for (size_t i = 0; i < raw_.size() && n < end - beg;) {
        out[n++] = nt16_of(raw_[i]);
        if (++col == s.line_bases) {
            col = 0;
            i += (size_t)(s.line_width - s.line_bases) + 1;
        } else {
            ++i;
        }
    }
    if (n != end - beg) {
        *err = "--Reference: internal error: span of sequence " + s.name + " came out short";
        return kErrInvalid;
    }
    return kOk;
}

}  // namespace fasta
}  // namespace vb2
