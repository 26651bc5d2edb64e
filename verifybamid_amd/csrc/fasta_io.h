// fasta_io.h -- the reference FASTA of --ApplyBAQ on the host: a plain FASTA with its .fai index.
// Plain C++17, no HIP header and nothing of context.h: tests/baq_check_main.cpp links the unit alone under the host
// sanitizers.  Every offset and length of the index is checked against the file's size before a byte of it is read, so a
// mutilated index ends in a code with a message, never in a read outside the file.
#ifndef VB2_FASTA_IO_H_
#define VB2_FASTA_IO_H_

#include <cstdint>
#include <string>
#include <vector>

namespace vb2 {
namespace fasta {

constexpr int kOk = 0, kErrInvalid = -1, kErrIo = -4;      // the C-ABI's codes, as bam_io.h restates them

struct Sequence {
    std::string name;
    int64_t length = 0, offset = 0, line_bases = 0, line_width = 0;
};

struct Index {
    std::string path;
    int64_t file_size = 0;
    std::vector<Sequence> seqs;
    int find(const std::string& name) const;      // -1: the FASTA lacks it
};

// Reads <fasta>.fai (five columns; further ones are ignored).  A missing index is kErrIo with a message that names
// `samtools faidx`; a bgzipped FASTA is refused (kErrInvalid).
int open_index(const std::string& fasta_path, Index* out, std::string* err);

// htslib's seq_nt16_table: the 4-bit code of a base character (either case), 15 for everything else
uint8_t nt16_of(unsigned char c);

// The bases [beg, end) of sequence `seq` as nt16 codes, one per byte; 0 <= beg <= end <= length.
int fetch_nt16(const Index& idx, int seq, int64_t beg, int64_t end, uint8_t* out, std::string* err);

// Many spans of one file: the FASTA opened once.
class Reader {
public:
    explicit Reader(const Index& idx) : idx_(idx) {}
    ~Reader();
    Reader(const Reader&) = delete;
    Reader& operator=(const Reader&) = delete;
    int fetch_nt16(int seq, int64_t beg, int64_t end, uint8_t* out, std::string* err);

private:
    const Index& idx_;
    void* file_ = nullptr;      // FILE*
    std::vector<unsigned char> raw_;
};

}  // namespace fasta
}  // namespace vb2

#endif
