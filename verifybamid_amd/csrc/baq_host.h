// baq_host.h -- the host side of --ApplyBAQ: the tables baq_core.h's device code cannot build (libm),
// the reference spans the fetched records can touch, a record's task for the device stage, the end of the cap, and a
// SEQUENTIAL driver of baq_core.h over one record.  The driver serves vb2_baq_records(where = 0) and
// tests/baq_check_main.cpp; it is NOT a CPU fallback of the product (a load without a device is VB2_ERR_NO_DEVICE).
// Plain C++17 like bam_io.h and fasta_io.h: no HIP header.
#ifndef VB2_BAQ_HOST_H_
#define VB2_BAQ_HOST_H_

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vb2_abi.h"      // vb2_baq_stats (plain C)
#include "bam_io.h"
#include "baq_core.h"
#include "fasta_io.h"

namespace vb2 {
namespace baq {

// pow and log of THIS host's libm: the quality table, and per j the largest double z with (int)(-4.343*log(z) + .499) >=
// j + 1, found by bisection over the doubles' bit patterns.  Built once per process.
const Tables& tables();
int reference_quality(double z);      // (int)(-4.343*log(z) + .499) with libm, for 0 < z (what the table must reproduce)

// what the effective mpileup options ask for (mplp_func, SimplePileupViewer.cpp:204-234)
struct Options {
    bool illumina = false, realn = true, redo = false;
    int cap = 40;                      // applied when > 10
    bool cap_on() const { return cap > 10; }
    bool needs_fasta() const { return realn || cap_on(); }
};
Options options_of(int incl_flags, int adjust_mq);

// The spans of the FASTA the scan's records can touch, nt16 codes one per byte.  A chunk's records lie in file order; a
// new span starts where a record's need begins more than kSpanGap bases behind the end of the span so far (a panel's
// markers lie far apart, and a merged chunk covers many of them), so only what the records can touch is read, once.
constexpr int64_t kSpanGap = 1024;
struct Spans {
    struct Span {
        int64_t beg = 0, end = 0;      // [beg, end) on the chunk's sequence
        uint64_t off = 0;              // of beg in `codes`
    };
    std::vector<uint8_t> codes;
    std::vector<std::vector<Span>> of_chunk;           // parallel to Scan::chunks: the chunk's spans, ascending
    std::vector<std::vector<uint32_t>> span_of_rec;    // per chunk, parallel to its recs: the record's span
    std::vector<int64_t> ref_len;      // per tid: the .fai's length (at most 2^31 - 1 counts), -1 = the FASTA lacks the sequence
    double seconds = 0;
    int64_t bytes_read = 0;
};
// fasta_path is not opened when the options need no FASTA (every ref_len is -1 then).
int load_spans(const bamio::Scan& scan, const std::string& fasta_path, const Options& opt, Spans* out, std::string* err);

// One record as the device stage gets it, beside its descriptor.  32 bytes.
struct Task {
    int32_t xb, l_ref, bw;             // the HMM's window [xb, xb + l_ref) and conf.bw (kind 2)
    int32_t span_beg;                  // position of the span's first code
    uint32_t span_off;                 // ... and where that code is in the spans' buffer
    int32_t ref_len;                   // the sequence's length (cap walk); 0 without a reference
    uint32_t bq_off;                   // the BQ string in the batch's extra bytes (kind 1)
    uint8_t kind;                      // 0 qualities copied (shifted), 1 BQ tag applied, 2 HMM
    uint8_t cap;                       // 1: the cap's walk runs
    uint8_t outcome;                   // baq_core.h's Outcome, final but for kCapDropped
    uint8_t pad;
};
static_assert(sizeof(Task) == 32, "tasks are 32 bytes");

// The record's auxiliary BQ / ZQ strings within its chunk's bytes (a field whose length passes the record ends the walk).
struct Tags {
    const uint8_t* bq = nullptr;       // l_seq bytes at least, else null
    bool zq = false;
};
Tags find_tags(const bamio::Chunk& ch, const bamio::RecordDesc& d);

// task of record `ri` of chunk `ci`; *bq (may come back null) are the bytes to put at Task::bq_off
Task make_task(const bamio::Scan& scan, size_t ci, size_t ri, const Spans& spans, const Options& opt, const uint8_t** bq);

// bam_cap_mapQ's end (bam_md.c:202-209) from the walk's four integers, with libm: -1 drops the read
int cap_finish(const int32_t cap4[4], int thres);
// mplp_func's use of it: the record's mapQ afterwards, -1 = dropped
inline int capped_mapq(int mapq, int cap) { return cap < 0 ? -1 : (mapq > cap ? cap : mapq); }
// A record's end once its cap4 is known: the mapQ the pileup sees (-1 = dropped: outside the sequence, or by the cap) and
// the final outcome, which is counted into *st (records and the outcome's own counter).
struct Finished {
    int mapq;
    uint8_t outcome;
};
Finished finish_record(int mapq, const Task& t, const int32_t cap4[4], const Options& opt, vb2_baq_stats* st);

// One record on the host, sequentially: out_qual (l_seq bytes) and cap4; returns the undefined rows.  rec: the record's
// variable part (name, CIGAR, bases, qualities); span: the spans' codes; extra: the bytes Task::bq_off points into.
int run_record(const bamio::RecordDesc& d, const uint8_t* rec, const Task& t, const uint8_t* span_codes, const uint8_t* extra,
               const Options& opt, uint8_t* out_qual, int32_t cap4[4], std::vector<double>* scratch);

// kpa_glocal alone over codes 0..4 (the fixture's cases): state and q, each l_query long; returns the undefined rows
int run_case(const uint8_t* ref, int l_ref, const uint8_t* query, const uint8_t* qual, int l_query, int conf_bw, int32_t* state,
             uint8_t* q);

}  // namespace baq

// vb2_baq_records: what --ApplyBAQ makes of the records the scan sends up (where 0: the host driver, 1: the device stage)
struct BaqRecords {
    std::vector<uint64_t> qual_off{0};       // record r's adjusted qualities are qual[qual_off[r], qual_off[r + 1])
    std::vector<uint8_t> qual, outcome;
    std::vector<int16_t> mapq;
    std::vector<int32_t> cap4;
    vb2_baq_stats stats{};
    void append(const uint8_t* q, int32_t l_seq, const baq::Finished& end, const int32_t c4[4])
    {
        qual.insert(qual.end(), q, q + l_seq);
        qual_off.push_back(qual.size());
        mapq.push_back((int16_t)end.mapq);
        outcome.push_back(end.outcome);
        cap4.insert(cap4.end(), c4, c4 + 4);
    }
};

}  // namespace vb2

#endif
