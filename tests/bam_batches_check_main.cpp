// bam_batches_check_main.cpp -- TEST INFRASTRUCTURE ONLY: the batch cutter of the built-in BAM reader (bam_batches.cpp) in a
// program of its own, so that tests/test_bam_batches_cpu.py can build it with -fsanitize=address,undefined and run it
// directly (no LD_PRELOAD, nothing loaded into Python).  It builds bamio::Scans by hand from the lines of <cases>:
//
//   plan <name> <kb>                   an empty scan through plan_batches alone (nothing is allocated)
//   cut  <name> <kb> <who> <chunks>    chunks: "-" (none) or chunks joined by "|"; a chunk is "e" (empty) or records
//                                      "l_read_name:n_cigar:l_seq" joined by ","
//   pass <name> <kb> <who> <chunks>    as cut, the last chunk's bytes one short of its last record
//   baq  <name> <kb> <records>         one chunk of whole records "l_seq:tag" (b: a BQ tag of l_seq, s: a BQ tag one short,
//                                      n: none), names of 200 bytes, position 100 on a sequence of 100 000; BAQ on, cap off
//
// and prints per case "case <name> rc <rc> bytes <batch_bytes> rec <batch_rec> err <text>", then per batch
// "batch <nr> <nb> off <data offsets> grp <groups> [kind <kinds> bq <bq_offs> extra <hex>]" and "copied <0|1>" (the
// batch's bytes are the records' own).  Exit status 0 unless a line cannot be parsed.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bam_batches.h"

using namespace vb2;

static std::vector<std::string> split(const std::string& s, char sep)
{
    std::vector<std::string> out;
    std::string one;
    std::istringstream in(s);
    while (std::getline(in, one, sep)) out.push_back(one);
    return out;
}

static void put32(std::vector<uint8_t>* b, uint32_t v)
{
    for (int k = 0; k < 4; ++k) b->push_back((uint8_t)(v >> (8 * k)));
}

// "l_read_name:n_cigar:l_seq" records: the variable parts alone, back to back, filled with a pattern
static void add_chunk(bamio::Scan* scan, const std::string& spec, bool with_groups)
{
    bamio::Chunk ch;
    ch.tid = 0;
    if (spec != "e")
        for (const std::string& r : split(spec, ',')) {
            int ln = 0, nc = 0, ls = 0;
            if (std::sscanf(r.c_str(), "%d:%d:%d", &ln, &nc, &ls) != 3) continue;
            bamio::RecordDesc d{};
            d.data = (uint32_t)ch.bytes.size();
            d.l_read_name = (uint8_t)ln;
            d.n_cigar = (uint16_t)nc;
            d.l_seq = ls;
            d.order = (uint32_t)ch.recs.size();
            for (size_t k = 0; k < var_bytes(d); ++k) ch.bytes.push_back((uint8_t)(31 * scan->chunks.size() + 7 * ch.recs.size() + k));
            if (with_groups) ch.group.push_back((uint16_t)(ch.recs.size() % 3));
            ch.recs.push_back(d);
        }
    scan->chunks.push_back(ch);
}

// whole records with a BQ tag or without, and the spans that cover them
static void add_baq_chunk(bamio::Scan* scan, baq::Spans* spans, const std::string& spec)
{
    scan->ref_name.assign(1, "chr1");
    scan->ref_len.assign(1, 100000);
    bamio::Chunk ch;
    ch.tid = 0;
    for (const std::string& r : split(spec, ',')) {
        int ls = 0;
        char tag = 'n';
        if (std::sscanf(r.c_str(), "%d:%c", &ls, &tag) != 2) continue;
        std::vector<uint8_t> body(32, 0);          // the fixed fields: nothing below the cutter reads them
        bamio::RecordDesc d{};
        d.tid = 0;
        d.pos = 100;
        d.mapq = 60;
        d.l_read_name = 200;
        d.n_cigar = 1;
        d.l_seq = ls;
        d.order = (uint32_t)ch.recs.size();
        for (int k = 0; k < 199; ++k) body.push_back((uint8_t)('a' + (k + ch.recs.size()) % 26));
        body.push_back(0);
        put32(&body, (uint32_t)ls << 4);           // <l_seq>M
        for (int k = 0; k < (ls + 1) / 2; ++k) body.push_back(0x12);
        for (int k = 0; k < ls; ++k) body.push_back((uint8_t)(20 + k % 20));
        if (tag != 'n') {
            body.push_back('B');
            body.push_back('Q');
            body.push_back('Z');
            for (int k = 0; k < (tag == 'b' ? ls : ls - 1); ++k) body.push_back((uint8_t)('@' + (k + ch.recs.size()) % 5));
            body.push_back(0);
        }
        put32(&ch.bytes, (uint32_t)body.size());
        d.data = (uint32_t)ch.bytes.size() + 32;
        ch.bytes.insert(ch.bytes.end(), body.begin(), body.end());
        ch.recs.push_back(d);
    }
    spans->codes.assign(2000, 1);
    spans->ref_len.assign(1, 100000);
    baq::Spans::Span one;
    one.beg = 0;
    one.end = 2000;
    spans->of_chunk.assign(1, std::vector<baq::Spans::Span>(1, one));
    spans->span_of_rec.assign(1, std::vector<uint32_t>(ch.recs.size(), 0u));
    scan->chunks.push_back(ch);
}

enum How { kPlanOnly, kCut, kCutWithGroups };

static void run_case(const bamio::Scan& scan, int kb, const std::string& name, const std::string& who, const baq::Spans* spans, How how)
{
    const bool with_groups = how == kCutWithGroups;
    const baq::Options opt = baq::options_of(16, 0);
    BatchPlan plan;
    std::string err;
    int rc = plan_batches(scan, kb, who, &plan, &err);
    if (rc || how == kPlanOnly) {
        std::printf("case %s rc %d bytes %zu rec %zu err %s\n", name.c_str(), rc, plan.batch_bytes, plan.batch_rec, err.empty() ? "-" : err.c_str());
        return;
    }
    std::vector<uint8_t> bytes(plan.batch_bytes);
    std::vector<bamio::RecordDesc> desc(plan.batch_rec);
    std::vector<uint16_t> group(plan.batch_rec);
    RecordBatch b;
    b.bytes = bytes.data();
    b.desc = desc.data();
    b.group = with_groups ? group.data() : nullptr;
    std::ostringstream lines;
    size_t ci = 0, ri = 0;                        // the records in order, to compare the copied bytes with
    for (BatchCursor cur(scan, plan, spans, spans ? &opt : nullptr); !rc && !cur.done();) {
        rc = cur.next(&b, who, &err);
        if (rc) break;
        lines << "batch " << b.nr << " " << b.nb << " off";
        bool copied = true;
        for (size_t r = 0; r < b.nr; ++r) {
            lines << (r ? "," : " ") << b.desc[r].data;
            while (ri >= scan.chunks[ci].recs.size()) {
                ++ci;
                ri = 0;
            }
            const bamio::RecordDesc& d = scan.chunks[ci].recs[ri++];
            copied = copied && d.order == b.desc[r].order && d.l_seq == b.desc[r].l_seq &&
                     std::memcmp(b.bytes + b.desc[r].data, scan.chunks[ci].bytes.data() + d.data, var_bytes(d)) == 0;
        }
        lines << " grp";
        for (size_t r = 0; r < b.nr && b.group; ++r) lines << (r ? "," : " ") << b.group[r];
        if (spans) {
            lines << " kind";
            for (size_t r = 0; r < b.tasks.size(); ++r) lines << (r ? "," : " ") << (int)b.tasks[r].kind;
            lines << " bq";
            for (size_t r = 0; r < b.tasks.size(); ++r) lines << (r ? "," : " ") << b.tasks[r].bq_off;
            lines << " extra ";
            char hex[3];
            for (const uint8_t x : b.extra) {
                std::snprintf(hex, sizeof(hex), "%02x", x);
                lines << hex;
            }
        }
        lines << "\ncopied " << (copied ? 1 : 0) << "\n";
    }
    std::printf("case %s rc %d bytes %zu rec %zu err %s\n%s", name.c_str(), rc, plan.batch_bytes, plan.batch_rec, err.empty() ? "-" : err.c_str(),
                lines.str().c_str());
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: bam_batches_check cases\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string mode, name, who, spec;
        int kb = 0;
        f >> mode >> name >> kb;
        bamio::Scan scan;
        baq::Spans spans;
        if (mode == "plan") {
            run_case(scan, kb, name, "--BamFile", nullptr, kPlanOnly);
        } else if (mode == "cut" || mode == "pass") {
            f >> who >> spec;
            if (spec != "-")
                for (const std::string& c : split(spec, '|')) add_chunk(&scan, c, scan.chunks.size() > 0);      // (the first chunk without groups)
            if (mode == "pass" && !scan.chunks.empty() && !scan.chunks.back().bytes.empty()) scan.chunks.back().bytes.pop_back();
            run_case(scan, kb, name, who, nullptr, kCutWithGroups);
        } else if (mode == "baq") {
            f >> spec;
            add_baq_chunk(&scan, &spans, spec);
            run_case(scan, kb, name, "--BamFile", &spans, kCut);
        } else {
            std::fprintf(stderr, "cannot parse: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
