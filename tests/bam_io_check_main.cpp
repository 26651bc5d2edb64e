// bam_io_check_main.cpp -- TEST INFRASTRUCTURE ONLY: the built-in BAM reader's host stage (verifybamid_amd/csrc/bam_io.cpp)
// in a program of its own, so that tests/test_bam_cpu.py can run it under the host sanitizers:
//
//     g++ -std=c++17 -fsanitize=address,undefined -I verifybamid_amd/csrc tests/bam_io_check_main.cpp \
//         verifybamid_amd/csrc/bam_io.cpp -lz -lpthread -o bam_io_check
//     bam_io_check MARKERS THREADS (ok|fail) FILE.bam [(ok|fail) FILE.bam ...]
//
// MARKERS: lines "sequence position" (1-based).  Per file one line "ok <records> <bytes>" or "error <code> <message>";
// every kept record's name, CIGAR, bases and qualities are read through once, so that a descriptor that points outside
// its chunk is a sanitizer report.  Exit status 0 when every file met its expectation (a failure must come with a message).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "bam_io.h"

int main(int argc, char** argv)
{
    if (argc < 5 || (argc - 3) % 2 != 0) {
        std::fprintf(stderr, "usage: %s MARKERS THREADS (ok|fail) FILE.bam ...\n", argv[0]);
        return 2;
    }
    std::map<std::string, std::vector<int32_t>> by_name;
    std::vector<std::string> order;
    {
        std::ifstream in(argv[1]);
        std::string name;
        long pos;
        while (in >> name >> pos) {
            if (!by_name.count(name)) order.push_back(name);
            by_name[name].push_back((int32_t)pos);
        }
    }
    std::vector<vb2::bamio::SeqMarkers> markers;
    for (const std::string& name : order) {
        vb2::bamio::SeqMarkers m;
        m.name = name;
        m.pos = by_name[name];
        std::sort(m.pos.begin(), m.pos.end());
        m.pos.erase(std::unique(m.pos.begin(), m.pos.end()), m.pos.end());
        markers.push_back(m);
    }
    const int threads = std::atoi(argv[2]);
    int bad = 0;
    for (int a = 3; a + 1 < argc; a += 2) {
        const bool want_ok = std::strcmp(argv[a], "ok") == 0;
        vb2::bamio::Scan scan;
        std::string err;
        const int rc = vb2::bamio::scan(argv[a + 1], markers, threads, &scan, &err);
        if (rc == vb2::bamio::kOk) {
            unsigned long long sum = 0, bytes = 0, recs = 0;
            for (const vb2::bamio::Chunk& ch : scan.chunks)
                for (const vb2::bamio::RecordDesc& d : ch.recs) {
                    const size_t n = (size_t)d.l_read_name + 4 * (size_t)d.n_cigar + ((size_t)d.l_seq + 1) / 2 + (size_t)d.l_seq;
                    for (size_t i = 0; i < n; ++i) sum += ch.bytes[(size_t)d.data + i];      // (operator[] of the vector: ASan checks it)
                    bytes += n;
                    ++recs;
                }
            std::printf("ok %llu %llu %llu %s\n", recs, bytes, sum, argv[a + 1]);
            if (!want_ok) ++bad;
        } else {
            std::printf("error %d %s\n", rc, err.c_str());
            if (want_ok || err.empty() || (rc != vb2::bamio::kErrIo && rc != vb2::bamio::kErrInvalid)) ++bad;
        }
    }
    return bad ? 1 : 0;
}
