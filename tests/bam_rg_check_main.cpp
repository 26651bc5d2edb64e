// bam_rg_check_main.cpp -- TEST INFRASTRUCTURE ONLY: the read-group side of the built-in BAM reader's host stage
// (verifybamid_amd/csrc/bam_io.cpp: the @RG lines and the walk over a record's auxiliary fields) in a
// program of its own, so that tests/test_readgroups_cpu.py can run it under the host sanitizers:
//
//     g++ -std=c++17 -fsanitize=address,undefined -I verifybamid_amd/csrc tests/bam_rg_check_main.cpp \
//         verifybamid_amd/csrc/bam_io.cpp -lz -lpthread -o bam_rg_check
//     bam_rg_check MARKERS THREADS (ok|aux) FILE.bam [(ok|aux) FILE.bam ...]
//
// MARKERS: lines "sequence position" (1-based).  Per file two lines.  The scan that was asked for groups:
// "groups ok <records> <unassigned> <number of groups> <sum of the records' group numbers>" or "groups error <code>
// <message>"; the plain scan of the same file: "plain ok <records>" or "plain error <code> <message>".  ok: both succeed
// with the same records.  aux: a file whose auxiliary fields are malformed -- the first must end in kErrInvalid with a
// message, the second must succeed, because it does not look at them.  Exit status 0 when every file met its expectation.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "bam_io.h"

int main(int argc, char** argv)
{
    if (argc < 5 || (argc - 3) % 2 != 0) {
        std::fprintf(stderr, "usage: %s MARKERS THREADS (ok|aux) FILE.bam ...\n", argv[0]);
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
        unsigned long long recs_groups = 0, recs_plain = 0;
        {
            vb2::bamio::Scan scan;
            std::string err;
            const int rc = vb2::bamio::scan(argv[a + 1], markers, threads, &scan, &err, true);
            if (rc == vb2::bamio::kOk) {
                unsigned long long sum = 0, none = 0;
                for (const vb2::bamio::Chunk& ch : scan.chunks) {
                    if (ch.group.size() != ch.recs.size()) ++bad;
                    for (const uint16_t g : ch.group) {
                        if (g == vb2::bamio::kNoGroup) ++none;
                        else if (g >= scan.groups.size()) ++bad;
                        else sum += g;
                    }
                    recs_groups += ch.recs.size();
                }
                if (none != (unsigned long long)scan.stats.records_unassigned) ++bad;
                std::printf("groups ok %llu %llu %zu %llu\n", recs_groups, none, scan.groups.size(), sum);
                if (!want_ok) ++bad;
            } else {
                std::printf("groups error %d %s\n", rc, err.c_str());
                if (want_ok || err.empty() || rc != vb2::bamio::kErrInvalid) ++bad;
            }
        }
        {
            vb2::bamio::Scan scan;
            std::string err;
            const int rc = vb2::bamio::scan(argv[a + 1], markers, threads, &scan, &err);
            if (rc == vb2::bamio::kOk) {
                for (const vb2::bamio::Chunk& ch : scan.chunks) {
                    if (!ch.group.empty() || !scan.groups.empty()) ++bad;      // not asked for: not looked at
                    recs_plain += ch.recs.size();
                }
                std::printf("plain ok %llu\n", recs_plain);
                if (want_ok && recs_plain != recs_groups) ++bad;
            } else {
                std::printf("plain error %d %s\n", rc, err.c_str());
                ++bad;
            }
        }
    }
    return bad ? 1 : 0;
}
