// bam_inflater_check_main.cpp -- TEST INFRASTRUCTURE ONLY: the BlockInflater hook of the built-in BAM reader's host stage
// (verifybamid_amd/csrc/bam_io.cpp) with a host-side inflater that calls the decoder of bgzf_inflate_core.h -- the hook, the
// zlib fallback and the identity of the errors without a GPU, in a program of its own so that tests/test_bam_cohort_cpu.py can
// run it under the host sanitizers:
//
//     g++ -std=c++17 -fsanitize=address,undefined -I verifybamid_amd/csrc tests/bam_inflater_check_main.cpp \
//         verifybamid_amd/csrc/bam_io.cpp -lz -lpthread -o bam_inflater_check
//     bam_inflater_check MARKERS THREADS FILE.bam [FILE.bam ...]
//
// Every file is scanned four times: without an inflater; with the core as inflater; with an inflater that refuses every
// second block (those go through zlib again); with one that says 0 for a block whose bytes it has spoilt (the CRC32 finds it
// out and zlib inflates the block again).  All four must agree in code, message, every chunk's bytes and every record, and
// the fourth must have had a block taken away from it wherever the first ended well over at least one byte.  Per file one line
//     same <code> <blocks given> <refused by the core> <refused by the second> <message, or "ok <records>"> | differ <what>
// Exit status 0 when no file differed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "bam_io.h"
#include "bgzf_inflate_core.h"

namespace bio = vb2::bamio;
namespace bz = vb2::bgzf;

struct CoreInflater : bio::BlockInflater {
    int mode;          // 0 the core; 1 every second block refused; 2 the first non-empty block spoilt, status 0
    size_t given = 0, refused = 0;
    explicit CoreInflater(int m) : mode(m) {}
    int run(const bio::InflateItem* items, size_t n, int32_t* status, std::string*) override
    {
        bool spoilt = false;
        for (size_t i = 0; i < n; ++i) {
            ++given;
            if (mode == 1 && (i & 1)) {
                status[i] = bz::kNotRun;
                ++refused;
                continue;
            }
            // exact-size copies on the heap: a byte outside is the sanitizer's
            std::vector<uint8_t> in(items[i].raw, items[i].raw + items[i].raw_len), out(items[i].isize);
            bz::Tables t;
            bz::PtrSource src{in.data()};
            bz::PtrSink sink{out.data()};
            uint64_t steps = 0;
            status[i] = bz::inflate(src, (uint32_t)in.size(), sink, items[i].isize, t, &steps);
            if (steps > bz::step_budget((uint32_t)in.size(), items[i].isize)) std::abort();
            if (status[i] != bz::kDone) {
                ++refused;
                continue;
            }
            if (mode == 2 && !spoilt && !out.empty()) {
                out[out.size() / 2] ^= 0x20;
                spoilt = true;
            }
            if (!out.empty()) std::memcpy(items[i].dst, out.data(), out.size());
        }
        return bio::kOk;
    }
};

static bool same_scan(const bio::Scan& a, const bio::Scan& b, std::string* what)
{
    if (a.chunks.size() != b.chunks.size()) { *what = "chunk count"; return false; }
    if (a.sample != b.sample || a.stats.blocks != b.stats.blocks || a.stats.records_seen != b.stats.records_seen ||
        a.stats.records_kept != b.stats.records_kept || a.stats.bytes_inflated != b.stats.bytes_inflated) { *what = "stats"; return false; }
    for (size_t i = 0; i < a.chunks.size(); ++i) {
        const bio::Chunk &x = a.chunks[i], &y = b.chunks[i];
        if (x.bytes != y.bytes) { *what = "bytes of chunk " + std::to_string(i); return false; }
        if (x.voffset != y.voffset || x.recs.size() != y.recs.size()) { *what = "records of chunk " + std::to_string(i); return false; }
        for (size_t r = 0; r < x.recs.size(); ++r)
            if (std::memcmp(&x.recs[r], &y.recs[r], sizeof(bio::RecordDesc)) != 0) { *what = "a descriptor of chunk " + std::to_string(i); return false; }
    }
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s MARKERS THREADS FILE.bam ...\n", argv[0]);
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
    std::vector<bio::SeqMarkers> markers;
    for (const std::string& name : order) {
        bio::SeqMarkers m;
        m.name = name;
        m.pos = by_name[name];
        std::sort(m.pos.begin(), m.pos.end());
        m.pos.erase(std::unique(m.pos.begin(), m.pos.end()), m.pos.end());
        markers.push_back(m);
    }
    const int threads = std::atoi(argv[2]);
    int bad = 0;
    for (int a = 3; a < argc; ++a) {
        bio::Scan plain, core, half, lied;
        std::string e0, e1, e2, e3, what;
        CoreInflater c0(0), c1(1), c2(2);
        const int r0 = bio::scan(argv[a], markers, threads, &plain, &e0);
        const int r1 = bio::scan(argv[a], markers, threads, &core, &e1, false, &c0);
        const int r2 = bio::scan(argv[a], markers, threads, &half, &e2, false, &c1);
        const int r3 = bio::scan(argv[a], markers, threads, &lied, &e3, false, &c2);
        bool ok = r0 == r1 && r0 == r2 && e0 == e1 && e0 == e2;
        if (!ok) what = "code or message: [" + std::to_string(r0) + " " + e0 + "] [" + std::to_string(r1) + " " + e1 + "] [" + std::to_string(r2) + " " + e2 + "]";
        if (ok && r0 == bio::kOk) ok = same_scan(plain, core, &what) && same_scan(plain, half, &what);
        if (ok && !(r3 == r0 && e3 == e0)) {
            ok = false;
            what = "code or message after a spoilt block: [" + std::to_string(r3) + " " + e3 + "]";
        }
        if (ok && r0 == bio::kOk) ok = same_scan(plain, lied, &what);
        if (ok && r0 == bio::kOk && plain.stats.bytes_inflated > 0 && lied.stats.inflater_refused < 1) {
            ok = false;
            what = "a spoilt block with status 0 passed its CRC32";
        }
        if (ok) {
            unsigned long long recs = 0;
            for (const bio::Chunk& ch : plain.chunks) recs += ch.recs.size();
            std::printf("same %d %zu %zu %zu %s\n", r0, c0.given, c0.refused, c1.refused, r0 == bio::kOk ? ("ok " + std::to_string(recs)).c_str() : e0.c_str());
        } else {
            std::printf("differ %s: %s\n", argv[a], what.c_str());
            ++bad;
        }
    }
    return bad ? 1 : 0;
}
