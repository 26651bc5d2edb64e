// baq_check_main.cpp -- TEST INFRASTRUCTURE ONLY: the FASTA reader (fasta_io.cpp) and the host core of --ApplyBAQ
// (baq_core.h through baq_host.cpp) in a program of their own, so that tests/test_baq_cpu.py can build them with
// -fsanitize=address,undefined and run them directly (no LD_PRELOAD, nothing loaded into Python).
//
//   baq_check <cases> <markers> <bam> <fasta> <incl_flags> <adjust_mq> <expected> [fail <fasta>]...
//
// <cases>: per line "name bw ref query qual state q", arrays as hex ("-" = empty): the HMM alone must give state and q.
// <markers>: per line "sequence position" (1-based).  <expected>: per record of the scan "outcome mapq mm q len clip_q
// qualities-as-hex" -- what the wrapper and the cap must give under the two options.  Every "fail" FASTA (a mutilated
// file or index) must end in an error code with a message.  Prints one line per check; exit status 0 when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "bam_io.h"
#include "baq_host.h"
#include "fasta_io.h"

using namespace vb2;

static std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

int main(int argc, char** argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: baq_check cases markers bam fasta incl_flags adjust_mq expected [fail fasta]...\n");
        return 2;
    }
    int failures = 0;
    {   // the HMM alone
        std::ifstream in(argv[1]);
        std::string name, r, q, ql, st, qq;
        int bw, n = 0, bad = 0;
        while (in >> name >> bw >> r >> q >> ql >> st >> qq) {
            const std::vector<uint8_t> ref = unhex(r), query = unhex(q), qual = unhex(ql), want_state = unhex(st), want_q = unhex(qq);
            std::vector<int32_t> state(query.size() + 1);
            std::vector<uint8_t> got_q(query.size() + 1);
            const int und = baq::run_case(ref.data(), (int)ref.size(), query.data(), qual.data(), (int)query.size(), bw, state.data(), got_q.data());
            bool ok = und == 0 && want_q.size() == query.size() && want_state.size() == 4 * query.size();
            for (size_t i = 0; ok && i < query.size(); ++i) {
                const int32_t w = (int32_t)baq::rd32u(want_state.data() + 4 * i);
                ok = w == state[i] && want_q[i] == got_q[i];
            }
            ++n;
            if (!ok) {
                ++bad;
                std::printf("case %s differs\n", name.c_str());
            }
        }
        std::printf("cases %d bad %d\n", n, bad);
        failures += bad + (n == 0);
    }
    std::vector<bamio::SeqMarkers> markers;
    {
        std::ifstream in(argv[2]);
        std::map<std::string, size_t> at;
        std::string name;
        int32_t pos;
        while (in >> name >> pos) {
            if (!at.count(name)) {
                at[name] = markers.size();
                markers.push_back(bamio::SeqMarkers{name, {}});
            }
            markers[at[name]].pos.push_back(pos);
        }
        for (bamio::SeqMarkers& m : markers) {
            std::sort(m.pos.begin(), m.pos.end());
            m.pos.erase(std::unique(m.pos.begin(), m.pos.end()), m.pos.end());
        }
    }
    bamio::Scan scan;
    std::string err;
    if (int rc = bamio::scan(argv[3], markers, 2, &scan, &err)) {
        std::printf("scan failed %d %s\n", rc, err.c_str());
        return 1;
    }
    const baq::Options opt = baq::options_of(std::atoi(argv[5]), std::atoi(argv[6]));
    {   // the wrapper and the cap over the records
        baq::Spans spans;
        if (int rc = baq::load_spans(scan, argv[4], opt, &spans, &err)) {
            std::printf("spans failed %d %s\n", rc, err.c_str());
            return 1;
        }
        std::ifstream in(argv[7]);
        int n = 0, bad = 0;
        std::vector<double> scratch;
        vb2_baq_stats tally{};
        for (size_t ci = 0; ci < scan.chunks.size(); ++ci) {
            const bamio::Chunk& ch = scan.chunks[ci];
            for (size_t ri = 0; ri < ch.recs.size(); ++ri) {
                const bamio::RecordDesc& d = ch.recs[ri];
                const uint8_t* bq = nullptr;
                baq::Task t = baq::make_task(scan, ci, ri, spans, opt, &bq);
                if (t.kind == 1) t.bq_off = 0;
                std::vector<uint8_t> q((size_t)d.l_seq + 1);
                int32_t c4[4];
                baq::run_record(d, ch.bytes.data() + d.data, t, spans.codes.data(), bq, opt, q.data(), c4, &scratch);
                const baq::Finished end = baq::finish_record(d.mapq, t, c4, opt, &tally);
                const int mq = end.mapq, oc = end.outcome;
                int w_oc, w_mq, w4[4];
                std::string hex;
                if (!(in >> w_oc >> w_mq >> w4[0] >> w4[1] >> w4[2] >> w4[3] >> hex)) {
                    std::printf("expected file ends at record %d\n", n);
                    return 1;
                }
                const std::vector<uint8_t> wq = unhex(hex);
                bool ok = w_oc == oc && w_mq == mq && wq.size() == (size_t)d.l_seq;
                for (int k = 0; k < 4; ++k) ok = ok && w4[k] == c4[k];
                for (size_t i = 0; ok && i < wq.size(); ++i) ok = wq[i] == q[i];
                ++n;
                if (!ok) {
                    ++bad;
                    std::printf("record %d differs (outcome %d want %d, mapq %d want %d)\n", n - 1, oc, w_oc, mq, w_mq);
                }
            }
        }
        std::printf("records %d bad %d fasta_bytes %lld\n", n, bad, (long long)spans.bytes_read);
        failures += bad + (n == 0) + (tally.records != n);
    }
    for (int a = 8; a + 1 < argc; a += 2) {
        baq::Spans spans;
        err.clear();
        const int rc = baq::load_spans(scan, argv[a + 1], opt, &spans, &err);
        const bool ok = rc != 0 && !err.empty();
        std::printf("%s %s rc %d %s\n", ok ? "refused" : "ACCEPTED", argv[a + 1], rc, err.c_str());
        failures += ok ? 0 : 1;
    }
    return failures ? 1 : 0;
}
