// bgzf_inflate_check_main.cpp -- the DEFLATE decoder of verifybamid_amd/csrc/bgzf_inflate_core.h on the CPU, against zlib,
// as a program of its own so that it runs under the host sanitizers (tests/test_bgzf_inflate_cpu.py builds it with
// -fsanitize=address,undefined and -lz alone).
//
//   bgzf_inflate_check <file of BAM record bytes>
//
// It makes its corpus with zlib's deflate in raw mode (levels 0, 1, 6, 9 x strategies default, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE x
// no flush, Z_SYNC_FLUSH and Z_FULL_FLUSH in mid-stream x eleven lengths x five contents), inflates every stream with the
// core and with zlib, and prints per stream
//   stream <content> <length> <level> <strategy> <flush> <raw_len> <status> <steps> <budget> <equal 0/1>
// (after the cross product three streams zlib's deflate never writes, assembled by hand: content hand_*, level -1), then
// one line `census ...` over the corpus, then per small stream `small <name> <raw_len> <status> stored <n> fixed <n>
// dynamic <n> <the stream in hex>` and its mutilations (every single-bit flip, every truncation):
//   mut <stored|fixed|dynamic> <flip|cut> <index> <status> <steps> <budget> <zlib ok 0/1> <equal 0/1/-1 (not compared)>
// Exit status 0 when every line is as it must be (the Python test reads the lines as well), 1 otherwise.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bgzf_inflate_core.h"

namespace bz = vb2::bgzf;

// the generator tests/bgzf_ref.py restates: x <- (1103515245 x + 12345) mod 2^31, a value is x >> 16
struct Lcg {
    uint32_t x;
    uint32_t next() { x = (1103515245u * x + 12345u) & 0x7fffffffu; return x >> 16; }
};

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t>& in, int level, int strategy, int flush_mid)
{
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) { std::fprintf(stderr, "deflateInit2 failed\n"); std::exit(2); }
    std::vector<uint8_t> out(deflateBound(&zs, (uLong)in.size()) + 64);
    static uint8_t none = 0;
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    const size_t half = in.size() / 2;
    if (flush_mid != Z_NO_FLUSH) {
        zs.next_in = in.empty() ? &none : const_cast<uint8_t*>(in.data());
        zs.avail_in = (uInt)half;
        if (deflate(&zs, flush_mid) != Z_OK) { std::fprintf(stderr, "deflate(flush) failed\n"); std::exit(2); }
    }
    const size_t done = flush_mid != Z_NO_FLUSH ? half : 0;
    zs.next_in = in.empty() ? &none : const_cast<uint8_t*>(in.data() + done);
    zs.avail_in = (uInt)(in.size() - done);
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { std::fprintf(stderr, "deflate(finish) failed\n"); std::exit(2); }
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

// zlib's verdict on a raw stream that must give exactly isize bytes
static bool zlib_inflate(const std::vector<uint8_t>& raw, uint32_t isize, std::vector<uint8_t>* out)
{
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) std::exit(2);
    out->assign((size_t)isize + 1, 0);
    static uint8_t none = 0;
    zs.next_in = raw.empty() ? &none : const_cast<uint8_t*>(raw.data());
    zs.avail_in = (uInt)raw.size();
    zs.next_out = out->data();
    zs.avail_out = (uInt)out->size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == isize;
    inflateEnd(&zs);
    out->resize(isize);
    return ok;
}

static int32_t core_inflate(const std::vector<uint8_t>& raw, uint32_t isize, std::vector<uint8_t>* out, uint64_t* steps, bz::Census* census)
{
    // exact sizes on the heap: a read or write one byte outside is the sanitizer's
    std::vector<uint8_t> in(raw);
    out->assign(isize, 0xAA);
    bz::Tables t;
    bz::PtrSource src{in.data()};
    bz::PtrSink sink{out->data()};
    return bz::inflate(src, (uint32_t)in.size(), sink, isize, t, steps, census);
}

// ---- streams zlib's deflate never writes, assembled by hand from RFC 1951 (tests/bgzf_ref.py restates them) ----
// zlib 1.2.11 keeps matches within 32 768 - 262 bytes and gives every distance tree at least two codes, so a match at
// distance 32 768, a distance tree of one code and one of none come from here.  zlib's inflate accepts all three.
struct BitWriter {
    std::vector<uint8_t> bytes;
    uint32_t nbit = 0;
    void bits(uint32_t v, uint32_t n)                  // n bits of v, least significant first (3.1.1: everything but codes)
    {
        for (uint32_t i = 0; i < n; ++i) {
            if ((nbit & 7) == 0) bytes.push_back(0);
            bytes.back() |= (uint8_t)(((v >> i) & 1u) << (nbit & 7));
            ++nbit;
        }
    }
    void code(uint32_t c, uint32_t n) { for (uint32_t i = n; i-- > 0;) bits((c >> i) & 1u, 1); }       // a Huffman code: most significant first
    void align() { nbit = (nbit + 7) & ~7u; }
};

// canonical codes of a set of lengths (3.2.2)
static std::vector<uint32_t> canonical(const std::vector<int>& len)
{
    int count[16] = {0};
    for (int l : len) ++count[l];
    count[0] = 0;
    uint32_t next[16] = {0}, c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + (uint32_t)count[b - 1]) << 1; next[b] = c; }
    std::vector<uint32_t> code(len.size(), 0);
    for (size_t i = 0; i < len.size(); ++i) if (len[i]) code[i] = next[len[i]]++;
    return code;
}

struct Token { int sym; int dsym; };                    // a literal (dsym < 0), or a length symbol without extra bits and a distance symbol without

// one dynamic block: the code-length code is complete whatever it has to carry (0..15: 5 bits, 16 and 17: 3 bits, 18: 2 bits)
static void dynamic_block(BitWriter& w, bool final_block, const std::vector<int>& lit, const std::vector<int>& dist, const std::vector<Token>& tokens)
{
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    std::vector<int> cl(19, 5);
    cl[16] = cl[17] = 3;
    cl[18] = 2;
    const std::vector<uint32_t> clc = canonical(cl), lc = canonical(lit), dc = canonical(dist);
    w.bits(final_block ? 1 : 0, 1);
    w.bits(2, 2);
    w.bits((uint32_t)lit.size() - 257, 5);
    w.bits((uint32_t)dist.size() - 1, 5);
    w.bits(19 - 4, 4);
    for (int i = 0; i < 19; ++i) w.bits((uint32_t)cl[order[i]], 3);
    std::vector<int> all(lit);
    all.insert(all.end(), dist.begin(), dist.end());
    for (size_t i = 0; i < all.size();) {
        size_t run = 1;
        while (i + run < all.size() && all[i + run] == all[i]) ++run;
        if (all[i] == 0 && run >= 11) {
            const size_t r = run > 138 ? 138 : run;
            w.code(clc[18], 2);
            w.bits((uint32_t)r - 11, 7);
            i += r;
        } else if (all[i] == 0 && run >= 3) {
            w.code(clc[17], 3);
            w.bits((uint32_t)run - 3, 3);
            i += run;
        } else {
            w.code(clc[(size_t)all[i]], 5);
            ++i;
        }
    }
    for (const Token& t : tokens) {
        w.code(lc[(size_t)t.sym], (uint32_t)lit[(size_t)t.sym]);
        if (t.dsym >= 0) w.code(dc[(size_t)t.dsym], (uint32_t)dist[(size_t)t.dsym]);
    }
    w.code(lc[256], (uint32_t)lit[256]);
}

struct Hand { const char* name; std::vector<uint8_t> raw, plain; };

static std::vector<Hand> handmade()
{
    std::vector<Hand> out;
    {   // a stored block of 32 768 bytes, then a fixed block: length 258 (symbol 285) at distance 32 768 (symbol 29, 13 extra bits all set)
        Hand h{"hand_dist32768", {}, std::vector<uint8_t>(32768)};
        Lcg g{777u};
        for (uint8_t& b : h.plain) b = (uint8_t)g.next();
        BitWriter w;
        w.bits(0, 1);
        w.bits(0, 2);
        w.align();
        w.bits(32768, 16);
        w.bits(32768 ^ 0xffffu, 16);
        w.bytes.insert(w.bytes.end(), h.plain.begin(), h.plain.end());
        w.nbit = (uint32_t)w.bytes.size() * 8;
        w.bits(1, 1);
        w.bits(1, 2);
        w.code(0xC0 + (285 - 280), 8);
        w.code(29, 5);
        w.bits(8191, 13);
        w.code(0, 7);
        for (int i = 0; i < 258; ++i) h.plain.push_back(h.plain[(size_t)i]);
        h.raw = w.bytes;
        out.push_back(h);
    }
    {   // "abc", then two matches of 258 at distance 3; the distance tree is the one code of symbol 2
        Hand h{"hand_one_dist", {}, {}};
        std::vector<int> lit(286, 0), dist(3, 0);
        lit['a'] = lit['b'] = lit['c'] = 2;
        lit[256] = lit[285] = 3;
        dist[2] = 1;
        BitWriter w;
        dynamic_block(w, true, lit, dist, {{'a', -1}, {'b', -1}, {'c', -1}, {285, 2}, {285, 2}});
        for (int i = 0; i < 3 + 2 * 258; ++i) h.plain.push_back((uint8_t)"abc"[i % 3]);
        h.raw = w.bytes;
        out.push_back(h);
    }
    {   // literals only, HDIST = 1 with a length of zero: no distance code at all
        Hand h{"hand_empty_dist", {}, {}};
        std::vector<int> lit(257, 0), dist(1, 0);
        lit['a'] = lit['b'] = lit['c'] = lit[256] = 2;
        BitWriter w;
        std::vector<Token> tokens;
        for (int i = 0; i < 40; ++i) {
            tokens.push_back({"abc"[(i * i) % 3], -1});
            h.plain.push_back((uint8_t)"abc"[(i * i) % 3]);
        }
        dynamic_block(w, true, lit, dist, tokens);
        h.raw = w.bytes;
        out.push_back(h);
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <file of BAM record bytes>\n", argv[0]); return 2; }
    std::vector<uint8_t> bam;
    if (FILE* fh = std::fopen(argv[1], "rb")) {
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), fh)) > 0) bam.insert(bam.end(), buf, buf + n);
        std::fclose(fh);
    }
    if (bam.empty()) { std::fprintf(stderr, "%s: empty or unreadable\n", argv[1]); return 2; }
    int bad = 0;

    const uint32_t lengths[] = {0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65280, 65536};
    const char* content_names[] = {"zeros", "random", "twice32k", "period3", "bam"};
    const int levels[] = {0, 1, 6, 9};
    const int strategies[] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE};
    const char* strategy_names[] = {"default", "fixed", "huffman", "rle"};
    const int flushes[] = {Z_NO_FLUSH, Z_SYNC_FLUSH, Z_FULL_FLUSH};
    const char* flush_names[] = {"none", "sync", "full"};
    bz::Census census;
    for (int c = 0; c < 5; ++c)
        for (uint32_t n : lengths) {
            std::vector<uint8_t> plain(n);
            Lcg g{12345u + (uint32_t)c};
            if (c == 1) for (uint32_t i = 0; i < n; ++i) plain[i] = (uint8_t)g.next();
            if (c == 2) {                                  // 32 768 random bytes, then the same again: distance 32 768
                for (uint32_t i = 0; i < n && i < 32768; ++i) plain[i] = (uint8_t)g.next();
                for (uint32_t i = 32768; i < n; ++i) plain[i] = plain[i - 32768];
            }
            if (c == 3) for (uint32_t i = 0; i < n; ++i) plain[i] = (uint8_t)"abc"[i % 3];
            if (c == 4) for (uint32_t i = 0; i < n; ++i) plain[i] = bam[i % bam.size()];
            for (int li = 0; li < 4; ++li)
                for (int si = 0; si < 4; ++si)
                    for (int fi = 0; fi < 3; ++fi) {
                        const std::vector<uint8_t> raw = deflate_raw(plain, levels[li], strategies[si], flushes[fi]);
                        std::vector<uint8_t> want, got;
                        if (!zlib_inflate(raw, n, &want) || want != plain) { std::fprintf(stderr, "zlib does not round-trip its own stream\n"); return 2; }
                        uint64_t steps = 0;
                        const int32_t st = core_inflate(raw, n, &got, &steps, &census);
                        const uint64_t budget = bz::step_budget((uint32_t)raw.size(), n);
                        const bool equal = got == plain;
                        std::printf("stream %s %u %d %s %s %zu %d %llu %llu %d\n", content_names[c], n, levels[li], strategy_names[si],
                                    flush_names[fi], raw.size(), (int)st, (unsigned long long)steps, (unsigned long long)budget, (int)equal);
                        if (st != bz::kDone || !equal || steps > budget) ++bad;
                    }
        }
    for (const Hand& h : handmade()) {
        const uint32_t n = (uint32_t)h.plain.size();
        std::vector<uint8_t> want, got;
        const bool zok = zlib_inflate(h.raw, n, &want) && want == h.plain;
        uint64_t steps = 0;
        const int32_t st = core_inflate(h.raw, n, &got, &steps, &census);
        const uint64_t budget = bz::step_budget((uint32_t)h.raw.size(), n);
        const bool equal = got == h.plain;
        std::printf("stream %s %u -1 hand none %zu %d %llu %llu %d\n", h.name, n, h.raw.size(), (int)st, (unsigned long long)steps,
                    (unsigned long long)budget, (int)equal);
        if (!zok) std::fprintf(stderr, "%s: zlib does not accept the hand-made stream\n", h.name);
        if (!zok || st != bz::kDone || !equal || steps > budget) ++bad;
    }
    std::printf("census stored %u fixed %u dynamic %u empty_stored_off_byte %u longest_match %u largest_distance %u overlapping %u "
                "rep16 %u rep17 %u rep18 %u one_code_dist %u empty_dist %u\n",
                census.stored, census.fixed, census.dynamic, census.empty_stored_off_byte, census.longest_match, census.largest_distance,
                census.overlapping, census.rep16, census.rep17, census.rep18, census.one_code_dist, census.empty_dist);

    // ---- mutilations of three small streams (tests/bgzf_ref.py builds the same three) ----
    std::vector<uint8_t> text(480);
    {
        Lcg g{2024u};
        for (uint8_t& b : text) {
            const uint32_t r = g.next() & 15u;
            b = (uint8_t)(r < 8 ? 'A' : r < 12 ? 'C' : r < 14 ? 'G' : r < 15 ? 'T' : 'N');
        }
    }
    struct Small { const char* name; std::vector<uint8_t> plain; int level, strategy; };
    const Small smalls[3] = {{"stored", std::vector<uint8_t>(text.begin(), text.begin() + 60), 0, Z_DEFAULT_STRATEGY},
                             {"fixed", std::vector<uint8_t>(text.begin(), text.begin() + 120), 6, Z_FIXED},
                             {"dynamic", text, 9, Z_DEFAULT_STRATEGY}};
    for (const Small& sm : smalls) {
        const std::vector<uint8_t> raw = deflate_raw(sm.plain, sm.level, sm.strategy, Z_NO_FLUSH);
        const uint32_t isize = (uint32_t)sm.plain.size();
        bz::Census one;
        std::vector<uint8_t> got;
        uint64_t steps = 0;
        const int32_t st0 = core_inflate(raw, isize, &got, &steps, &one);
        std::printf("small %s %zu %d stored %u fixed %u dynamic %u ", sm.name, raw.size(), (int)st0, one.stored, one.fixed, one.dynamic);
        for (uint8_t b : raw) std::printf("%02x", b);
        std::printf("\n");
        if (st0 != bz::kDone || got != sm.plain || raw.size() > 200) ++bad;
        for (int kind = 0; kind < 2; ++kind) {
            const size_t count = kind == 0 ? raw.size() * 8 : raw.size();
            for (size_t k = 0; k < count; ++k) {
                std::vector<uint8_t> m(raw);
                if (kind == 0) m[k >> 3] ^= (uint8_t)(1u << (k & 7));
                else m.resize(k);
                std::vector<uint8_t> want;
                const bool zok = zlib_inflate(m, isize, &want);
                const int32_t st = core_inflate(m, isize, &got, &steps, nullptr);
                const uint64_t budget = bz::step_budget((uint32_t)m.size(), isize);
                int equal = -1;
                if (st == bz::kDone && zok) equal = got == want ? 1 : 0;
                std::printf("mut %s %s %zu %d %llu %llu %d %d\n", sm.name, kind == 0 ? "flip" : "cut", k, (int)st, (unsigned long long)steps,
                            (unsigned long long)budget, (int)zok, equal);
                if (steps > budget || equal == 0) ++bad;
            }
        }
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
