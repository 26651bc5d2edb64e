// bgzf_inflate_core.h -- a DEFLATE decoder (RFC 1951) for the payload of one BGZF block, written once for host and device
// (DESIGN.md section 21).  Written from the specification: stored, fixed and dynamic blocks, any number of them, ending at the
// block marked final.  No preset dictionary: the window of a BGZF block is its own output, at most 65 536 bytes.
//
// A template over the byte source, the byte sink and the tables' storage, like tile_sched.h: the host build (the CPU check
// of tests/bgzf_inflate_check_main.cpp, the host-side BlockInflater of the tests) gives it plain pointers, the kernel
// (bgzf_inflate_kernels.hip) a global pointer, a window in LDS whose bulk moves the whole wave shares, and tables in LDS.
// No HIP header and no array in a local variable: what is indexed at run time lives in `Tables`.
//
//   Source:  uint8_t operator[](uint32_t i) const                        byte i of the payload, i < raw_len
//   Sink:    void put(uint32_t at, uint8_t b)                            one literal
//            void copy_back(uint32_t at, uint32_t dist, uint32_t len)    a match: out[at + i] = out[at - dist + i], i ascending
//                                                                        (dist < len repeats the last dist bytes)
//            void copy_in(uint32_t at, const Source&, uint32_t from, uint32_t len)    a stored block's bytes
//
// THE LOOP IS BOUNDED BY CONSTRUCTION.  Every step (one block header, one code-length symbol, one literal/length symbol)
// consumes at least one bit of the input, and no bit past raw_len is ever made up: a read beyond the payload ends the
// decode with kInputExhausted.  The steps are counted all the same and checked against step_budget(raw_len, isize); the
// inner loops run over a code's at most 15 bits or over bytes whose number was checked against isize before.
#ifndef VB2_BGZF_INFLATE_CORE_H_
#define VB2_BGZF_INFLATE_CORE_H_

#include <cstdint>

// (always inlined: on the device a pointer into the tables then keeps its address space, and nothing is called)
#if defined(__HIPCC__)
#define VB2_BGZF_HD __host__ __device__ __attribute__((always_inline))
#else
#define VB2_BGZF_HD __attribute__((always_inline))
#endif

namespace vb2 {
namespace bgzf {

enum : int32_t {
    kDone = 0,             // exactly isize bytes produced, no more than raw_len consumed
    kInputExhausted = 1,   // the payload ends inside a block
    kOutputOverrun = 2,    // the next literal, match or stored run would pass isize
    kReservedBlock = 3,    // block type 3
    kStoredLength = 4,     // a stored block's LEN and NLEN are not complements
    kCodeLengths = 5,      // over-subscribed code lengths, or a literal/length code without the end-of-block symbol
    kRepeat = 6,           // a repeat with nothing before it, or one that runs past HLIT + HDIST
    kSymbol = 7,           // no code of the tree matches, or length symbol 286/287, or distance symbol 30/31
    kDistance = 8,         // a distance beyond what has been produced
    kShortStream = 9,      // the final block ends before isize bytes
    kBudget = 10,          // more steps than step_budget() (cannot happen: see above; checked all the same)
    kBadJob = 11,          // the kernel's own: a job that points outside its buffers was not run
    kNotRun = 12           // the host's own: the block was never given to the decoder
};

constexpr uint32_t kMaxIsize = 65536;
// code lengths: 288 + 32 of the fixed trees; 19 of the code-length code with up to 286 + 30 behind them while a dynamic
// block's are being read
constexpr uint32_t kNumLit = 288, kNumDist = 32, kNumLens = 344;

VB2_BGZF_HD inline uint64_t step_budget(uint32_t raw_len, uint32_t isize) { return 8ull * raw_len + isize + 64; }

// What a decode indexes at run time (1 080 bytes; the kernel keeps it in LDS).  A tree is the canonical form of RFC 1951
// 3.2.2: how many codes each length has, and the symbols ordered by (length, symbol).
struct Tables {
    uint16_t lit_count[16], dist_count[16], offs[16];
    uint16_t lit_sym[kNumLit], dist_sym[kNumDist];
    uint8_t len[kNumLens];
};

// What the streams of a corpus exercised; the host build's counters (the device build never takes one).
struct Census {
    uint32_t stored = 0, fixed = 0, dynamic = 0, empty_stored_off_byte = 0;
    uint32_t longest_match = 0, largest_distance = 0, overlapping = 0;
    uint32_t rep16 = 0, rep17 = 0, rep18 = 0, one_code_dist = 0, empty_dist = 0;
};
#if defined(__HIP_DEVICE_COMPILE__)
#define VB2_BGZF_CENSUS(stmt)
#else
#define VB2_BGZF_CENSUS(stmt) do { if (census) { stmt; } } while (0)
#endif

namespace detail {

template <class Source> struct Bits {
    const Source& src;
    uint32_t raw_len, pos = 0, cnt = 0;
    uint64_t buf = 0;
    VB2_BGZF_HD Bits(const Source& s, uint32_t n) : src(s), raw_len(n) {}
    // More bits into buf, as far as the payload has them: four bytes at once where it can (four independent loads: one trip
    // to memory, not four), single bytes towards the payload's end.  Called with cnt < 16.
    VB2_BGZF_HD void refill()
    {
        if (raw_len - pos >= 4) {
            const uint32_t b0 = src[pos], b1 = src[pos + 1], b2 = src[pos + 2], b3 = src[pos + 3];
            buf |= (uint64_t)(b0 | (b1 << 8) | (b2 << 16) | (b3 << 24)) << cnt;
            cnt += 32;
            pos += 4;
            return;
        }
        while (cnt < 16 && pos < raw_len) {
            buf |= (uint64_t)src[pos++] << cnt;
            cnt += 8;
        }
    }
    // at least k <= 16 bits in buf, or false: the payload is over
    VB2_BGZF_HD bool need(uint32_t k)
    {
        if (cnt < k) refill();
        return cnt >= k;
    }
    VB2_BGZF_HD uint32_t take(uint32_t k)           // after need(k)
    {
        const uint32_t v = (uint32_t)buf & ((1u << k) - 1u);
        buf >>= k;
        cnt -= k;
        return v;
    }
    VB2_BGZF_HD void to_byte_boundary()
    {
        buf >>= (cnt & 7u);
        cnt -= (cnt & 7u);
    }
};

// count[] and sym[] of the n code lengths at len[0..n); false: over-subscribed
VB2_BGZF_HD inline bool build_tree(const uint8_t* len, uint32_t n, uint16_t* count, uint16_t* sym, uint16_t* offs)
{
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t i = 0; i < n; ++i) ++count[len[i]];
    int32_t left = 1;                                // codes still free at this length
    for (uint32_t l = 1; l < 16; ++l) {
        left = left * 2 - (int32_t)count[l];
        if (left < 0) return false;
    }
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (uint32_t i = 0; i < n; ++i)
        if (len[i]) sym[offs[len[i]]++] = (uint16_t)i;
    return true;
}

// One symbol: the code's bits come most significant first (RFC 1951 3.1.1).  The codes of length l are the count[l]
// consecutive values from first_l on, first_l = (first_(l-1) + count[l-1]) << 1 (3.2.2).  -1: input over; -2: no code matches.
// The bits are looked at in a register and consumed once the code's length is known, and the fifteen counts do not depend on
// them: on the device their reads leave together, and a symbol costs two trips to LDS (the counts, the symbol), not one per bit.
template <class Source> VB2_BGZF_HD inline int32_t decode_symbol(Bits<Source>& in, const uint16_t* count, const uint16_t* sym)
{
    if (in.cnt < 15) in.refill();
    const uint32_t avail = in.cnt, bits = (uint32_t)in.buf;
    uint32_t code = 0, first = 0, index = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t l = 1; l < 16; ++l) {
        if (l > avail) return -1;
        code = (code << 1) | ((bits >> (l - 1)) & 1u);
        const uint32_t c = count[l];
        if (code - first < c) {
            in.buf >>= l;
            in.cnt -= l;
            return (int32_t)sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
    }
    return -2;
}

VB2_BGZF_HD inline uint32_t length_base(uint32_t s)      // s = symbol - 257 in [0, 28]: RFC 1951 3.2.5
{
    if (s < 8) return 3 + s;
    if (s == 28) return 258;
    const uint32_t e = (s - 4) >> 2;                      // extra bits
    return 3 + ((4 + (s & 3u)) << e);
}
VB2_BGZF_HD inline uint32_t length_extra(uint32_t s) { return (s < 8 || s == 28) ? 0 : (s - 4) >> 2; }
VB2_BGZF_HD inline uint32_t dist_base(uint32_t s)        // s in [0, 29]
{
    if (s < 4) return 1 + s;
    const uint32_t e = (s - 2) >> 1;
    return 1 + ((2 + (s & 1u)) << e);
}
VB2_BGZF_HD inline uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s - 2) >> 1; }

// the order in which a dynamic block sends the lengths of the code-length code (3.2.7), packed five bits each
VB2_BGZF_HD inline uint32_t clen_order(uint32_t i)
{
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

}  // namespace detail

// Inflates src[0, raw_len) into the sink, which must hold isize bytes.  *steps (may be null) gets the number of steps.
template <class Source, class Sink>
VB2_BGZF_HD inline int32_t inflate(const Source& src, uint32_t raw_len, Sink& sink, uint32_t isize, Tables& t, uint64_t* steps = nullptr,
                                   Census* census = nullptr)
{
    using namespace detail;
    (void)census;
    Bits<Source> in(src, raw_len);
    const uint64_t budget = step_budget(raw_len, isize);
    uint64_t n_step = 0;
    uint32_t out = 0;
    int32_t status = kDone;
#define VB2_BGZF_FAIL(code) do { status = (code); goto done; } while (0)
#define VB2_BGZF_STEP() do { if (++n_step > budget) VB2_BGZF_FAIL(kBudget); } while (0)
    for (;;) {
        VB2_BGZF_STEP();
        if (!in.need(3)) VB2_BGZF_FAIL(kInputExhausted);
        const uint32_t final_block = in.take(1);
        const uint32_t type = in.take(2);
        if (type == 3) VB2_BGZF_FAIL(kReservedBlock);
        if (type == 0) {
            VB2_BGZF_CENSUS(++census->stored);
            const bool off_byte = (in.cnt & 7u) != 0;
            (void)off_byte;
            in.to_byte_boundary();
            if (!in.need(16)) VB2_BGZF_FAIL(kInputExhausted);
            const uint32_t len = in.take(16);
            if (!in.need(16)) VB2_BGZF_FAIL(kInputExhausted);
            const uint32_t nlen = in.take(16);
            if ((len ^ nlen) != 0xffffu) VB2_BGZF_FAIL(kStoredLength);
            VB2_BGZF_CENSUS(if (len == 0 && off_byte) ++census->empty_stored_off_byte);
            if (len > isize - out) VB2_BGZF_FAIL(kOutputOverrun);
            // (the bit buffer holds whole bytes only here: hand them back, then the run comes straight from the source)
            in.pos -= in.cnt >> 3;
            in.buf = 0;
            in.cnt = 0;
            if (len > raw_len - in.pos) VB2_BGZF_FAIL(kInputExhausted);
            if (len) sink.copy_in(out, src, in.pos, len);
            in.pos += len;
            out += len;
        } else {
            const uint16_t *lcount = t.lit_count, *lsym = t.lit_sym, *dcount = t.dist_count, *dsym = t.dist_sym;
            if (type == 1) {
                VB2_BGZF_CENSUS(++census->fixed);
                for (uint32_t i = 0; i < 288; ++i) t.len[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                for (uint32_t i = 0; i < 32; ++i) t.len[288 + i] = 5;
                (void)build_tree(t.len, 288, t.lit_count, t.lit_sym, t.offs);
                (void)build_tree(t.len + 288, 32, t.dist_count, t.dist_sym, t.offs);
            } else {
                VB2_BGZF_CENSUS(++census->dynamic);
                if (!in.need(14)) VB2_BGZF_FAIL(kInputExhausted);
                const uint32_t hlit = in.take(5) + 257, hdist = in.take(5) + 1, hclen = in.take(4) + 4;
                if (hlit > 286 || hdist > 30) VB2_BGZF_FAIL(kCodeLengths);
                for (uint32_t i = 0; i < 19; ++i) t.len[i] = 0;
                for (uint32_t i = 0; i < hclen; ++i) {
                    if (!in.need(3)) VB2_BGZF_FAIL(kInputExhausted);
                    t.len[clen_order(i)] = (uint8_t)in.take(3);
                }
                // the code-length code borrows the distance tree's arrays (19 symbols fit its 32)
                if (!build_tree(t.len, 19, t.dist_count, t.dist_sym, t.offs)) VB2_BGZF_FAIL(kCodeLengths);
                const uint32_t total = hlit + hdist;
                uint32_t got = 0;
                while (got < total) {
                    VB2_BGZF_STEP();
                    const int32_t s = decode_symbol(in, t.dist_count, t.dist_sym);
                    if (s == -1) VB2_BGZF_FAIL(kInputExhausted);
                    if (s < 0) VB2_BGZF_FAIL(kSymbol);
                    if (s < 16) {
                        t.len[19 + got++] = (uint8_t)s;         // (kept behind the 19 lengths of the code-length code)
                        continue;
                    }
                    uint32_t value = 0, rep;
                    if (s == 16) {
                        VB2_BGZF_CENSUS(++census->rep16);
                        if (got == 0) VB2_BGZF_FAIL(kRepeat);
                        value = t.len[19 + got - 1];
                        if (!in.need(2)) VB2_BGZF_FAIL(kInputExhausted);
                        rep = 3 + in.take(2);
                    } else if (s == 17) {
                        VB2_BGZF_CENSUS(++census->rep17);
                        if (!in.need(3)) VB2_BGZF_FAIL(kInputExhausted);
                        rep = 3 + in.take(3);
                    } else {
                        VB2_BGZF_CENSUS(++census->rep18);
                        if (!in.need(7)) VB2_BGZF_FAIL(kInputExhausted);
                        rep = 11 + in.take(7);
                    }
                    if (rep > total - got) VB2_BGZF_FAIL(kRepeat);
                    for (uint32_t k = 0; k < rep; ++k) t.len[19 + got++] = (uint8_t)value;
                }
                // the lengths move down over the code-length code's, which is done with
                for (uint32_t i = 0; i < total; ++i) t.len[i] = t.len[19 + i];
                if (t.len[256] == 0) VB2_BGZF_FAIL(kCodeLengths);
                if (!build_tree(t.len, hlit, t.lit_count, t.lit_sym, t.offs)) VB2_BGZF_FAIL(kCodeLengths);
                if (!build_tree(t.len + hlit, hdist, t.dist_count, t.dist_sym, t.offs)) VB2_BGZF_FAIL(kCodeLengths);
#if !defined(__HIP_DEVICE_COMPILE__)
                if (census) {
                    uint32_t used = 0;
                    for (uint32_t i = 0; i < hdist; ++i) used += t.len[hlit + i] != 0;
                    if (used == 1) ++census->one_code_dist;
                    if (used == 0) ++census->empty_dist;
                }
#endif
            }
            for (;;) {
                VB2_BGZF_STEP();
                const int32_t s = decode_symbol(in, lcount, lsym);
                if (s == -1) VB2_BGZF_FAIL(kInputExhausted);
                if (s < 0) VB2_BGZF_FAIL(kSymbol);
                if (s < 256) {
                    if (out >= isize) VB2_BGZF_FAIL(kOutputOverrun);
                    sink.put(out++, (uint8_t)s);
                    continue;
                }
                if (s == 256) break;
                if (s > 285) VB2_BGZF_FAIL(kSymbol);
                const uint32_t ls = (uint32_t)s - 257, le = length_extra(ls);
                if (!in.need(le)) VB2_BGZF_FAIL(kInputExhausted);
                const uint32_t len = length_base(ls) + in.take(le);
                const int32_t d = decode_symbol(in, dcount, dsym);
                if (d == -1) VB2_BGZF_FAIL(kInputExhausted);
                if (d < 0 || d > 29) VB2_BGZF_FAIL(kSymbol);
                const uint32_t de = dist_extra((uint32_t)d);
                if (!in.need(de)) VB2_BGZF_FAIL(kInputExhausted);
                const uint32_t dist = dist_base((uint32_t)d) + in.take(de);
                if (dist > out) VB2_BGZF_FAIL(kDistance);
                if (len > isize - out) VB2_BGZF_FAIL(kOutputOverrun);
                VB2_BGZF_CENSUS(if (len > census->longest_match) census->longest_match = len;
                                if (dist > census->largest_distance) census->largest_distance = dist;
                                if (dist < len) ++census->overlapping);
                sink.copy_back(out, dist, len);
                out += len;
            }
        }
        if (final_block) break;
    }
    if (out != isize) status = kShortStream;
done:
#undef VB2_BGZF_FAIL
#undef VB2_BGZF_STEP
    if (steps) *steps = n_step;
    return status;
}

// The host's source and sink: plain memory.
struct PtrSource {
    const uint8_t* p;
    VB2_BGZF_HD uint8_t operator[](uint32_t i) const { return p[i]; }
};
struct PtrSink {
    uint8_t* p;
    VB2_BGZF_HD void put(uint32_t at, uint8_t b) { p[at] = b; }
    VB2_BGZF_HD void copy_back(uint32_t at, uint32_t dist, uint32_t len)
    {
        for (uint32_t i = 0; i < len; ++i) p[at + i] = p[at - dist + i];
    }
    VB2_BGZF_HD void copy_in(uint32_t at, const PtrSource& s, uint32_t from, uint32_t len)
    {
        for (uint32_t i = 0; i < len; ++i) p[at + i] = s.p[from + i];
    }
};

}  // namespace bgzf
}  // namespace vb2

#endif
