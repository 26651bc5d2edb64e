"""The test side's deflate streams and BGZF blocks for the device inflate: the corpus of
tests/bgzf_inflate_check_main.cpp restated with Python's zlib -- the same generator, contents, lengths, levels, strategies
and flushes --, the three streams zlib's deflate never writes, assembled by hand from RFC 1951, and the three small
streams whose mutilations the CPU check decides."""
import struct
import zlib

LENGTHS = (0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65280, 65536)
CONTENTS = ("zeros", "random", "twice32k", "period3", "bam")
LEVELS = (0, 1, 6, 9)
STRATEGIES = (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE))
FLUSHES = (("none", None), ("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH))

# the decoder's statuses (verifybamid_amd/csrc/bgzf_inflate_core.h)
DONE, INPUT_EXHAUSTED, OUTPUT_OVERRUN, RESERVED_BLOCK, STORED_LENGTH, CODE_LENGTHS, REPEAT, SYMBOL, DISTANCE, SHORT_STREAM, BUDGET = range(11)

_cache = {}


def lcg(seed, n, mask=0xFF):
    """n values of x <- (1103515245 x + 12345) mod 2^31, each x >> 16 (& mask)"""
    key = (seed, n, mask)
    if key not in _cache:
        out = bytearray(n)
        x = seed
        for i in range(n):
            x = (1103515245 * x + 12345) & 0x7FFFFFFF
            out[i] = (x >> 16) & mask
        _cache[key] = bytes(out)
    return _cache[key]


def content(c, n, bam_bytes):
    """content number c of CONTENTS, n bytes (the check program seeds its generator with 12345 + c)"""
    if c == 0:
        return bytes(n)
    if c == 1:
        return lcg(12345 + 1, n)
    if c == 2:
        first = lcg(12345 + 2, min(n, 32768))
        return (first + first)[:n] if n > 32768 else first
    if c == 3:
        return (b"abc" * (n // 3 + 1))[:n]
    return (bam_bytes * (n // len(bam_bytes) + 1))[:n]


def deflate_raw(plain, level, strategy, flush=None):
    """zlib's deflate in raw mode; flush: Z_SYNC_FLUSH / Z_FULL_FLUSH after the first half of the input"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out = b""
    half = len(plain) // 2 if flush is not None else 0
    if flush is not None:
        out += co.compress(plain[:half]) + co.flush(flush)
    return out + co.compress(plain[half:]) + co.flush(zlib.Z_FINISH)


def corpus(bam_bytes, lengths=LENGTHS):
    """(name, raw deflate stream, plain bytes) over the whole cross product, then the hand-made streams"""
    for c, cname in enumerate(CONTENTS):
        for n in lengths:
            plain = content(c, n, bam_bytes)
            for level in LEVELS:
                for sname, strategy in STRATEGIES:
                    for fname, flush in FLUSHES:
                        yield "%s/%d/%d/%s/%s" % (cname, n, level, sname, fname), deflate_raw(plain, level, strategy, flush), plain
    for name, raw, plain in handmade():
        yield name, raw, plain


def bgzf_wrap(raw, plain=None, isize=None, crc=None):
    """One BGZF block around a raw deflate stream (SAMv1 4.1).  None when the block would pass 65 536 bytes."""
    if isize is None:
        isize = len(plain)
    if crc is None:
        crc = zlib.crc32(plain) & 0xFFFFFFFF if plain is not None else 0
    size = 18 + len(raw) + 8
    if size > 65536 or isize > 65536:
        return None
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, size - 1) + raw +
            struct.pack("<II", crc, isize))


# ---- streams zlib's deflate never writes (RFC 1951 by hand) ----

class BitWriter:
    def __init__(self):
        self.bytes = bytearray()
        self.nbit = 0

    def bits(self, v, n):
        """n bits of v, least significant first"""
        for i in range(n):
            if self.nbit % 8 == 0:
                self.bytes.append(0)
            self.bytes[-1] |= ((v >> i) & 1) << (self.nbit % 8)
            self.nbit += 1

    def code(self, c, n):
        """a Huffman code: most significant bit first"""
        for i in reversed(range(n)):
            self.bits((c >> i) & 1, 1)

    def align(self):
        self.nbit = (self.nbit + 7) // 8 * 8


def canonical(lengths):
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    codes = [0] * len(lengths)
    for i, l in enumerate(lengths):
        if l:
            codes[i] = nxt[l]
            nxt[l] += 1
    return codes


_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_block(w, final, lit, dist, tokens):
    """tokens: (literal/length symbol, distance symbol or -1), none of them with extra bits.  The code-length code is
    complete whatever it carries: 0..15 in 5 bits, 16 and 17 in 3, 18 in 2."""
    cl = [5] * 19
    cl[16] = cl[17] = 3
    cl[18] = 2
    clc, lc, dc = canonical(cl), canonical(lit), canonical(dist)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit) - 257, 5)
    w.bits(len(dist) - 1, 5)
    w.bits(19 - 4, 4)
    for i in range(19):
        w.bits(cl[_ORDER[i]], 3)
    both = list(lit) + list(dist)
    i = 0
    while i < len(both):
        run = 1
        while i + run < len(both) and both[i + run] == both[i]:
            run += 1
        if both[i] == 0 and run >= 11:
            r = min(run, 138)
            w.code(clc[18], 2)
            w.bits(r - 11, 7)
            i += r
        elif both[i] == 0 and run >= 3:
            w.code(clc[17], 3)
            w.bits(run - 3, 3)
            i += run
        else:
            w.code(clc[both[i]], 5)
            i += 1
    for sym, dsym in tokens:
        w.code(lc[sym], lit[sym])
        if dsym >= 0:
            w.code(dc[dsym], dist[dsym])
    w.code(lc[256], lit[256])


def handmade():
    """zlib 1.2.11 keeps matches within 32 768 - 262 bytes and gives every distance tree at least two codes: a match at
    distance 32 768, a distance tree of one code and one of none are assembled here.  zlib's inflate accepts all three."""
    out = []
    plain = bytearray(lcg(777, 32768))
    w = BitWriter()
    w.bits(0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(32768, 16)
    w.bits(32768 ^ 0xFFFF, 16)
    w.bytes += plain
    w.nbit = len(w.bytes) * 8
    w.bits(1, 1)
    w.bits(1, 2)
    w.code(0xC0 + (285 - 280), 8)          # length 258
    w.code(29, 5)                          # distance 24 577 + 13 extra bits
    w.bits(8191, 13)
    w.code(0, 7)                           # end of block
    plain += plain[:258]
    out.append(("hand_dist32768", bytes(w.bytes), bytes(plain)))

    lit, dist = [0] * 286, [0] * 3
    lit[ord("a")] = lit[ord("b")] = lit[ord("c")] = 2
    lit[256] = lit[285] = 3
    dist[2] = 1
    w = BitWriter()
    dynamic_block(w, True, lit, dist, [(ord("a"), -1), (ord("b"), -1), (ord("c"), -1), (285, 2), (285, 2)])
    out.append(("hand_one_dist", bytes(w.bytes), (b"abc" * 200)[:3 + 2 * 258]))

    lit, dist = [0] * 257, [0]
    lit[ord("a")] = lit[ord("b")] = lit[ord("c")] = lit[256] = 2
    text = bytes(b"abc"[(i * i) % 3] for i in range(40))
    w = BitWriter()
    dynamic_block(w, True, lit, dist, [(b, -1) for b in text])
    out.append(("hand_empty_dist", bytes(w.bytes), text))
    return out


# ---- the three small streams and their mutilations ----

def small_streams():
    """name -> (raw, plain): one stored, one fixed and one dynamic block, each at most 200 bytes"""
    r = lcg(2024, 480, mask=15)
    text = bytes(b"AAAAAAAACCCCGGTN"[v] for v in r)
    return {"stored": (deflate_raw(text[:60], 0, zlib.Z_DEFAULT_STRATEGY), text[:60]),
            "fixed": (deflate_raw(text[:120], 6, zlib.Z_FIXED), text[:120]),
            "dynamic": (deflate_raw(text, 9, zlib.Z_DEFAULT_STRATEGY), text)}


def mutilate(raw, kind, index):
    if kind == "cut":
        return raw[:index]
    b = bytearray(raw)
    b[index >> 3] ^= 1 << (index & 7)
    return bytes(b)


# Twenty mutilated streams for which the CPU check (tests/test_bgzf_inflate_cpu.py, under ASan and UBSan) showed these
# non-zero statuses within the step budget: what the kernel is given as broken input, and nothing else.
MUTILATED = [
    ("stored", "cut", 0, INPUT_EXHAUSTED), ("stored", "flip", 8, STORED_LENGTH), ("stored", "flip", 2, SYMBOL),
    ("stored", "flip", 1, SHORT_STREAM),
    ("fixed", "flip", 596, INPUT_EXHAUSTED), ("fixed", "flip", 72, OUTPUT_OVERRUN), ("fixed", "flip", 2, RESERVED_BLOCK),
    ("fixed", "flip", 1, STORED_LENGTH), ("fixed", "flip", 454, SYMBOL), ("fixed", "flip", 11, DISTANCE),
    ("fixed", "flip", 19, SHORT_STREAM),
    ("dynamic", "flip", 1426, INPUT_EXHAUSTED), ("dynamic", "flip", 271, OUTPUT_OVERRUN), ("dynamic", "flip", 1, RESERVED_BLOCK),
    ("dynamic", "flip", 2, STORED_LENGTH), ("dynamic", "flip", 6, CODE_LENGTHS), ("dynamic", "flip", 12, REPEAT),
    ("dynamic", "flip", 14, SYMBOL), ("dynamic", "flip", 3, DISTANCE), ("dynamic", "flip", 145, SHORT_STREAM),
]
