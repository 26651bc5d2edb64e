"""bam_ref.py -- TEST INFRASTRUCTURE ONLY: the test side of the built-in BAM reader.

`struct` and `zlib` only.  A writer of BAM files whose BGZF blocks are so small that records straddle them, a writer of
the .bai index (bins and linear index of the SAM specification, section 5), a parser that returns every record's virtual
offset, and `pileup_ref`, a restatement of the reader's pileup rules straight from the list of records.  Expected values
of the tests come from here and from the reference's golden files, never from the code under test.

A record is a dict: name, tid, pos (0-based), mapq, flag, cigar [(op, length)] with op one of "MIDNSHP=X", seq (a
string over "=ACMGRSVTWYHKDBN", may be empty), qual (a list of ints, or None: 0xFF for every base), mtid, mpos, tlen.
"""
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"

_NT16_CODE = bytes(NT16.index(chr(c)) if chr(c) in NT16 else 15 for c in range(256))

FPAIRED, FPROPER, FUNMAP, FMUNMAP, FREVERSE, FSECONDARY, FQCFAIL, FDUP = 1, 2, 4, 8, 16, 256, 512, 1024

# the reference's defaults (main.cpp:81-96); incl_flags is its mplp.flag: bit 16 BAQ (not applied here), bit 1024 overlaps
DEFAULT_OPTS = dict(min_bq=13, min_mq=2, adjust_mq=40, max_depth=8000, no_orphans=0, incl_flags=16 | 1024,
                    excl_flags=FUNMAP | FSECONDARY | FQCFAIL | FDUP)


def rec(name, tid, pos, cigar, seq, qual=None, flag=0, mapq=60, mtid=-1, mpos=-1, tlen=0):
    ops = []
    num = ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            ops.append((ch, int(num)))
            num = ""
    return dict(name=name, tid=tid, pos=pos, mapq=mapq, flag=flag, cigar=ops, seq=seq, qual=qual, mtid=mtid, mpos=mpos,
                tlen=tlen)


def ref_length(cigar):
    return sum(n for op, n in cigar if op in "MDN=X")


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def record_end(r):
    """exclusive 0-based end on the reference, as the index sees the record"""
    n = ref_length(r["cigar"])
    return r["pos"] + (n if n > 0 else 1)


def encode_record(r):
    name = r["name"].encode() + b"\0"
    seq = r["seq"]
    l_seq = len(seq)
    codes = seq.encode().translate(_NT16_CODE) + b"\0"
    packed = bytes(a << 4 | b for a, b in zip(codes[0:l_seq:2], codes[1:l_seq + 1:2]))
    assert len(packed) == (l_seq + 1) // 2 and all(ch in NT16 for ch in set(seq))
    qual = bytes([0xFF] * l_seq) if r["qual"] is None else bytes(r["qual"])
    assert len(qual) == l_seq
    cig = b"".join(struct.pack("<I", (n << 4) | CIGAR_OPS.index(op)) for op, n in r["cigar"])
    beg = r["pos"] if r["pos"] >= 0 else 0
    body = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"], len(name), r["mapq"], reg2bin(beg, max(record_end(r), beg + 1)),
                       len(r["cigar"]), r["flag"], l_seq, r["mtid"], r["mpos"], r["tlen"])
    body += name + cig + bytes(packed) + qual + r.get("aux", b"")
    return struct.pack("<i", len(body)) + body


def bgzf_block(payload):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = co.compress(payload) + co.flush()
    bsize = 18 + len(data) + 8 - 1
    assert bsize < 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + data +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


BGZF_EOF = bgzf_block(b"")


def header_bytes(refs, text):
    t = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode() + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out


def write_bam(path, refs, records, block_payload=300, text=None, eof=True, encoded=None):
    """Writes the file and returns (voffsets, end_voffsets, blocks): per record the virtual offset of its first byte and
    of the byte behind it, and the list of (file offset, first stream offset, payload length) of the blocks.  The header
    gets blocks of its own, so the first record starts a block.  Records must be sorted by (tid, pos), tid -1 last.
    encoded: the records' bytes, where a test wants them different from what encode_record gives."""
    if text is None:
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    key = [(r["tid"] if r["tid"] >= 0 else 1 << 30, r["pos"]) for r in records]
    assert key == sorted(key), "records must be coordinate-sorted"
    head = header_bytes(refs, text)
    enc = [encode_record(r) for r in records] if encoded is None else list(encoded)
    body = b"".join(enc)
    payloads = [head[i:i + block_payload] for i in range(0, len(head), block_payload)]
    n_head = len(payloads)
    payloads += [body[i:i + block_payload] for i in range(0, len(body), block_payload)]
    blocks, out, stream = [], bytearray(), 0
    for i, p in enumerate(payloads):
        if i == n_head:
            stream = 0
        blocks.append((len(out), stream if i >= n_head else -1, len(p)))
        out += bgzf_block(p)
        stream += len(p)
    end_of_data = len(out)
    if eof:
        out += BGZF_EOF
    with open(path, "wb") as fh:
        fh.write(bytes(out))
    body_blocks = blocks[n_head:]

    def voff(o):
        # the block that holds stream offset o; the offset behind the last byte is the start of what follows
        lo, hi = 0, len(body_blocks)
        while lo < hi:
            mid = (lo + hi) // 2
            if body_blocks[mid][1] + body_blocks[mid][2] <= o:
                lo = mid + 1
            else:
                hi = mid
        if lo == len(body_blocks):
            return end_of_data << 16
        return (body_blocks[lo][0] << 16) | (o - body_blocks[lo][1])

    vo, ve, o = [], [], 0
    for e in enc:
        vo.append(voff(o))
        o += len(e)
        ve.append(voff(o))
    return vo, ve, blocks


def write_bai(path, n_ref, records, voffsets, end_voffsets, trailing=True):
    """The index of the SAM specification, section 5.2: per sequence the chunks of every bin (records that follow each
    other in a bin share a chunk) and the linear index of 16 kb windows, empty windows filled from the next one."""
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    last_bin = [None] * n_ref
    for r, vo, ve in zip(records, voffsets, end_voffsets):
        t = r["tid"]
        if t < 0 or r["pos"] < 0:
            continue
        beg, end = r["pos"], record_end(r)
        b = reg2bin(beg, end)
        chunks = bins[t].setdefault(b, [])
        if chunks and last_bin[t] == b and chunks[-1][1] == vo:
            chunks[-1][1] = ve
        else:
            chunks.append([vo, ve])
        last_bin[t] = b
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if w not in lin[t]:
                lin[t][w] = vo
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for t in range(n_ref):
        out += struct.pack("<i", len(bins[t]))
        for b in sorted(bins[t]):
            out += struct.pack("<Ii", b, len(bins[t][b]))
            for vo, ve in bins[t][b]:
                out += struct.pack("<QQ", vo, ve)
        n_intv = max(lin[t]) + 1 if lin[t] else 0
        iv = [lin[t].get(w, 0) for w in range(n_intv)]
        for w in range(n_intv - 2, -1, -1):
            if w not in lin[t]:
                iv[w] = iv[w + 1]
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in iv)
    if trailing:
        out += struct.pack("<Q", sum(1 for r in records if r["tid"] < 0))
    with open(path, "wb") as fh:
        fh.write(out)


def write_indexed_bam(path, refs, records, block_payload=300, text=None):
    vo, ve, blocks = write_bam(path, refs, records, block_payload, text)
    write_bai(path + ".bai", len(refs), records, vo, ve)
    return vo, ve, blocks


def parse_bam(path):
    """(refs, text, records): every record as a dict with its `voffset`."""
    data = open(path, "rb").read()
    stream, starts, off = bytearray(), [], 0           # starts: (stream offset, file offset) per block
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        bsize, x = None, off + 12
        while x < off + 12 + xlen:
            si, slen = data[x:x + 2], struct.unpack_from("<H", data, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        raw = zlib.decompress(data[off + 12 + xlen:off + bsize + 1 - 8], -15)
        crc, isize = struct.unpack_from("<II", data, off + bsize + 1 - 8)
        assert isize == len(raw) and crc == zlib.crc32(raw) & 0xffffffff
        starts.append((len(stream), off))
        stream += raw
        off += bsize + 1
    s = bytes(stream)

    def voff(o):
        k = max(i for i, (so, _) in enumerate(starts) if so <= o and (i + 1 == len(starts) or starts[i + 1][0] > o or
                                                                       starts[i + 1][0] == so))
        return (starts[k][1] << 16) | (o - starts[k][0])

    assert s[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", s, 4)[0]
    text = s[8:8 + l_text].decode()
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", s, o)[0]
    o += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", s, o)[0]
        name = s[o + 4:o + 4 + ln - 1].decode()
        refs.append((name, struct.unpack_from("<i", s, o + 4 + ln)[0]))
        o += 8 + ln
    records = []
    while o < len(s):
        bs = struct.unpack_from("<i", s, o)[0]
        tid, pos, lrn, mapq, _bin, ncig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", s, o + 4)
        p = o + 36
        name = s[p:p + lrn - 1].decode()
        p += lrn
        cigar = []
        for k in range(ncig):
            c = struct.unpack_from("<I", s, p + 4 * k)[0]
            cigar.append((CIGAR_OPS[c & 15], c >> 4))
        p += 4 * ncig
        seq = "".join(NT16[(s[p + (i >> 1)] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        p += (l_seq + 1) // 2
        qual = list(s[p:p + l_seq])
        records.append(dict(name=name, tid=tid, pos=pos, mapq=mapq, flag=flag, cigar=cigar, seq=seq, qual=qual, mtid=mtid,
                            mpos=mpos, tlen=tlen, voffset=voff(o)))
        o += 4 + bs
    return refs, text, records


# ------------------------------------------------------------------ the pileup rules, restated

def passes_read_filter(r, opts):
    """mplp_func's order (SimplePileupViewer.cpp:172-237), less BAQ and the mapQ cap"""
    if (r["flag"] & FUNMAP) or r["tid"] < 0:
        return False
    if r["flag"] & opts["excl_flags"]:
        return False
    if r["mapq"] < opts["min_mq"]:
        return False
    if opts["no_orphans"] and (r["flag"] & FPAIRED) and not (r["flag"] & FPROPER):
        return False
    return True


def covered(r, pos0):
    """None when the record does not span 0-based pos0, else (qpos, deleted): one walk of the CIGAR; under D or N qpos is
    the query offset at which the operation starts."""
    x, y = r["pos"], 0
    for op, n in r["cigar"]:
        if op in "M=X":
            if x <= pos0 < x + n:
                return y + (pos0 - x), False
            x += n
            y += n
        elif op in "DN":
            if x <= pos0 < x + n:
                return y, True
            x += n
        elif op in "IS":
            y += n
    return None


def site_entries(records, tid, pos1, opts):
    """the site's entries in file order: dicts with nib, q, rev, deleted, eligible, rec"""
    out = []
    for r in records:
        if r["tid"] != tid or not passes_read_filter(r, opts) or r["pos"] < 0:
            continue
        c = covered(r, pos1 - 1)
        if c is None:
            continue
        qpos, deleted = c
        have = qpos < len(r["seq"])
        q = (0xFF if r["qual"] is None else r["qual"][qpos]) if have else 0
        nib = NT16.index(r["seq"][qpos]) if have and not deleted else 15
        f = r["flag"]
        eligible = bool(f & FPAIRED) and bool(f & FPROPER) and not (f & FMUNMAP) and r["mtid"] == r["tid"] and not deleted
        out.append(dict(nib=nib, q=q, rev=bool(f & FREVERSE), deleted=deleted, eligible=eligible, rec=r))
    return out


def resolve_overlaps(entries):
    """returns the number of pairs that met"""
    pending, met = {}, 0
    for e in entries:
        if not e["eligible"]:
            continue
        name = e["rec"]["name"]
        if name in pending:
            a = pending.pop(name)
            met += 1
            if a["nib"] == e["nib"]:
                a["q"], e["q"] = min(a["q"] + e["q"], 200), 0
            elif a["q"] >= e["q"]:
                a["q"], e["q"] = int(0.8 * a["q"]), 0
            else:
                a["q"], e["q"] = 0, int(0.8 * e["q"])
        elif e["rec"]["mpos"] >= e["rec"]["pos"]:
            pending[name] = e
    return met


def site_strings(entries, ref_base, opts, counts=None):
    """(bases, quals) of a site from its entries in file order: depth cap, overlap rule, min-BQ, characters, the
    deletion quirk (a deleted read's quality stays in the list; the site stores the first len(bases) of them)"""
    if counts is not None and len(entries) > max(opts["max_depth"], 0):
        counts["capped_sites"] += 1
    entries = entries[:max(opts["max_depth"], 0)]
    if opts["incl_flags"] & 1024:
        met = resolve_overlaps(entries)
        if counts is not None:
            counts["pairs_resolved"] += met
    rn = NT16.index(ref_base.upper()) if ref_base.upper() in NT16 else 15
    bases, quals = [], []
    for e in entries:
        if e["q"] < opts["min_bq"]:
            continue
        quals.append(chr(min(e["q"] + 33, 126)))
        if e["deleted"]:
            continue
        if e["nib"] == 0 or e["nib"] == rn:
            c = "," if e["rev"] else "."
        else:
            c = NT16[e["nib"]]
            if e["rev"]:
                c = c.lower()
        bases.append(c)
    return "".join(bases), "".join(quals[:len(bases)])


def read_bed_rows(path):
    """(chr, pos1, ref, alt) per row: the third column is the position; first characters of the alleles"""
    rows = []
    for line in open(path):
        t = line.split()
        if len(t) >= 5:
            rows.append((t[0], int(t[2]), t[3][0], t[4][0]))
    return rows


def pileup_ref(records, refs, bed_rows, opts=None, num_marker=None, candidates=None):
    """What the reader must produce.  sites: {(chr, pos1): (bases, quals)} for every position some record that passes the
    read filters spans (possibly empty strings: indexed, depth 0); rows: per .bed row (the first num_marker) its
    (bases, quals), empty for an absent site, a position listed twice once per row, its last row's REF allele used;
    num_site (rows whose position is indexed), num_bases, avg_depth = num_bases / sites with a base; entries (records
    over positions after the read filters), pairs_resolved and capped_sites as vb2_bam_stats counts them.
    candidates (optional): {(chr, pos1): records in file order} as readgroup_ref._candidates makes it -- for every position
    at least the records whose reference span reaches it.  It only narrows what site_entries looks at, which still makes
    the exact decision; without it every record is tried at every position, minutes on a file of 100 000 reads."""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    tid_of = {}
    for t, (name, _) in enumerate(refs):
        tid_of.setdefault(name, t)
    ref_of = {}
    for c, p, ref, _ in bed_rows:
        ref_of[(c, p)] = ref
    sites, counts = {}, dict(pairs_resolved=0, capped_sites=0, entries=0)
    for (c, p), ref in ref_of.items():
        if c not in tid_of:
            continue
        ent = site_entries(records if candidates is None else candidates.get((c, p), []), tid_of[c], p, o)
        if ent:
            counts["entries"] += len(ent)
            sites[(c, p)] = site_strings(ent, ref, o, counts)
    M = len(bed_rows) if num_marker is None else num_marker
    rows = [sites.get((c, p), ("", "")) for c, p, _, _ in bed_rows[:M]]
    num_site = sum(1 for c, p, _, _ in bed_rows[:M] if (c, p) in sites)
    num_bases = sum(len(b) for b, _ in sites.values())
    eff = sum(1 for b, _ in sites.values() if b)
    return dict(sites=sites, rows=rows, num_site=num_site, num_bases=num_bases, avg_depth=num_bases / eff if eff else 0.0,
                **counts)


def pileup_text(bed_rows, sites):
    """<prefix>.Pileup as the writer prints it: .bed row order, indexed sites with a base only (a position listed twice
    twice), the REF allele of the position's last row"""
    ref_of = {}
    for c, p, ref, _ in bed_rows:
        ref_of[(c, p)] = ref
    out = []
    for c, p, _, _ in bed_rows:
        b, q = sites.get((c, p), ("", ""))
        if b:
            out.append("%s\t%d\t%s\t%d\t%s\t%s\n" % (c, p, ref_of[(c, p)], len(b), b, q))
    return "".join(out)


def records_from_pileup(lines, ref_of, tid_of, lengths=(1, 7, 30, 100)):
    """One read per parsed base of a text pileup (lines: (chr, pos1, bases, quals) as oracle/refio.py's parser leaves
    them): '.' and ',' carry the panel's REF allele of the position, letters themselves; lower case and ',' are reverse
    strand.  Read lengths and the marker's offset within the read vary; the other bases are N of quality 0.  A read
    reaches no other position of ref_of (it shrinks to one base where it would), and the reads of a site start in the
    order of its bases, so the site comes out of a coordinate-sorted file in the order it went in."""
    others = {}
    for c, p in ref_of:
        others.setdefault(c, []).append(p)
    recs, n = [], 0
    for c, p, bases, quals in lines:
        shapes = []
        for _ in bases:
            length = lengths[n % len(lengths)]
            offset = min((n * 3) % length, p - 1)
            lo, hi = p - offset, p - offset + length - 1                 # 1-based span of the read
            if any(lo <= x <= hi and x != p for x in others[c]):
                length, offset = 1, 0
            shapes.append((length, offset))
            n += 1
        shapes.sort(key=lambda s: -s[1])                                  # starts ascending in the order of the bases
        for (length, offset), b, q in zip(shapes, bases, quals):
            base = ref_of[(c, p)].upper() if b in ".," else b.upper()
            seq = "N" * offset + base + "N" * (length - offset - 1)
            qual = [0] * length
            qual[offset] = ord(q) - 33
            flag = FREVERSE if (b == "," or b.islower()) else 0
            recs.append(rec("r%d" % len(recs), tid_of[c], p - 1 - offset, "%dM" % length, seq, qual, flag=flag))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))           # (stable: the reads of a site keep their order)
    return recs
