"""baq_ref.py -- TEST INFRASTRUCTURE ONLY: a sequential restatement of --ApplyBAQ in plain Python.

Python floats are IEEE doubles and Python never contracts a*b+c, so the statements below, which follow the reference's
bundled samtools/kprobaln.c (kpa_glocal) and samtools/bam_md.c (bam_prob_realn_core, bam_cap_mapQ) in their order of
operations, give the reference's bits wherever the host's libm gives its `log` and `pow`.  The single-precision gap
parameters go through numpy.float32.  Records are bam_ref.py's dicts; `aux` tags BQ / ZQ are read from r["aux"].

tests/golden/baq/kpa_cases.json (recipe: tests/golden/make_baq_fixtures.py) holds what the reference's own compiled HMM
gives on seeded cases; test_baq_cpu.py holds this restatement and the library's host core to it.
"""
import math

import numpy as np

import bam_ref

EI = .25
EM = .33333333333
_F = np.float32
_D = float(_F(0.001))
_E = float(_F(0.1))
_ONE_2D = float(_F(1) - _F(0.001) - _F(0.001))
_ONE_E = float(_F(1) - _F(0.1))
_ONE_D = _F(1) - _F(0.001)
QUAL2PROB = [float(_F(math.pow(10, -i / 10.))) for i in range(256)]

REALIGNED, ALONE, TAG_APPLIED, NO_REFERENCE, OUTSIDE, CAP_DROPPED, NOT_ASKED = range(7)

NT16_INT = [4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4]


def nt16_of(ch):
    ch = ch.upper()
    return bam_ref.NT16.index(ch) if ch in bam_ref.NT16 else 15


def quality_of(z):
    return int(-4.343 * math.log(z) + .499)


def _set_u(b, i, k):
    x = i - b
    x = x if x > 0 else 0
    return (k - x + 1) * 3


_MEMO = {}


def kpa_glocal(ref, query, iqual, conf_bw):
    """ref, query: codes 0..4; iqual: qualities.  Returns (state, q, undefined_rows).  (Memoised: the tests' option sets
    mostly ask the same alignments again, and a 5 kb read takes a second here.)"""
    key = (bytes(ref), bytes(query), bytes(iqual), conf_bw)
    if key not in _MEMO:
        _MEMO[key] = _kpa_glocal(ref, query, iqual, conf_bw)
    st, q, u = _MEMO[key]
    return list(st), list(q), u


def _kpa_glocal(ref, query, iqual, conf_bw):
    l_ref, l_query = len(ref), len(query)
    state = [0] * l_query
    q = [0] * l_query
    if l_ref <= 0 or l_query <= 0:
        return state, q, 0
    bw = max(l_ref, l_query)
    if bw > conf_bw:
        bw = conf_bw
    if bw < abs(l_ref - l_query):
        bw = abs(l_ref - l_query)
    bw2 = bw * 2 + 1
    W = bw2 * 3 + 6
    f = [[0.] * W for _ in range(l_query + 1)]
    s = [0.] * (l_query + 2)
    qual = [QUAL2PROB[x] for x in iqual]
    sM = sI = 1. / (2 * l_query + 2)
    m = [0.] * 9
    m[0] = _ONE_2D * (1 - sM)
    m[1] = m[2] = _D * (1 - sM)
    m[3] = _ONE_E * (1 - sI)
    m[4] = _E * (1 - sI)
    m[6] = _ONE_E
    m[8] = _E
    bM = float(_ONE_D / _F(l_ref))
    bI = float(_F(0.001) / _F(l_ref))

    def emit(rk, qy, ql):
        if rk > 3 or qy > 3:
            return 1.
        return 1. - ql if rk == qy else ql * EM

    f[0][_set_u(bw, 0, 0)] = s[0] = 1.
    fi = f[1]
    end = l_ref if l_ref < bw + 1 else bw + 1
    tot = 0.
    for k in range(1, end + 1):
        e = emit(ref[k - 1], query[0], qual[0])
        u = _set_u(bw, 1, k)
        fi[u] = e * bM
        fi[u + 1] = EI * bI
        tot += fi[u] + fi[u + 1]
    s[1] = tot
    for k in range(_set_u(bw, 1, 1), _set_u(bw, 1, end) + 3):
        fi[k] /= tot
    for i in range(2, l_query + 1):
        fi, fi1 = f[i], f[i - 1]
        qli, qyi = qual[i - 1], query[i - 1]
        beg, end = max(1, i - bw), min(l_ref, i + bw)
        tot = 0.
        for k in range(beg, end + 1):
            e = emit(ref[k - 1], qyi, qli)
            u, v11, v10, v01 = _set_u(bw, i, k), _set_u(bw, i - 1, k - 1), _set_u(bw, i - 1, k), _set_u(bw, i, k - 1)
            fi[u] = e * (m[0] * fi1[v11] + m[3] * fi1[v11 + 1] + m[6] * fi1[v11 + 2])
            fi[u + 1] = EI * (m[1] * fi1[v10] + m[4] * fi1[v10 + 1])
            fi[u + 2] = m[2] * fi[v01] + m[8] * fi[v01 + 2]
            tot += fi[u] + fi[u + 1] + fi[u + 2]
        s[i] = tot
        r = 1. / tot if tot != 0 else math.inf
        for k in range(_set_u(bw, i, beg), _set_u(bw, i, end) + 3):
            fi[k] *= r
    tot = 0.
    for k in range(1, l_ref + 1):
        u = _set_u(bw, l_query, k)
        if u < 3 or u >= bw2 * 3 + 3:
            continue
        tot += f[l_query][u] * sM + f[l_query][u + 1] * sI
    s[l_query + 1] = tot
    # backward
    b = [[0.] * W for _ in range(l_query + 1)]
    bi = b[l_query]

    def div(a, c):
        if c == 0:
            return math.nan if a == 0 or a != a else math.copysign(math.inf, a)
        return a / c
    for k in range(1, l_ref + 1):
        u = _set_u(bw, l_query, k)
        if u < 3 or u >= bw2 * 3 + 3:
            continue
        bi[u] = div(div(sM, s[l_query]), s[l_query + 1])
        bi[u + 1] = div(div(sI, s[l_query]), s[l_query + 1])
    for i in range(l_query - 1, 0, -1):
        bi, bi1 = b[i], b[i + 1]
        y = 1. if i > 1 else 0.
        qli1, qyi1 = qual[i], query[i]
        beg, end = max(1, i - bw), min(l_ref, i + bw)
        for k in range(end, beg - 1, -1):
            u, v11, v10, v01 = _set_u(bw, i, k), _set_u(bw, i + 1, k + 1), _set_u(bw, i + 1, k), _set_u(bw, i, k + 1)
            e = (0. if k >= l_ref else emit(ref[k], qyi1, qli1)) * bi1[v11]
            bi[u] = e * m[0] + EI * m[1] * bi1[v10 + 1] + m[2] * bi[v01 + 2]
            bi[u + 1] = e * m[3] + EI * m[4] * bi1[v10 + 1]
            bi[u + 2] = (e * m[6] + m[8] * bi[v01 + 2]) * y
        yy = div(1., s[i])
        for k in range(_set_u(bw, i, beg), _set_u(bw, i, end) + 3):
            bi[k] *= yy
    undefined = 0
    for i in range(1, l_query + 1):
        fi, bi = f[i], b[i]
        tot, mx, max_k = 0., 0., -1
        beg, end = max(1, i - bw), min(l_ref, i + bw)
        for k in range(beg, end + 1):
            u = _set_u(bw, i, k)
            z = fi[u] * bi[u]
            if z > mx:
                mx, max_k = z, (k - 1) << 2 | 0
            tot += z
            z = fi[u + 1] * bi[u + 1]
            if z > mx:
                mx, max_k = z, (k - 1) << 2 | 1
            tot += z
        state[i - 1] = max_k
        if tot > 0. and 1. - mx / tot > 0.:
            kq = quality_of(1. - mx / tot)
            q[i - 1] = 99 if kq > 100 else kq
        else:                       # the reference converts a NaN or an infinity to int here: outside the contract
            undefined += 1
            q[i - 1] = 0
    return state, q, undefined


# ---- the wrapper and the cap over bam_ref records ----
def find_tags(r):
    """BQ / ZQ strings (bytes) of r["aux"], or None"""
    aux = r.get("aux", b"")
    p, out = 0, {}
    width = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while len(aux) - p >= 3:
        tag, ty = aux[p:p + 2].decode("latin1"), chr(aux[p + 2])
        p += 3
        if ty in "ZH":
            e = aux.index(b"\0", p)
            if ty == "Z" and tag in ("BQ", "ZQ") and tag not in out:
                out[tag] = aux[p:e]
            p = e + 1
        elif ty == "B":
            w = width[chr(aux[p])]
            n = int.from_bytes(aux[p + 1:p + 5], "little")
            p += 5 + n * w
        else:
            p += width[ty]
    return out.get("BQ"), out.get("ZQ")


def shifted(quals, illumina):
    return [(x - 31 if x > 31 else 0) for x in quals] if illumina else list(quals)


def record_quals(r):
    return [0xFF] * len(r["seq"]) if r["qual"] is None else list(r["qual"])


def prob_realn(r, qual, ref_codes, ref_len, redo):
    """bam_prob_realn_core with flag 3 (7 with redo) on qual (already shifted), in place.  ref_codes(i) -> nt16 code of
    position i.  Returns (outcome, undefined_rows, (l_ref, bw) or None)."""
    l_qseq = len(r["seq"])
    if (r["flag"] & 4) or l_qseq == 0 or qual[0] == 0xFF:
        return ALONE, 0, None
    bq, zq = find_tags(r)
    if bq is not None and len(bq) < l_qseq:
        bq = None
    if bq is not None and redo:
        bq = None
    if bq is not None and zq is not None:
        zq = None
    if zq is not None:
        return ALONE, 0, None
    if bq is not None:
        for i in range(l_qseq):
            qual[i] = 0 if qual[i] + 64 < bq[i] else qual[i] - (bq[i] - 64)
        return TAG_APPLIED, 0, None
    x, y = r["pos"], 0
    yb = ye = xb = xe = -1
    for op, l in r["cigar"]:
        if op in "M=X":
            if yb < 0:
                yb = y
            if xb < 0:
                xb = x
            ye, xe = y + l, x + l
            x += l
            y += l
        elif op in "SI":
            y += l
        elif op == "D":
            x += l
        elif op == "N":
            return ALONE, 0, None
    if y != l_qseq:
        return ALONE, 0, None
    bw = 7
    if abs((xe - xb) - (ye - yb)) > bw:
        bw = abs((xe - xb) - (ye - yb)) + 3
    xb -= yb + bw // 2
    if xb < 0:
        xb = 0
    xe += l_qseq - ye + bw // 2
    if xe - xb - l_qseq > bw:
        xb += int((xe - xb - l_qseq - bw) / 2)
        xe -= int((xe - xb - l_qseq - bw) / 2)
    xe = min(xe, ref_len)
    xe = max(xe, xb)
    s = [NT16_INT[nt16_of(c)] for c in r["seq"]]
    rr = [NT16_INT[ref_codes(i)] for i in range(xb, xe)]
    state, q, undefined = kpa_glocal(rr, s, qual, bw)
    bqv = list(qual)
    x, y = r["pos"], 0
    for op, l in r["cigar"]:
        if op in "M=X":
            for i in range(y, y + l):
                bqv[i] = 0 if (state[i] & 3) != 0 or state[i] >> 2 != x - xb + (i - y) else q[i]
            if l > 0:
                left = [0] * l
                rght = [0] * l
                left[0] = bqv[y]
                for i in range(1, l):
                    left[i] = max(bqv[y + i], left[i - 1])
                rght[l - 1] = bqv[y + l - 1]
                for i in range(l - 2, -1, -1):
                    rght[i] = max(bqv[y + i], rght[i + 1])
                for i in range(l):
                    bqv[y + i] = min(left[i], rght[i])
            x += l
            y += l
        elif op in "SI":
            y += l
        elif op == "D":
            x += l
    for i in range(l_qseq):
        t = 64 + (0 if qual[i] <= bqv[i] else qual[i] - bqv[i])
        qual[i] = (qual[i] - (t - 64)) & 0xFF
    return REALIGNED, undefined, (xe - xb, bw)


def cap_walk(r, qual, ref_codes, ref_len):
    mm = q = ln = clip_q = 0
    x, y = r["pos"], 0
    seq = r["seq"]
    for op, l in r["cigar"]:
        if op in "M=X":
            j = 0
            while j < l:
                z = y + j
                if x + j >= ref_len or z >= len(seq):
                    break
                c1, c2 = nt16_of(seq[z]), ref_codes(x + j)
                if c2 != 15 and c1 != 15 and qual[z] >= 13:
                    ln += 1
                    if c1 and c1 != c2:
                        mm += 1
                        q += 33 if qual[z] > 33 else qual[z]
                j += 1
            if j < l:
                break
            x += l
            y += l
            ln += l
        elif op == "D":
            if l > 0 and x + l > ref_len:
                break
            x += l
        elif op == "S":
            clip_q += sum(qual[y:y + l])
            y += l
        elif op == "H":
            clip_q += 13 * l
        elif op == "I":
            y += l
        elif op == "N":
            x += l
    return [mm, q, ln, clip_q]


def cap_finish(cap4, thres):
    mm, q, ln, clip_q = cap4
    t = 1.
    for i in range(mm):
        t *= float(ln) / (i + 1)
    t = q - 4.343 * math.log(t) + clip_q / 5.
    if t > thres:
        return -1
    if t < 0:
        t = 0
    t = math.sqrt((thres - t) / thres) * thres
    return int(t + .499)


def adjust_record(r, genome, ref_names, opts):
    """mplp_func's three steps on one record.  genome: {name: sequence string} (a name it lacks = no reference).
    Returns dict(qual, mapq (-1 dropped), outcome, cap4, undefined, shape)."""
    incl, thres = opts["incl_flags"], opts["adjust_mq"]
    qual = shifted(record_quals(r), incl & 128)
    out = dict(qual=qual, mapq=r["mapq"], outcome=NOT_ASKED, cap4=[0, 0, 0, 0], undefined=0, shape=None)
    realn, cap_on = bool(incl & 16), thres > 10
    name = ref_names[r["tid"]] if 0 <= r["tid"] < len(ref_names) else None
    if name not in genome or not (realn or cap_on):
        out["outcome"] = NO_REFERENCE if (realn or cap_on) else NOT_ASKED
        return out
    seq = genome[name]
    ref_len = len(seq)
    if r["pos"] >= ref_len:
        out["outcome"], out["mapq"] = OUTSIDE, -1
        return out

    def ref_codes(i):
        return nt16_of(seq[i])
    if realn:
        out["outcome"], out["undefined"], out["shape"] = prob_realn(r, qual, ref_codes, ref_len, bool(incl & 64))
    if cap_on:
        out["cap4"] = cap_walk(r, qual, ref_codes, ref_len)
        c = cap_finish(out["cap4"], thres)
        if c < 0:
            out["mapq"], out["outcome"] = -1, CAP_DROPPED
        elif out["mapq"] > c:
            out["mapq"] = c
    return out


def transformed_records(records, genome, ref_names, opts):
    """the records as pileup_ref should see them under --ApplyBAQ: dropped reads gone, qualities and mapQ adjusted"""
    out = []
    for r in records:
        a = adjust_record(r, genome, ref_names, opts)
        if a["mapq"] < 0:
            continue
        t = dict(r)
        t["qual"] = a["qual"]
        t["mapq"] = a["mapq"]
        out.append(t)
    return out


def write_fasta(path, genome, width=60, names=None):
    """a plain FASTA and its .fai"""
    fai = []
    with open(path, "wb") as f:
        for name in (names or list(genome)):
            seq = genome[name]
            f.write((">%s\n" % name).encode())
            off = f.tell()
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width].encode() + b"\n")
            fai.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, width, width + 1))
    with open(path + ".fai", "w") as f:
        f.write("".join(fai))
