"""baq_scenario.py -- TEST INFRASTRUCTURE ONLY: the scenario of the --ApplyBAQ tests (test_baq_cpu.py, test_baq_gpu.py).

A seeded genome of three sequences (a fourth is in the BAM header alone), a few hundred reads drawn from it, each over a
marker of its own so that the scan keeps it, and by name the smallest shapes at which the stage can go wrong.  Expected
values come from baq_ref.py and bam_ref.py, never from the code under test.
"""
import random

import bam_ref as br

PP = br.FPAIRED | br.FPROPER
# the header: chr3 is LONGER in the header than in the FASTA (a read can lie outside the sequence), chrX is not in the FASTA
REFS = [("chr1", 30000), ("chr2", 3000), ("chr3", 5000), ("chrX", 2000)]
FASTA_LEN = dict(chr1=30000, chr2=3000, chr3=3000)
LDS_KB = 32          # tunable baq_lds_kb of the GPU tests: 8192 bytes a record, so query lengths 16 and 17 straddle the tiers

OPTION_SETS = {
    "defaults": {},
    "redo": dict(incl_flags=16 | 64 | 1024),
    "cap_only": dict(incl_flags=1024, adjust_mq=40),
    "baq_only": dict(incl_flags=16 | 1024, adjust_mq=0),
    "cap_50": dict(adjust_mq=50),
    "illumina": dict(incl_flags=16 | 128 | 1024),
}


def full_opts(o):
    return dict(br.DEFAULT_OPTS, **o)


def make_genome(seed=11):
    rng = random.Random(seed)
    g = {name: "".join(rng.choice("ACGT") for _ in range(n)) for name, n in FASTA_LEN.items()}
    c2 = list(g["chr2"])
    c2[1500:1600] = "N" * 100                       # a span of all N
    c2[2000:2040] = list("acgtRYKMn" * 4 + "acgt")  # lower case and IUPAC codes
    g["chr2"] = "".join(c2)
    c1 = list(g["chr1"])
    c1[25000:25060] = list("CA" * 30)               # a repeat: an indel inside it has many equivalent placements
    g["chr1"] = "".join(c1)
    return g


def build(seed=5):
    """(records sorted, bed rows, genome, notes): notes[name] = (chr, pos1) of the marker under the named read"""
    rng = random.Random(seed)
    genome = make_genome()
    R, rows, at = [], [], {}

    def marker(case, c, p1):
        rows.append((c, p1, "A", "C"))
        at[case] = (c, p1)

    def read(name, tid, pos, cigar, sub=0.02, qual="rand", mark=None, **kw):
        chrom = REFS[tid][0]
        seq = genome.get(chrom, "")
        ops = br.rec("x", 0, 0, cigar, "")["cigar"]
        s, x = [], pos
        for op, n in ops:
            if op in "M=X":
                for i in range(n):
                    b = seq[x + i].upper() if x + i < len(seq) else rng.choice("ACGT")
                    if b not in "ACGT" or rng.random() < sub:
                        b = rng.choice("ACGT")
                    s.append(b)
                x += n
            elif op in "IS":
                s += [rng.choice("ACGT") for _ in range(n)]
            elif op in "DN":
                x += n
        n = len(s)
        q = None if qual is None else ([rng.randrange(15, 41) for _ in range(n)] if qual == "rand" else list(qual))
        r = br.rec(name, tid, pos, cigar, "".join(s), q, **kw)
        R.append(r)
        if mark is not False:
            marker(name, chrom, pos + 1 + (mark or 0))
        return r

    p = 500
    for n in (1, 2, 7, 8, 15, 16, 17, 100, 151):          # 16 and 17: one row under and one over the LDS budget at LDS_KB
        read("len%d" % n, 0, p, "%dM" % n)
        p += 400
    read("long5k", 0, 10000, "5000M", sub=0.01)             # the global tier
    read("del12", 0, 16000, "50M12D50M")                    # bw = |delta| + 3
    read("ins12", 0, 16400, "50M12I50M")
    read("soft_both", 0, 16800, "5S40M6S")
    read("hard_both", 0, 17200, "4H40M3H")
    read("hard_soft", 0, 17600, "3H4S40M5S2H")
    read("ins_in_repeat", 0, 24980, "40M2I38M", mark=30)
    read("del_in_repeat", 0, 24990, "30M2D40M", mark=20)
    read("pos0", 1, 0, "40M")                               # xb clamps
    read("past_end", 1, 2980, "40M")                        # runs past the sequence: xe is cut, the cap's walk ends
    read("outside", 2, 3500, "40M")                         # pos >= the FASTA's length: dropped
    read("n_op", 1, 300, "20M50N20M")
    read("no_qual", 1, 500, "40M", qual=None)
    read("unmapped_placed", 1, 700, "40M", flag=br.FUNMAP)
    bq = bytes(64 + (i % 5) for i in range(40))
    read("tag_bq", 1, 900, "40M")["aux"] = b"BQZ" + bq + b"\0"
    read("tag_zq", 1, 1000, "40M")["aux"] = b"NMC\x01ZQZ" + bq + b"\0"
    read("tag_both", 1, 1100, "40M")["aux"] = b"ZQZ" + bq + b"\0XSi\x05\0\0\0BQZ" + bytes(64 + (i % 3) for i in range(40)) + b"\0"
    read("ref_all_n", 1, 1520, "40M")
    read("iupac_ref", 1, 2000, "40M")
    read("query_all_n", 1, 1200, "40M")
    R[-1]["seq"] = "N" * 40
    read("no_fasta_seq", 3, 100, "40M")
    read("high_qual", 1, 1300, "40M", qual=[0, 2, 41, 93, 255, 60, 13, 12] * 5)     # (also: the Illumina shift's edge at 31)
    # a read the cap drops: a dozen confident mismatches
    r = read("cap_drops", 2, 300, "100M", sub=0.0, qual=[35] * 100)
    s = list(r["seq"])
    for i in range(10, 100, 8):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1) % 4]
    r["seq"] = "".join(s)
    # ... and one it only lowers
    r = read("cap_lowers", 2, 600, "100M", sub=0.0, qual=[35] * 100, mapq=60)
    s = list(r["seq"])
    for i in (20, 60):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 2) % 4]
    r["seq"] = "".join(s)
    # an overlapping pair that disagrees at a marker: mate A has the better quality there but an insertion two bases
    # away, so BAQ takes its quality down and the winner changes
    at0 = 1000                                              # 0-based site on chr3
    g3 = genome["chr3"]
    for k, (pos, cigar, base, q, mate) in enumerate(((at0 - 30, "28M3I32M", "G", 38, at0 - 10), (at0 - 10, "60M", "T", 30, at0 - 30))):
        r = read("pair_baq", 2, pos, cigar, sub=0.0, qual=[38 if k == 0 else 30] * (63 if k == 0 else 60), mark=False,
                 flag=PP | (64 if k == 0 else 128 | br.FREVERSE), mtid=2, mpos=mate)
        s = list(r["seq"])
        qpos = (at0 - pos) + (3 if k == 0 else 0)
        alt = base if g3[at0] != base else "C"
        s[qpos] = alt
        r["seq"] = "".join(s)
    marker("pair_baq", "chr3", at0 + 1)
    # (the named sites, and the bases BAQ moves below min-BQ, are looked at in test_the_scenario_holds_its_cases)
    # a crowd of ordinary reads, some with indels: more than one wave, more than one batch
    for i in range(160):
        tid = i % 3
        n = 30 + (i * 7) % 90
        pos = 2000 + i * 13 if tid == 0 else (2100 + i * 5 if tid == 1 else 1500 + i * 9)
        if pos + n + 5 >= FASTA_LEN[REFS[tid][0]]:
            continue
        cigar = "%dM" % n
        if i % 5 == 1:
            cigar = "%dM%dI%dM" % (n // 2, 1 + i % 3, n - n // 2 - 1 - i % 3)
        elif i % 5 == 3:
            cigar = "%dM%dD%dM" % (n // 3, 1 + i % 4, n - n // 3)
        read("crowd%d" % i, tid, pos, cigar, sub=0.03, mark=n // 2, flag=br.FREVERSE if i % 2 else 0, mapq=20 + i % 41)
    R.sort(key=lambda r: (r["tid"], r["pos"]))
    return R, rows, genome, at


def write_panel(pre, rows):
    with open(pre + ".bed", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(pre + ".UD", "w") as fh:
        for i in range(len(rows)):
            fh.write("%g %g\n" % (0.01 * (i % 7 - 3), 0.02 * (i % 5 - 2)))
    with open(pre + ".mu", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s:%d_%s/%s 0.4\n" % (c, p, r, a))


def fasta_genome(genome):
    """the FASTA's sequences: what the test genome holds, in the header's order"""
    return {name: genome[name] for name, _ in REFS if name in genome}


def write_all(d):
    """the scenario's files in directory d and a cache of the restatement: dict(recs, rows, genome, at, pre, bam, fasta,
    names, adjusted(option-set name) -> per record baq_ref.adjust_record, want(option-set name, **more) -> pileup_ref of the
    transformed records)"""
    import os

    import baq_ref
    recs, rows, genome, at = build()
    pre = os.path.join(d, "panel")
    write_panel(pre, rows)
    bam = os.path.join(d, "s.bam")
    br.write_indexed_bam(bam, REFS, recs, block_payload=300)
    fasta = os.path.join(d, "genome.fa")
    fg = fasta_genome(genome)
    baq_ref.write_fasta(fasta, fg)
    names = [n for n, _ in REFS]
    cache, piles = {}, {}

    def adjusted(name):
        if name not in cache:
            opts = full_opts(OPTION_SETS[name])
            cache[name] = [baq_ref.adjust_record(r, fg, names, opts) for r in recs]
        return cache[name]

    def want(name, **more):
        key = (name, tuple(sorted(more.items())))
        if key not in piles:
            opts = dict(OPTION_SETS[name], **more)
            out = []
            for r, a in zip(recs, adjusted(name)):
                if a["mapq"] < 0:
                    continue
                t = dict(r)
                t["qual"], t["mapq"] = a["qual"], a["mapq"]
                out.append(t)
            piles[key] = br.pileup_ref(out, REFS, rows, opts)
        return piles[key]

    return dict(recs=recs, rows=rows, genome=genome, at=at, pre=pre, bam=bam, fasta=fasta, names=names, adjusted=adjusted, want=want,
                dir=d)
