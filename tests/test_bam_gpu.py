"""GPU tests of --BamFile through the built-in reader: host stage, bam_cover_kernel, the sort,
bam_overlap_kernel and bam_site_kernel, then everything downstream.

One synthetic BAM (tests/bam_ref.py's writer: blocks of 300 payload bytes) of fewer than 500 reads over fewer than 60
markers on three sequences holds every case by name; what the reader must produce comes from bam_ref.pileup_ref, computed
from the list of records, and from the reference's golden files -- never from the code under test.  Every test marked
gpu fails on a library in which --BamFile cannot succeed; the one unmarked test checks the scenario itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
from test_bam_batches_cpu import cut, var_bytes  # noqa: E402  (the restatement of the cutting rule)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
HAPMAP = os.path.join("hapmap", "hapmap_3.3.b37.dat")
REFS = [("chr1", 500000), ("chr2", 500000), ("chr3", 500000)]
P, PP = br.FPAIRED, br.FPAIRED | br.FPROPER


def _seq(n, start=0):
    return "".join("ACGT"[(start + i * 7 + i // 3) % 4] for i in range(n))


def _q(n, base=20):
    return [base + (i * 3) % 15 for i in range(n)]


def _pair(name, tid, pos_a, pos_b, n, base_a, base_b, qa, qb, at, flag=PP, mtid=None, third=None):
    """two mates of n bases that both span 0-based `at` with the given bases and qualities there"""
    out = []
    for k, (pos, base, q, mate) in enumerate(((pos_a, base_a, qa, pos_b), (pos_b, base_b, qb, pos_a))):
        s = list(_seq(n, pos))
        s[at - pos] = base
        qq = _q(n)
        qq[at - pos] = q
        out.append(br.rec(name, tid, pos, "%dM" % n, "".join(s), qq, flag=flag | (64 if k == 0 else 128 | br.FREVERSE),
                          mtid=tid if mtid is None else mtid, mpos=mate, tlen=0))
    if third is not None:
        pos, base, q = third
        s = list(_seq(n, pos))
        s[at - pos] = base
        qq = _q(n)
        qq[at - pos] = q
        out.append(br.rec(name, tid, pos, "%dM" % n, "".join(s), qq, flag=flag | 64 | 2048, mtid=tid, mpos=pos + 5))
    return out


def _scenario():
    """(records, bed rows, notes): notes maps a case to the (chr, pos1) it lives at"""
    R, rows, at = [], [], {}

    def marker(case, c, p, ref="A", alt="C"):
        rows.append((c, p, ref, alt))
        at[case] = (c, p)

    # -- first and last base of a read, forward and reverse
    marker("first_last", "chr1", 1000)
    R += [br.rec("first", 0, 999, "30M", _seq(30, 1), _q(30)), br.rec("last", 0, 970, "30M", _seq(30, 2), _q(30), flag=br.FREVERSE),
          br.rec("just_behind", 0, 1000, "30M", _seq(30, 3), _q(30)), br.rec("just_before", 0, 969, "30M", _seq(30, 0), _q(30))]
    # -- every CIGAR operation over a marker of its own (the marker is the 13th reference base of where the read lies)
    for i, (case, cigar, n) in enumerate([("S", "12S20M", 32), ("H", "12H20M", 20), ("I", "12M5I20M", 37), ("D", "10M5D20M", 30),
                                          ("N", "10M300N20M", 30), ("P", "12M3P20M", 32), ("EQ", "10=10X10=", 30), ("X", "12X18=", 30),
                                          ("S_tail", "20M12S", 32), ("I_then_D", "12M3I2D15M", 30), ("lead_I", "3I27M", 30)]):
        p0 = 2000 + 400 * i
        marker(case, "chr1", p0 + 13, ref="ACGT"[i % 4])
        R.append(br.rec("op_" + case, 0, p0, cigar, _seq(n, i), _q(n), flag=br.FREVERSE if i % 2 else 0))
        if case in ("I", "D", "N", "I_then_D"):           # a second marker two bases before: inside D and N too, before the I
            rows.append(("chr1", p0 + 11, "G", "T"))
        if case in ("S", "H"):                            # where the clipped bases would lie: they cover nothing
            marker(case + "_shadow", "chr1", p0 - 3)
    # -- a CIGAR of 40 operations and a 5 kb read over several markers
    ops40 = "".join("%d%s" % (2 + k % 3, "MIMDM=XMNM"[k % 10]) for k in range(40))
    n40 = sum(n for op, n in br.rec("x", 0, 0, ops40, "")["cigar"] if op in "MIS=X")
    R.append(br.rec("ops40", 0, 8000, ops40, _seq(n40, 2), _q(n40)))
    for k, off in enumerate((1, 7, 19, 33, 62)):
        marker("ops40_%d" % k, "chr1", 8000 + off, ref="ACGT"[k % 4])
    R.append(br.rec("long5k", 0, 20000, "5000M", _seq(5000, 1), _q(5000)))
    R.append(br.rec("long5k_r", 0, 20010, "2500M10D2490M", _seq(4990, 3), _q(4990), flag=br.FREVERSE))
    for k, off in enumerate((1, 385, 2515, 4999, 5000, 5009, 5011)):      # 2515: in long5k_r's deletion; 5011: behind both
        marker("long_%d" % k, "chr1", 20000 + off, ref="ACGT"[k % 4])
    # -- N bases, no bases at all (l_seq = 0), absent qualities (0xFF)
    marker("odd_bases", "chr2", 500, ref="N")
    R += [br.rec("enn", 1, 490, "20M", "N" * 20, _q(20, 30)), br.rec("enn_r", 1, 491, "20M", "N" * 20, _q(20, 30), flag=br.FREVERSE),
          br.rec("noseq", 1, 492, "20M", "", []), br.rec("noqual", 1, 493, "20M", _seq(20), None),
          br.rec("noqual_r", 1, 494, "20M", _seq(20, 1), None, flag=br.FREVERSE), br.rec("eq_base", 1, 495, "20M", "=" * 20, _q(20, 30))]
    # -- the read filters, one read each at a marker that only it covers ... and all of them at a shared marker
    marker("filters", "chr2", 1500)
    kinds = [("unmapped", br.FUNMAP, 60), ("secondary", br.FSECONDARY, 60), ("qcfail", br.FQCFAIL, 60), ("dup", br.FDUP, 60),
             ("mapq1", 0, 1), ("mapq2", 0, 2), ("orphan", P, 60), ("proper", PP, 60), ("plain", 0, 60)]
    for i, (case, flag, mq) in enumerate(kinds):
        R.append(br.rec("f_" + case, 1, 1480 + i, "40M", _seq(40, i), _q(40, 25), flag=flag, mapq=mq, mtid=1, mpos=1480 + i))
        marker("only_" + case, "chr2", 3000 + 100 * i)
        R.append(br.rec("o_" + case, 1, 2990 + 100 * i, "40M", _seq(40, i + 1), _q(40, 25), flag=flag, mapq=mq, mtid=1, mpos=2990 + 100 * i))
    # -- the --min-BQ edge, and a site that is indexed although it holds no base
    marker("bq_edge", "chr2", 6000)
    for i, q in enumerate((12, 13, 12, 14, 0, 13)):
        qq = _q(30, 30)
        qq[6000 - 1 - (5990 + i)] = q
        R.append(br.rec("bq%d" % i, 1, 5990 + i, "30M", _seq(30, i), qq, flag=br.FREVERSE if i == 3 else 0))
    marker("empty_site", "chr2", 7000)
    R += [br.rec("lowq", 1, 6990, "30M", _seq(30), [3] * 30), br.rec("gap", 1, 6980, "10M30D10M", _seq(20), _q(20, 30))]
    marker("absent_site", "chr2", 7500)
    marker("not_in_header", "chrZ", 7500)
    # -- a position the .bed lists twice (the later alleles win), next to each other and apart
    rows.append(("chr2", 8000, "A", "C"))
    at["dup_row"] = ("chr2", 8000)
    R += [br.rec("d%d" % i, 1, 7990 + i, "25M", ("G" if i % 2 else "A") * 25, _q(25, 30), flag=br.FREVERSE if i % 3 == 0 else 0)
          for i in range(6)]
    # -- overlapping mates
    cases = [("agree", "G", "G", 30, 25, PP, None, None), ("disagree", "G", "T", 30, 20, PP, None, None),
             ("disagree_late", "G", "T", 20, 30, PP, None, None), ("tie", "G", "T", 30, 30, PP, None, None),
             ("sum_above_200", "C", "C", 150, 120, PP, None, None), ("three", "G", "G", 30, 25, PP, None, ("G", 40)),
             ("mate_elsewhere", "G", "G", 30, 25, PP, 0, None), ("not_proper", "G", "T", 30, 20, P, None, None),
             ("agree_is_ref", "A", "A", 5, 9, PP, None, None)]
    for i, (case, ba, bb, qa, qb, flag, mtid, third) in enumerate(cases):
        c0 = 1000 + 300 * i
        marker("mates_" + case, "chr3", c0 + 1)
        R += _pair("m_" + case, 2, c0 - 40, c0 - 10, 60, ba, bb, qa, qb, c0, flag=flag, mtid=mtid,
                   third=None if third is None else (c0 - 5, third[0], third[1]))
        R.append(br.rec("single_" + case, 2, c0 - 20, "50M", _seq(50, i), _q(50, 30)))
    # a mate whose partner lies BEFORE it never waits; a deleted mate is not eligible
    marker("mates_behind", "chr3", 5001)
    R += [br.rec("mb", 2, 4980, "60M", _seq(60), _q(60, 30), flag=PP | 64, mtid=2, mpos=100),
          br.rec("mb", 2, 4990, "60M", _seq(60, 1), _q(60, 30), flag=PP | 128, mtid=2, mpos=4980)]
    marker("mates_deleted", "chr3", 5501)
    R += [br.rec("md", 2, 5480, "15M10D30M", _seq(45), _q(45, 30), flag=PP | 64, mtid=2, mpos=5490),
          br.rec("md", 2, 5490, "60M", _seq(60, 1), _q(60, 30), flag=PP | 128, mtid=2, mpos=5480)]
    # -- a site of 70 reads and one of 300, with mates, deletions and low qualities inside
    for case, c0, depth in (("deep70", 10000, 70), ("deep300", 20000, 300)):
        marker(case, "chr3", c0 + 1, ref="T")
        for i in range(depth):
            pos = c0 - 90 + (i * 88) // depth                       # ascending: file order is i
            name, flag, mpos = "%s_%d" % (case, i), 0, -1
            if i % 7 == 3 and i + 2 < depth:                        # pairs (i, i + 2): the second is two records on
                name, flag, mpos = "%s_p%d" % (case, i), PP | 64, c0 - 90 + ((i + 2) * 88) // depth
            if i % 7 == 5 and i >= 2:
                name, flag, mpos = "%s_p%d" % (case, i - 2), PP | 128 | br.FREVERSE, c0 - 90 + ((i - 2) * 88) // depth
            cigar = "100M" if i % 11 else "%dM4D%dM" % (c0 - pos - 1, 100 - (c0 - pos - 1))
            qq = _q(100, 18 + i % 9)
            if i % 13 == 0:
                qq[c0 - pos] = 5
            R.append(br.rec(name, 2, pos, cigar, _seq(100, i), qq, flag=flag | (br.FREVERSE if i % 5 == 0 else 0), mtid=2, mpos=mpos))
    R.sort(key=lambda r: (r["tid"], r["pos"]))
    # the duplicated position's second row goes last: its alleles are the ones that count
    rows.append(("chr2", 8000, "G", "T"))
    return R, rows, at


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam")
    recs, rows, at = _scenario()
    assert len(recs) <= 500 and len(set((c, p) for c, p, _, _ in rows)) <= 60
    pre = str(d / "panel")
    with open(pre + ".bed", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(pre + ".UD", "w") as fh:
        for i in range(len(rows)):
            fh.write("%g %g\n" % (0.01 * (i % 7 - 3), 0.02 * (i % 5 - 2)))
    with open(pre + ".mu", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s:%d_%s/%s 0.4\n" % (c, p, r, a))
    bam = str(d / "s.bam")
    vo, _, _ = br.write_indexed_bam(bam, REFS, recs, block_payload=300)
    cache = {}

    def want(**opts):
        key = tuple(sorted(opts.items()))
        if key not in cache:
            cache[key] = br.pileup_ref(recs, REFS, rows, opts)
        return cache[key]

    return dict(recs=recs, rows=rows, at=at, pre=pre, bam=bam, want=want, dir=str(d), vo=vo)


def _same(got, want, rows):
    """pools, per-marker offsets, the site set, numBases and avgDepth: byte for byte"""
    off = got["read_off"]
    assert len(off) == len(rows) + 1
    for i, (c, p, _, _) in enumerate(rows):
        b, q = got["bases"][off[i]:off[i + 1]].decode("latin-1"), got["quals"][off[i]:off[i + 1]].decode("latin-1")
        assert (b, q) == want["rows"][i], ("%s:%d" % (c, p), b, q, want["rows"][i])
    assert got["num_site"] == want["num_site"]
    assert got["num_bases"] == want["num_bases"]
    assert got["avg_depth"] == want["avg_depth"]


def test_the_scenario_holds_its_cases(scenario):
    """The restatement's own answers at the named sites: the cases are really in the file (no device involved)."""
    w, at = scenario["want"]()["sites"], scenario["at"]
    assert len(w[at["first_last"]][0]) == 2                                   # "just_behind" and "just_before" miss it
    for case in ("S", "H"):
        assert at[case + "_shadow"] not in w and len(w[at[case]][0]) == 1     # a clipped base covers nothing
    assert w[at["D"]] == ("", "") and w[at["N"]] == ("", "")                  # deleted: a quality, no base: nothing stored
    assert len(w[at["I"]][0]) == 1 and len(w[at["P"]][0]) == 1 and len(w[at["EQ"]][0]) == 1
    # N on N is a match; the read without bases has quality 0 there and drops out; 0xFF qualities print as the cap
    assert w[at["odd_bases"]] == (".,Ac.", "KH~~K")
    assert scenario["want"](min_bq=0)["sites"][at["odd_bases"]] == (".,.Ac.", "KH!~~K")
    assert len(w[at["filters"]][0]) == 4                                      # mapq2, orphan, proper, plain
    for case in ("unmapped", "secondary", "qcfail", "dup", "mapq1"):
        assert at["only_" + case] not in w
    assert len(w[at["bq_edge"]][0]) == 3
    assert w[at["empty_site"]] == ("", "") and at["absent_site"] not in w and at["not_in_header"] not in w
    assert w[at["mates_agree"]][1].count(chr(33 + 55)) == 1 and len(w[at["mates_agree"]][0]) == 2
    assert chr(33 + 24) in w[at["mates_disagree"]][1] and chr(33 + 24) in w[at["mates_disagree_late"]][1] and chr(33 + 24) in w[at["mates_tie"]][1]
    assert "~" in w[at["mates_sum_above_200"]][1]
    assert len(w[at["mates_three"]][0]) == 3 and len(w[at["mates_mate_elsewhere"]][0]) == 3 and len(w[at["mates_not_proper"]][0]) == 3
    assert w[at["mates_agree_is_ref"]][0].count(".") + w[at["mates_agree_is_ref"]][0].count(",") == 1     # 5 + 9 = 14 passes, alone neither would
    assert 40 < len(w[at["deep70"]][0]) < 70 and 200 < len(w[at["deep300"]][0]) < 300
    w0 = scenario["want"](incl_flags=0)["sites"]
    assert len(w0[at["mates_agree"]][0]) == 3 and len(w0[at["deep300"]][0]) > len(w[at["deep300"]][0])


OPTION_SETS = {
    "defaults": {},
    "min_bq_0": dict(min_bq=0),
    "min_bq_12": dict(min_bq=12),
    "min_bq_14": dict(min_bq=14),
    "no_read_flag_excluded": dict(excl_flags=0),
    "only_dups_excluded": dict(excl_flags=br.FDUP),
    "min_mq_0": dict(min_mq=0),
    "min_mq_30": dict(min_mq=30),
    "no_orphans": dict(no_orphans=1),
    "no_overlap_rule": dict(incl_flags=0),
    "no_overlap_rule_min_bq_0": dict(incl_flags=16, min_bq=0),
    "max_depth_5": dict(max_depth=5),
    "max_depth_64_min_bq_0": dict(max_depth=64, min_bq=0),
}


@gpu
@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_pileup_is_the_restatements_byte_for_byte(scenario, name):
    opts = OPTION_SETS[name]
    want = scenario["want"](**opts)
    got = vb.api.load_bam(scenario["pre"], scenario["bam"], mpileup=opts or None)
    print(name, "sites %d bases %d" % (got["num_site"], got["num_bases"]), got["stats"])
    _same(got, want, scenario["rows"])
    st = got["stats"]
    assert st["sites"] == len(want["sites"]) and st["empty_sites"] == sum(1 for b, _ in want["sites"].values() if not b)
    assert st["records_kept"] <= len(scenario["recs"]) and st["long_cigar_skipped"] == 0
    assert (st["entries"], st["pairs_resolved"], st["capped_sites"]) == (want["entries"], want["pairs_resolved"], want["capped_sites"])
    if name == "max_depth_5":
        assert st["capped_sites"] >= 2
    if name == "defaults":
        assert st["capped_sites"] == 0 and st["pairs_resolved"] >= 40
    if name == "no_overlap_rule":
        assert st["pairs_resolved"] == 0


@gpu
def test_small_batches_give_the_same_bytes(scenario, tunable):
    one = vb.api.load_bam(scenario["pre"], scenario["bam"])
    assert one["stats"]["batches"] == 1
    tunable("bam_batch_kb", 8)
    many = vb.api.load_bam(scenario["pre"], scenario["bam"])
    assert many["stats"]["batches"] >= 3, many["stats"]
    assert many["bases"] == one["bases"] and many["quals"] == one["quals"] and list(many["read_off"]) == list(one["read_off"])
    assert many["stats"]["entries"] == one["stats"]["entries"] and many["stats"]["pairs_resolved"] == one["stats"]["pairs_resolved"]
    _same(many, scenario["want"](), scenario["rows"])


def _write_panel(pre, rows):
    with open(pre + ".bed", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(pre + ".UD", "w") as fh:
        for i in range(len(rows)):
            fh.write("%g %g\n" % (0.01 * (i % 7 - 3), 0.02 * (i % 5 - 2)))
    with open(pre + ".mu", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s:%d_%s/%s 0.4\n" % (c, p, r, a))


def _cut_of(bam, bed, recs, vo, kb):
    """(batch_bytes, batch_rec, batches) of the cutting rule over the records the host stage keeps, in its order, with
    the sizes of their variable parts taken from the record list"""
    rec_at = dict(zip(vo, recs))
    kept = [rec_at[int(v)] for v in vb.api.bam_scan(bam, bed)["voffsets"]]
    return cut(kb, [var_bytes(len(r["name"]) + 1, len(r["cigar"]), len(r["seq"])) for r in kept])


@gpu
def test_batches_are_the_cutting_rules(scenario, tunable, tmp_path):
    """stats["batches"] at 8 KiB on the scenario, and at 1 KiB on a dozen reads one of which is longer than 1 KiB: it
    raises the batch to its own size"""
    tunable("bam_batch_kb", 8)
    _, _, want = _cut_of(scenario["bam"], scenario["pre"] + ".bed", scenario["recs"], scenario["vo"], 8)
    got = vb.api.load_bam(scenario["pre"], scenario["bam"])
    print("8 KiB:", [(len(b), sum(b)) for b in want], got["stats"])
    assert len(want) >= 3 and got["stats"]["batches"] == len(want)
    recs = [br.rec("r%d" % i, 0, 100 + 10 * i, "50M", _seq(50, i), _q(50)) for i in range(11)]
    recs.append(br.rec("long", 0, 150, "1500M", _seq(1500, 1), _q(1500)))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    rows = [("chr1", p, "A", "C") for p in (130, 160, 190, 220, 1000)]
    pre, bam = str(tmp_path / "dozen"), str(tmp_path / "dozen.bam")
    _write_panel(pre, rows)
    vo, _, _ = br.write_indexed_bam(bam, REFS, recs, block_payload=300)
    tunable("bam_batch_kb", 1)
    batch_bytes, _, want = _cut_of(bam, pre + ".bed", recs, vo, 1)
    got = vb.api.load_bam(pre, bam)
    print("1 KiB:", batch_bytes, [(len(b), sum(b)) for b in want], got["stats"])
    assert batch_bytes == var_bytes(5, 1, 1500) > 1024 and sum(len(b) for b in want) == 12 == got["stats"]["records_kept"]
    assert len(want) >= 3 and got["stats"]["batches"] == len(want)
    _same(got, br.pileup_ref(recs, REFS, rows, {}), rows)


@gpu
def test_records_that_all_miss_the_panel_leave_nothing(scenario, tmp_path):
    """a dozen reads on chr1, one marker on chr3: no record is kept, no batch is cut, no entry and no site come back"""
    recs = [r for r in scenario["recs"] if r["tid"] == 0][:12]
    rows = [("chr3", 1000, "A", "C")]
    pre, bam = str(tmp_path / "miss"), str(tmp_path / "miss.bam")
    _write_panel(pre, rows)
    br.write_indexed_bam(bam, REFS, recs, block_payload=300)
    got = vb.api.load_bam(pre, bam)
    print(got["stats"])
    st = got["stats"]
    assert (st["records_kept"], st["batches"], st["entries"], st["sites"], st["empty_sites"]) == (0, 0, 0, 0, 0)
    assert (got["num_site"], got["num_bases"], got["avg_depth"]) == (0, 0, 0.0)
    assert got["bases"] == b"" and got["quals"] == b"" and list(got["read_off"]) == [0, 0]
    _same(got, br.pileup_ref(recs, REFS, rows, {}), rows)


@gpu
def test_batches_of_four_gib_are_refused(scenario, tunable):
    """bam_batch_kb one KiB above 0xfff00000 bytes: refused with its text and code before any staging buffer is asked for
    (the tunable's setter lets the value through); the next load is an ordinary one"""
    tunable("bam_batch_kb", 0xfff00000 // 1024 + 1)
    with pytest.raises(vb._abi.Vb2Error) as e:
        vb.api.load_bam(scenario["pre"], scenario["bam"])
    assert e.value.code == vb._abi.VB2_ERR_INVALID
    assert str(e.value).endswith("--BamFile: bam_batch_kb asks for batches of 4 GiB or more")
    tunable("bam_batch_kb", 65536)
    assert vb.api.load_bam(scenario["pre"], scenario["bam"])["stats"]["batches"] == 1


@gpu
def test_output_pileup_of_the_command_line(scenario, tmp_path):
    """--BamFile --OutputPileup: the site set as the writer prints it (an indexed site without a base and an absent one
    both leave no line; the position listed twice has two), and the NOTICEs about what is not applied."""
    out = str(tmp_path / "o")
    p = subprocess.run([EXE, "--SVDPrefix", scenario["pre"], "--BamFile", scenario["bam"], "--Reference", "unread.fa",
                        "--DisableSanityCheck", "--OutputPileup", "--Output", out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert open(out + ".Pileup").read() == br.pileup_text(scenario["rows"], scenario["want"]()["sites"])
    assert p.stderr.count("--incl-flags 1024 --adjust-MQ 0") == 2 and "REF allele" in p.stderr
    quiet = subprocess.run([EXE, "--SVDPrefix", scenario["pre"], "--BamFile", scenario["bam"], "--Reference", "unread.fa",
                            "--DisableSanityCheck", "--incl-flags", "1024", "--adjust-MQ", "0", "--Output", out + "2"],
                           capture_output=True, text=True, timeout=120)
    assert quiet.returncode == 0 and "--incl-flags 1024 --adjust-MQ 0" not in quiet.stderr, quiet.stderr
    row = open(out + ".selfSM").read().splitlines()[1].split("\t")
    assert row[0] == "DefaultSampleName" and row[4] == str(scenario["want"]()["num_bases"])


# ------------------------------------------------------------------ pinned to the reference's golden files

def _golden_bam(golden_dir, tmp, pileup_name):
    """the golden text pileup as a BAM: one read per parsed base (bam_ref.records_from_pileup), no @RG, mapQ 60"""
    from oracle import refio
    rows = br.read_bed_rows(os.path.join(golden_dir, HAPMAP + ".bed"))
    ref_of = {}
    for c, p, ref, _ in rows:
        ref_of[(c, p)] = ref
    lines = []
    for line in open(os.path.join(golden_dir, pileup_name)):
        t = line.split()
        if not t or (t[0], int(t[1])) not in ref_of:
            continue
        b, q = refio.parse_pileup_seq(t[4] if len(t) > 4 else "", t[5] if len(t) > 5 else "")
        lines.append((t[0], int(t[1]), b, q))
    chroms = sorted({c for c, _, _, _ in lines})
    refs = [(c, 1 << 28) for c in chroms]
    recs = br.records_from_pileup(lines, ref_of, {c: i for i, c in enumerate(chroms)})
    assert len({len(r["seq"]) for r in recs}) >= 3
    bam = os.path.join(tmp, os.path.basename(pileup_name) + ".bam")
    br.write_indexed_bam(bam, refs, recs, block_payload=300)
    return bam, sum(len(b) for _, _, b, _ in lines)


def _cli(golden_dir, out, extra):
    p = subprocess.run([EXE, "--DisableSanityCheck", "--SVDPrefix", os.path.join(golden_dir, HAPMAP), "--Reference",
                        "resource/test/chr20.fa.gz", "--NumPC", "2", "--Output", out] + extra, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


@gpu
def test_golden_result_from_bam_input(golden_dir, tmp_path):
    """expected/result.Pileup turned into a BAM and read with --BamFile: .Ancestry and .selfSM byte for byte -- #READS 71
    included, which text input can only print as NA."""
    bam, n = _golden_bam(golden_dir, str(tmp_path), os.path.join("expected", "result.Pileup"))
    assert n == 71
    out = str(tmp_path / "r")
    _cli(golden_dir, out, ["--BamFile", bam])
    assert open(out + ".Ancestry").read() == open(os.path.join(golden_dir, "expected", "result.Ancestry")).read()
    assert open(out + ".selfSM").read() == open(os.path.join(golden_dir, "expected", "result.selfSM")).read()


@gpu
def test_golden_long_read_from_bam_input(golden_dir, tmp_path):
    bam, _ = _golden_bam(golden_dir, str(tmp_path), "test.LongRead.pileup")
    out = str(tmp_path / "l")
    _cli(golden_dir, out, ["--BamFile", bam, "--min-BQ", "0"])
    assert open(out + ".Ancestry").read() == open(os.path.join(golden_dir, "expected", "test.LongRead.pileup.Ancestry")).read()
    got = open(out + ".selfSM").read().splitlines()
    want = open(os.path.join(golden_dir, "expected", "test.LongRead.pileup.selfSM")).read().splitlines()
    assert got[0] == want[0]
    g, w = got[1].split("\t"), want[1].split("\t")
    assert g[4].isdigit()
    g[4] = w[4]                                   # #READS: the expected file came from text input (NA)
    assert g == w


@gpu
def test_written_pileup_reingested_gives_the_same_estimate(golden_dir, tmp_path):
    bam, _ = _golden_bam(golden_dir, str(tmp_path), os.path.join("expected", "result.Pileup"))
    hap = os.path.join(golden_dir, HAPMAP)
    a = vb.run_files(hap, None, str(tmp_path / "a"), num_pc=2, disable_sanity=True, output_pileup=True, bam_path=bam)
    b = vb.run_files(hap, str(tmp_path / "a.Pileup"), str(tmp_path / "b"), num_pc=2, disable_sanity=True)
    assert a["alpha"] == b["alpha"] and a["llk1"] == b["llk1"] and a["llk0"] == b["llk0"]
    assert np.array_equal(a["pc"], b["pc"]) and np.array_equal(a["pc2"], b["pc2"])
    assert a["num_bases"] == 71 and a["num_site"] == b["num_site"] and a["avg_depth"] == b["avg_depth"]
    assert open(str(tmp_path / "a.Ancestry")).read() == open(str(tmp_path / "b.Ancestry")).read()
    ga, gb = (open(str(tmp_path / x) + ".selfSM").read().splitlines() for x in "ab")
    ra, rb = ga[1].split("\t"), gb[1].split("\t")
    assert (ra[4], rb[4]) == ("71", "NA")
    ra[4] = rb[4]
    assert ga[0] == gb[0] and ra == rb


@gpu
def test_confidence_interval_from_bam_input(golden_dir, tmp_path):
    bam, _ = _golden_bam(golden_dir, str(tmp_path), os.path.join("expected", "result.Pileup"))
    out = str(tmp_path / "ci")
    _cli(golden_dir, out, ["--BamFile", bam, "--ConfidenceInterval"])
    lines = open(out + ".CI").read().splitlines()
    assert lines[0].startswith("#PARAM") and lines[1].split("\t")[0] == "FREEMIX"
    via_text = str(tmp_path / "ci_text")
    _cli(golden_dir, via_text, ["--PileupFile", os.path.join(golden_dir, "expected", "result.Pileup"), "--ConfidenceInterval"])
    assert open(out + ".CI").read() == open(via_text + ".CI").read()
