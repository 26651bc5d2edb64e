"""GPU tests of --PerReadGroup: the records' groups up with their descriptors, the second key and
sort, the site kernel over (group, site), one vb2_flat per group, the lock-step search of the groups and <Output>.selfRG.

One synthetic BAM of a few hundred reads (tests/bam_ref.py's writer: blocks of 300 payload bytes) holds every case by
name; what every group's pileup must be comes from readgroup_ref.group_pileup_ref -- the definition restated over the list
of records -- and from the reference's golden files, never from the code under test.  Every test marked gpu fails on a
library without the feature, where the symbols do not exist; the one unmarked test checks the scenario itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
import readgroup_ref as rr  # noqa: E402

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
HAPMAP = os.path.join("hapmap", "hapmap_3.3.b37.dat")
REFS = [("chr1", 500000), ("chr2", 500000)]
P, PP = br.FPAIRED, br.FPAIRED | br.FPROPER
IDS = ["A", "B", "C", "D", "E"]                      # E: in the header, carried by no read
# the same reads under a header of 70 groups: more groups than a wave has lanes, D behind index 64
IDS70 = ["x%02d" % i for i in range(20)] + ["A"] + ["y%02d" % i for i in range(20)] + ["B", "C", "E"] + \
        ["z%02d" % i for i in range(25)] + ["D"]


def _seq(n, start=0):
    return "".join("ACGT"[(start + i * 7 + i // 3) % 4] for i in range(n))


def _q(n, base=20):
    return [base + (i * 3) % 15 for i in range(n)]


def _at(name, tid, pos, n, at, base, q, group, flag=0, cigar=None, **kw):
    """a read of n bases from 0-based pos with `base` and quality q at 0-based reference position `at`"""
    s, qq = list(_seq(n, pos)), _q(n, 30)
    if cigar is None:
        s[at - pos], qq[at - pos] = base, q
    r = br.rec(name, tid, pos, cigar or "%dM" % n, "".join(s), qq, flag=flag, **kw)
    return rr.tag(r, group) if group != "ZZ" else rr.tag(r, "ZZ", truth=None)


def _scenario():
    """(records, bed rows, at): at maps a case to the (chr, pos1) it lives at"""
    R, rows, at = [], [], {}

    def marker(case, c, p, ref="A", alt="C"):
        rows.append((c, p, ref, alt))
        at[case] = (c, p)

    # -- sites of 70 and 300 reads, the groups interleaved, with mates (of different groups, too), deletions and low
    #    qualities inside; untagged reads and reads of an unknown ID among them; D only behind entry 64 of the deep one
    for case, c0, depth in (("deep70", 10000, 70), ("deep300", 20000, 300)):
        marker(case, "chr1", c0 + 1, ref="T")
        for i in range(depth):
            pos = c0 - 90 + (i * 88) // depth                       # ascending: file order is i
            name, flag, mpos = "%s_%d" % (case, i), 0, -1
            if i % 7 == 3 and i + 2 < depth:
                name, flag, mpos = "%s_p%d" % (case, i), PP | 64, c0 - 90 + ((i + 2) * 88) // depth
            if i % 7 == 5 and i >= 2:
                name, flag, mpos = "%s_p%d" % (case, i - 2), PP | 128 | br.FREVERSE, c0 - 90 + ((i - 2) * 88) // depth
            cigar = "100M" if i % 11 else "%dM4D%dM" % (c0 - pos - 1, 100 - (c0 - pos - 1))
            qq = _q(100, 18 + i % 9)
            if i % 13 == 0:
                qq[c0 - pos] = 5
            group = "ABC"[i % 3]
            if case == "deep300" and i >= 64 and i % 6 == 0:
                group = "D"
            if i % 10 == 9:
                group = None
            if i % 17 == 16:
                group = "ZZ"
            r = br.rec(name, 0, pos, cigar, _seq(100, i), qq, flag=flag | (br.FREVERSE if i % 5 == 0 else 0), mtid=0, mpos=mpos)
            R.append(rr.tag(r, group) if group != "ZZ" else rr.tag(r, "ZZ", truth=None))
    # -- a group with only a deleted read at a site (indexed, depth 0), and one with only a read below --min-BQ
    marker("only_deleted", "chr2", 1000)
    R += [_at("od_a0", 1, 980, 40, 999, "C", 30, "A"), _at("od_b", 1, 985, 20, 999, "C", 30, "B", cigar="10M30D10M"),
          _at("od_a1", 1, 990, 40, 999, "A", 31, "A")]
    marker("only_lowq", "chr2", 2000)
    R += [_at("ol_a0", 1, 1980, 40, 1999, "C", 30, "A"), _at("ol_c", 1, 1985, 40, 1999, "C", 3, "C"),
          _at("ol_a1", 1, 1990, 40, 1999, "A", 31, "A")]
    # -- overlapping mates of one group whose resolution zeroes the second quality; a read of another group between them
    marker("overlap", "chr2", 3000)
    R += [_at("ov", 1, 2960, 60, 2999, "G", 30, "A", flag=PP | 64, mtid=1, mpos=2980),
          _at("ov_b", 1, 2970, 60, 2999, "C", 22, "B"),
          _at("ov", 1, 2980, 60, 2999, "G", 25, "A", flag=PP | 128 | br.FREVERSE, mtid=1, mpos=2960)]
    # -- the quirk within a group: A's deleted read comes first, its quality (that of the query offset where the deletion
    #    starts) stays in A's list and shifts A's quality string; B's reads lie between
    marker("quirk", "chr2", 4000)
    qd = br.rec("qk_del", 1, 3970, "20M20D20M", _seq(40, 1), [35] * 40)
    R += [rr.tag(qd, "A"), _at("qk_b0", 1, 3975, 40, 3999, "C", 40, "B"), _at("qk_a0", 1, 3980, 40, 3999, "C", 20, "A"),
          _at("qk_b1", 1, 3985, 40, 3999, "A", 41, "B"), _at("qk_a1", 1, 3990, 40, 3999, "A", 30, "A")]
    # -- max_depth 5 over 8 reads: A loses its tail, C loses the site, B keeps both of its reads
    marker("cap", "chr2", 5000)
    for i, g in enumerate("AABABACC"):
        R.append(_at("cap%d" % i, 1, 4970 + 3 * i, 40, 4999, "ACGT"[i % 4], 25 + i, g))
    # -- a site that only reads of no group cover; an orphan of A beside a plain read of B
    marker("nobody", "chr2", 6000)
    R += [_at("nb0", 1, 5980, 40, 5999, "C", 30, None), _at("nb1", 1, 5985, 40, 5999, "A", 30, "ZZ")]
    marker("orphan", "chr2", 7000)
    R += [_at("or_a", 1, 6980, 40, 6999, "C", 30, "A", flag=P, mtid=1, mpos=6980), _at("or_b", 1, 6985, 40, 6999, "A", 30, "B")]
    marker("absent_site", "chr2", 7500)
    # -- a position the .bed lists twice (the later alleles win)
    rows.append(("chr2", 8000, "A", "C"))
    at["dup_row"] = ("chr2", 8000)
    R += [_at("d%d" % i, 1, 7970 + 4 * i, 40, 7999, "GA"[i % 2], 30, "ABC"[i % 3], flag=br.FREVERSE if i % 3 == 0 else 0) for i in range(6)]
    R.sort(key=lambda r: (r["tid"], r["pos"]))
    rows.append(("chr2", 8000, "G", "T"))
    return R, rows, at


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("rg")
    recs, rows, at = _scenario()
    assert len(recs) <= 500
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
    bam, bam70 = str(d / "s.bam"), str(d / "s70.bam")
    br.write_indexed_bam(bam, REFS, recs, block_payload=300, text=rr.rg_header(REFS, IDS))
    br.write_indexed_bam(bam70, REFS, recs, block_payload=300, text=rr.rg_header(REFS, IDS70))
    cache = {}

    def want(ids=tuple(IDS), **opts):
        key = (ids, tuple(sorted(opts.items())))
        if key not in cache:
            cache[key] = (rr.group_pileup_ref(recs, REFS, rows, list(ids), opts), br.pileup_ref(recs, REFS, rows, opts))
        return cache[key]

    return dict(recs=recs, rows=rows, at=at, pre=pre, bam=bam, bam70=bam70, want=want, dir=str(d))


def test_the_scenario_holds_its_cases(scenario):
    """The restatement's own answers at the named sites: the cases are really in the file (no device involved)."""
    at, recs = scenario["at"], scenario["recs"]
    (groups, unassigned), whole = scenario["want"]()
    A, B, C, D, E = (g["sites"] for g in groups)
    assert len(IDS) == 5 and E == {} and all(r["rg"] != "E" for r in recs)                 # named in the header, carried by no read
    assert sum(1 for r in recs if r["rg"] is None and b"RGZ" not in r["aux"]) >= 30        # no tag
    assert sum(1 for r in recs if r["rg"] is None and b"RGZZZ\0" in r["aux"]) >= 15        # an unknown ID
    assert unassigned > 30 and at["nobody"] in whole["sites"] and all(at["nobody"] not in g["sites"] for g in groups)
    for case, depth in (("deep70", 70), ("deep300", 300)):
        ent = br.site_entries(recs, 0, at[case][1], dict(br.DEFAULT_OPTS))
        assert len(ent) == depth
        order = [e["rec"]["rg"] for e in ent]
        assert order[:6] == ["A", "B", "C", "A", "B", "C"]                                 # interleaved
        assert all(len(g[at[case]][0]) > 10 for g in (A, B, C))
    assert at["deep70"] not in D and len(D[at["deep300"]][0]) > 20
    first_d = next(i for i, e in enumerate(br.site_entries(recs, 0, at["deep300"][1], dict(br.DEFAULT_OPTS))) if e["rec"]["rg"] == "D")
    assert first_d >= 64                                                                    # D's entries lie behind entry 64
    assert B[at["only_deleted"]] == ("", "") and len(A[at["only_deleted"]][0]) == 2         # indexed, depth 0
    assert C[at["only_lowq"]] == ("", "") and scenario["want"](min_bq=0)[0][0][2]["sites"][at["only_lowq"]] == ("C", "$")
    assert A[at["overlap"]] == ("G", chr(33 + 55)) and B[at["overlap"]] == ("C", chr(33 + 22))      # 30 + 25, the second zeroed
    assert scenario["want"](incl_flags=16)[0][0][0]["sites"][at["overlap"]] == ("Gg", chr(33 + 30) + chr(33 + 25))
    # the quirk: A's two bases carry the deleted read's quality and the first base's, not their own (20, 30)
    assert A[at["quirk"]] == ("C.", chr(33 + 35) + chr(33 + 20)) and B[at["quirk"]] == ("C.", chr(33 + 40) + chr(33 + 41))
    capped = scenario["want"](max_depth=5)[0][0]
    assert len(A[at["cap"]][0]) == 4 and len(capped[0]["sites"][at["cap"]][0]) == 3         # A loses its tail
    assert at["cap"] in C and at["cap"] not in capped[2]["sites"]                           # C loses the site
    assert capped[1]["sites"][at["cap"]] == B[at["cap"]] and len(B[at["cap"]][0]) == 2
    assert at["orphan"] in A and at["orphan"] not in scenario["want"](no_orphans=1)[0][0][0]["sites"]
    assert all(at["absent_site"] not in g["sites"] for g in groups)
    assert IDS70.index("D") >= 64 and len(IDS70) == 70 and set(IDS) <= set(IDS70)
    # the groups partition the whole sample's bases
    assert sum(g["num_bases"] for g in groups) + unassigned == whole["num_bases"]


OPTION_SETS = {
    "defaults": {},
    "min_bq_0": dict(min_bq=0),
    "max_depth_5": dict(max_depth=5),
    "max_depth_64": dict(max_depth=64),
    "no_overlap_rule": dict(incl_flags=16),
    "no_orphans": dict(no_orphans=1),
    "header_of_70_groups": {},
    "small_batches": {},
}


def _same(got, want, rows, tag):
    """pools, per-marker offsets, the site set, numBases and avgDepth: byte for byte"""
    off = got["read_off"]
    assert len(off) == len(rows) + 1
    for i, (c, p, _, _) in enumerate(rows):
        b, q = got["bases"][off[i]:off[i + 1]].decode("latin-1"), got["quals"][off[i]:off[i + 1]].decode("latin-1")
        assert (b, q) == want["rows"][i], (tag, "%s:%d" % (c, p), b, q, want["rows"][i])
    assert got["num_site"] == want["num_site"], tag
    assert got["num_bases"] == want["num_bases"], tag
    assert got["avg_depth"] == want["avg_depth"], tag


@gpu
@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_every_groups_pileup_is_the_restatements_and_the_whole_sample_is_unchanged(scenario, name, tunable):
    opts = OPTION_SETS[name]
    ids = IDS70 if name == "header_of_70_groups" else IDS
    bam = scenario["bam70"] if name == "header_of_70_groups" else scenario["bam"]
    (want, unassigned), want_whole = scenario["want"](ids=tuple(ids), **opts)
    if name == "small_batches":
        tunable("bam_batch_kb", 8)
    got = vb.api.load_bam_groups(scenario["pre"], bam, mpileup=opts or None)
    plain = vb.api.load_bam(scenario["pre"], bam, mpileup=opts or None)
    print(name, "whole: sites %d bases %d" % (got["num_site"], got["num_bases"]), got["stats"])
    # 1. every group's pileup
    assert [g["id"] for g in got["groups"]] == ids
    for g, w in zip(got["groups"], want):
        print("  %s: records %d sites %d bases %d status %d" % (g["id"], g["records"], g["num_site"], g["num_bases"], g["status"]))
        _same(g, w, scenario["rows"], (name, g["id"]))
        assert g["records"] == sum(1 for r in scenario["recs"] if r["rg"] == g["id"])
        assert g["status"] == (_abi.VB2_OK if w["num_bases"] else _abi.VB2_GROUP_NO_BASE)
    assert got["unassigned"] == sum(1 for r in scenario["recs"] if r["rg"] is None)
    # A, B, C and D have bases; D lies behind entry 64 of its only site, so a cap of 64 or less leaves it none
    assert sum(1 for w in want if w["num_bases"]) == (3 if opts.get("max_depth", 8000) <= 64 else 4)
    # 2. the whole sample: what the load without groups gives, and the restatement's
    for key in ("bases", "quals", "num_site", "num_bases", "avg_depth"):
        assert got[key] == plain[key], (name, key)
    assert list(got["read_off"]) == list(plain["read_off"])
    for key in ("entries", "pairs_resolved", "capped_sites", "sites", "empty_sites", "records_kept", "batches"):
        assert got["stats"][key] == plain["stats"][key], (name, key)
    _same(got, want_whole, scenario["rows"], (name, "whole"))
    if name == "small_batches":
        assert got["stats"]["batches"] >= 3
    if name == "max_depth_5":
        assert got["stats"]["capped_sites"] >= 3
    # 3. the groups partition the whole sample's bases
    assert sum(g["num_bases"] for g in got["groups"]) + unassigned == got["num_bases"]


@gpu
def test_records_that_all_miss_the_panel_leave_every_group_empty(scenario, tmp_path):
    """reads on chr1 only, one marker on chr2: no record is kept; every group of the header is there, named and empty"""
    recs = [r for r in scenario["recs"] if r["tid"] == 0][:12]
    assert len(recs) == 12
    pre, bam = str(tmp_path / "miss"), str(tmp_path / "miss.bam")
    with open(pre + ".bed", "w") as fh:
        fh.write("chr2\t999\t1000\tA\tC\n")
    open(pre + ".UD", "w").write("0.01 0.02\n")
    open(pre + ".mu", "w").write("chr2:1000_A/C 0.4\n")
    br.write_indexed_bam(bam, REFS, recs, block_payload=300, text=rr.rg_header(REFS, IDS))
    got = vb.api.load_bam_groups(pre, bam)
    print(got["stats"], [(g["id"], g["records"], g["status"]) for g in got["groups"]])
    st = got["stats"]
    assert (st["records_kept"], st["batches"], st["entries"], st["sites"]) == (0, 0, 0, 0)
    assert (got["num_site"], got["num_bases"], got["avg_depth"], got["unassigned"]) == (0, 0, 0.0, 0)
    assert [g["id"] for g in got["groups"]] == IDS
    for g in got["groups"]:
        assert (g["records"], g["num_site"], g["num_bases"], g["avg_depth"]) == (0, 0, 0, 0.0)
        assert g["bases"] == b"" and g["quals"] == b"" and list(g["read_off"]) == [0, 0]
        assert g["status"] == _abi.VB2_GROUP_NO_BASE


# ------------------------------------------------------------------ end to end: three groups with different contamination

ALPHAS = (0.01, 0.05, 0.12)
E2E_IDS = ["g0", "g1", "g2", "tiny", "none"]


@pytest.fixture(scope="module")
def three_groups(tmp_path_factory):
    """One synthetic panel of 2 000 markers; three text pileups of depth 10 on it with different planted alpha, turned into
    reads (bam_ref.records_from_pileup), tagged g0..g2 and merged with a stable sort into one BAM of 60 000-byte blocks.
    Two more groups in the header: `tiny`, with reads at 40 markers only (it fails a sanity check), and `none`."""
    tmp = tmp_path_factory.mktemp("rg_e2e")
    k, M = 2, 2000
    base = vb.synth.make_pileup(M, 10, k, alpha_true=0.03, seed=50)
    pre = vb.synth.write_files(base, str(tmp / "panel"))
    rows = br.read_bed_rows(pre + ".bed")
    chrs, poss, refs_c, _ = vb.synth.read_bed_rows(pre + ".bed")
    ref_of = {(c, p): r for c, p, r, _ in rows}
    recs, piles = [], []
    for s, gid in enumerate(E2E_IDS[:4]):
        if gid == "tiny":
            off, b, q = vb.synth.reads_on_panel(base.means, base.meta["ref_base"], base.alt_base, 10, 0.0, seed=99)
            off = np.minimum(off, off[40])                      # reads at the first 40 markers only
        else:
            off, b, q = vb.synth.reads_on_panel(base.means, base.meta["ref_base"], base.alt_base, 10, ALPHAS[s], seed=70 + s)
        piles.append(vb.synth.write_pileup_text(str(tmp / (gid + ".pileup")), chrs, poss, refs_c, off, b, q))
        bs, qs = b.tobytes().decode("latin-1"), q.tobytes().decode("latin-1")
        lines = [(chrs[i], int(poss[i]), bs[off[i]:off[i + 1]], qs[off[i]:off[i + 1]]) for i in range(M) if off[i + 1] > off[i]]
        # records_from_pileup looks at every position of ref_of per base: 50 lines at a time, with the positions a read of
        # 100 bases could reach beside them (the markers are 10 apart)
        for lo in range(0, len(lines), 50):
            chunk = lines[lo:lo + 50]
            near = {(c, p): ref_of[(c, p)] for c, p in ((chunk[0][0], x) for x in range(chunk[0][1] - 110, chunk[-1][1] + 111))
                    if (c, p) in ref_of}
            for r in br.records_from_pileup(chunk, near, {"1": 0}):
                r["name"] = "%s_%d_%s" % (gid, lo, r["name"])
                recs.append(rr.tag(r, gid))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))               # stable: a group's reads of a site keep their order
    bam = str(tmp / "three.bam")
    br.write_indexed_bam(bam, [("1", 1 << 28)], recs, block_payload=60000, text=rr.rg_header([("1", 1 << 28)], E2E_IDS, sample="S3"))
    want, unassigned = rr.group_pileup_ref(recs, [("1", 1 << 28)], rows, E2E_IDS)
    assert unassigned == 0
    return dict(pre=pre, bam=bam, piles=piles, rows=rows, want=want, k=k, tmp=tmp, M=M)


def _cli(f, out, extra):
    p = subprocess.run([EXE, "--SVDPrefix", f["pre"], "--BamFile", f["bam"], "--Reference", "unread.fa", "--NumPC", str(f["k"]),
                        "--Output", out] + extra, capture_output=True, text=True, timeout=300)
    return p


def _fmt(x):
    return "%g" % x


@gpu
def test_three_groups_end_to_end(three_groups):
    f = three_groups
    tmp, k = f["tmp"], f["k"]
    out = str(tmp / "api")
    res = vb.run_files(f["pre"], None, out, num_pc=k, disable_sanity=True, bam_path=f["bam"], output_pileup=True,
                       per_read_group=True)
    groups = res["read_groups"]
    assert [g["header_index"] for g in groups] == list(range(5))
    assert [g["status"] for g in groups] == [0, 0, 0, 0, _abi.VB2_GROUP_NO_BASE]
    from oracle import binding, refio
    for s in range(3):
        # ... each group's estimate is that of a run on the group's own text pileup
        one = vb.run_files(f["pre"], f["piles"][s], str(tmp / ("single%d" % s)), num_pc=k, disable_sanity=True)
        g = groups[s]
        print("group %s: planted alpha %.2f, recovered %.6f (alone %.6f), llk1 %.6f (alone %.6f), num_eval %d (alone %d)"
              % (E2E_IDS[s], ALPHAS[s], g["alpha"], one["alpha"], g["llk1"], one["llk1"], g["num_eval"], one["num_eval"]))
        assert abs(g["alpha"] - one["alpha"]) <= 1e-6, s
        assert abs(g["llk1"] - one["llk1"]) <= 1e-9 * max(1.0, abs(one["llk1"])), s
        assert (g["num_site"], g["num_bases"], g["avg_depth"]) == (one["num_site"], f["want"][s]["num_bases"], one["avg_depth"])
        # ... and the oracle's search on the Python restatement of the readers of that pileup
        flat, _, _ = refio.load_flat(f["pre"], f["piles"][s], k, sanity_disabled=True)
        ref = binding.OracleData(flat).optimize()
        assert abs(g["alpha"] - ref["alpha"]) <= 1e-4, (s, g["alpha"], ref["alpha"])
        assert g["num_eval"] == ref["num_eval"], (s, g["num_eval"], ref["num_eval"])
    # .selfRG: those values formatted as write_selfsm formats
    lines = open(out + ".selfRG").read().splitlines()
    assert lines[0] == open(out + ".selfSM").read().splitlines()[0] and len(lines) == 6
    for s, g in enumerate(groups):
        al = g["alpha"] if g["alpha"] < 0.5 else 1 - g["alpha"]
        est = [_fmt(al), _fmt(-g["llk1"]), _fmt(-g["llk0"])] if g["status"] == 0 else ["NA"] * 3
        assert lines[1 + s].split("\t") == ["S3", E2E_IDS[s], "NA", str(f["M"]), str(f["want"][s]["num_bases"]),
                                             _fmt(f["want"][s]["avg_depth"])] + est + ["NA"] * 10, (s, lines[1 + s])
    # --OutputPileup: one file per group, the restatement's sites as the writer prints them
    for s in range(5):
        assert open("%s.RG%d.Pileup" % (out, s)).read() == br.pileup_text(f["rows"], f["want"][s]["sites"]), s
    assert open(out + ".RG0.Pileup").read() == open(f["piles"][0]).read()
    # the command line: stdout, .selfSM, .Ancestry and .Pileup byte for byte those of the run without the flag
    a = _cli(f, str(tmp / "with"), ["--DisableSanityCheck", "--OutputPileup", "--PerReadGroup"])
    b = _cli(f, str(tmp / "without"), ["--DisableSanityCheck", "--OutputPileup"])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and "FREEMIX" in a.stdout
    for ext in (".selfSM", ".Ancestry", ".Pileup"):
        assert open(str(tmp / "with") + ext, "rb").read() == open(str(tmp / "without") + ext, "rb").read(), ext
    assert open(str(tmp / "with") + ".selfRG").read() == open(out + ".selfRG").read()
    assert not os.path.exists(str(tmp / "without") + ".selfRG")
    assert open(str(tmp / "with") + ".selfSM").read() == open(out + ".selfSM").read()


@gpu
def test_groups_that_are_not_searched_have_na_rows(three_groups):
    """With the sanity check on, `tiny` (40 markers) and `none` fail their own check; with it off, `none` has no base."""
    f = three_groups
    out = str(f["tmp"] / "sanity")
    res = vb.run_files(f["pre"], None, out, num_pc=f["k"], bam_path=f["bam"], per_read_group=True)
    assert [g["status"] for g in res["read_groups"]] == [0, 0, 0, _abi.VB2_ERR_SANITY, _abi.VB2_ERR_SANITY]
    lines = [l.split("\t") for l in open(out + ".selfRG").read().splitlines()]
    assert [l[1] for l in lines[1:]] == E2E_IDS
    for s in (3, 4):
        assert lines[1 + s][6:9] == ["NA", "NA", "NA"] and res["read_groups"][s]["num_eval"] == 0
        assert lines[1 + s][4] == str(f["want"][s]["num_bases"])
    for s in range(3):
        assert "NA" not in lines[1 + s][4:9]
    whole, = [l.split("\t") for l in open(out + ".selfSM").read().splitlines()[1:]]
    assert whole[4] == str(sum(w["num_bases"] for w in f["want"]))
    off = vb.run_files(f["pre"], None, str(f["tmp"] / "nosanity"), num_pc=f["k"], bam_path=f["bam"], per_read_group=True,
                       disable_sanity=True)
    assert [g["status"] for g in off["read_groups"]] == [0, 0, 0, 0, _abi.VB2_GROUP_NO_BASE]
    last = open(str(f["tmp"] / "nosanity") + ".selfRG").read().splitlines()[5].split("\t")
    assert last[:2] == ["S3", "none"] and last[4:9] == ["0", "0", "NA", "NA", "NA"]


# ------------------------------------------------------------------ pinned to the reference's golden files

@gpu
def test_golden_result_as_one_read_group(golden_dir, tmp_path):
    """expected/result.Pileup turned into a BAM whose reads all carry one group (a header line without SM:): that group's
    .selfRG row is the golden result.selfSM row in every column but RG, #READS 71 included."""
    from oracle import refio
    rows = br.read_bed_rows(os.path.join(golden_dir, HAPMAP + ".bed"))
    ref_of = {(c, p): ref for c, p, ref, _ in rows}
    lines = []
    for line in open(os.path.join(golden_dir, "expected", "result.Pileup")):
        t = line.split()
        if not t or (t[0], int(t[1])) not in ref_of:
            continue
        b, q = refio.parse_pileup_seq(t[4] if len(t) > 4 else "", t[5] if len(t) > 5 else "")
        lines.append((t[0], int(t[1]), b, q))
    chroms = sorted({c for c, _, _, _ in lines})
    refs = [(c, 1 << 28) for c in chroms]
    recs = br.records_from_pileup(lines, ref_of, {c: i for i, c in enumerate(chroms)})
    for i, r in enumerate(recs):
        rr.tag(r, "lane7", before=rr.AUX_FIELDS["i"] if i % 2 else b"")
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@RG\tPL:x\tID:lane7\n"
    bam = str(tmp_path / "golden.bam")
    br.write_indexed_bam(bam, refs, recs, block_payload=300, text=text)
    out = str(tmp_path / "r")
    p = subprocess.run([EXE, "--DisableSanityCheck", "--SVDPrefix", os.path.join(golden_dir, HAPMAP), "--Reference",
                        "resource/test/chr20.fa.gz", "--NumPC", "2", "--Output", out, "--BamFile", bam, "--PerReadGroup"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    golden = open(os.path.join(golden_dir, "expected", "result.selfSM")).read()
    assert open(out + ".selfSM").read() == golden
    assert open(out + ".Ancestry").read() == open(os.path.join(golden_dir, "expected", "result.Ancestry")).read()
    got = open(out + ".selfRG").read().splitlines()
    want = golden.splitlines()
    assert got[0] == want[0] and len(got) == 2
    g, w = got[1].split("\t"), want[1].split("\t")
    assert g[1] == "lane7" and g[4] == "71"
    g[1] = w[1]
    assert g == w
