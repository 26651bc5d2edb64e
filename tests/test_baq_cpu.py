"""--ApplyBAQ without a device: the HMM against what the reference's own compiled kpa_glocal gave
(tests/golden/baq/kpa_cases.json, recipe tests/golden/make_baq_fixtures.py), the Python restatement (baq_ref.py) against
the same, the host core of csrc/baq_core.h against both, the threshold table against libm, the wrapper and the cap per
record of a scenario BAM, the FASTA reader, the plumbing of the switch, and a stand-alone program under the host
sanitizers.  Expected values never come from the code under test."""
import ctypes
import json
import math
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
import baq_ref  # noqa: E402
import baq_scenario as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
CASES = os.path.join(ROOT, "tests", "golden", "baq", "kpa_cases.json")


def _cases():
    out = []
    for c in json.load(open(CASES))["cases"]:
        out.append(dict(name=c["name"], bw=c["bw"], ref=list(bytes.fromhex(c["ref"])), query=list(bytes.fromhex(c["query"])),
                        qual=list(bytes.fromhex(c["qual"])), q=list(bytes.fromhex(c["q"])),
                        state=[int(x) for x in np.frombuffer(bytes.fromhex(c["state"]), dtype="<i4")]))
    return out


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    return sc.write_all(str(tmp_path_factory.mktemp("baq")))


def test_the_fixture_holds_its_cases():
    cases = _cases()
    lq = {len(c["query"]) for c in cases}
    assert {1, 2, 3, 8, 40, 100, 151, 600} <= lq and {1, 7, 10, 15} <= {c["bw"] for c in cases}
    assert any(4 in c["ref"] and 4 in c["query"] for c in cases) and any({0, 2, 41, 93, 255} <= set(c["qual"]) for c in cases)
    assert any(c["name"] == "nowhere" for c in cases) and os.path.getsize(CASES) <= 256 * 1024
    for c in cases:      # l_ref below, at and above l_query +- bw are all there for the lengths that allow it
        assert len(c["state"]) == len(c["q"]) == len(c["query"])
    d = {len(c["ref"]) - len(c["query"]) for c in cases if len(c["query"]) == 100 and c["bw"] == 7}
    assert {-9, -7, -1, 0, 1, 7, 9} <= d


def test_restatement_and_host_core_equal_the_references_hmm():
    for c in _cases():
        st, q, und = baq_ref.kpa_glocal(c["ref"], c["query"], c["qual"], c["bw"])
        assert und == 0 and st == c["state"] and q == c["q"], c["name"]
        st2, q2, und2 = vb.api.baq_case(c["ref"], c["query"], c["qual"], c["bw"])
        assert und2 == 0 and list(st2) == c["state"] and list(q2) == c["q"], c["name"]


def test_host_core_equals_the_restatement_on_random_cases():
    rng = random.Random(99)
    for i in range(300):
        lq = rng.choice((1, 2, 3, 5, 8, 13, 21, 34, 60))
        bw = rng.choice((1, 3, 7, 10))
        lr = max(1, lq + rng.randrange(-bw - 3, bw + 4))
        ref = [rng.choice((0, 1, 2, 3, 4)) if rng.random() < 0.1 else rng.randrange(4) for _ in range(lr)]
        query = [ref[min(lr - 1, max(0, j + (lr - lq) // 2))] if rng.random() > 0.15 else rng.randrange(5) for j in range(lq)]
        qual = [rng.choice((0, 2, 41, 93, 255)) if rng.random() < 0.1 else rng.randrange(2, 45) for _ in range(lq)]
        st, q, und = baq_ref.kpa_glocal(ref, query, qual, bw)
        st2, q2, und2 = vb.api.baq_case(ref, query, qual, bw)
        assert (st, q, und) == (list(st2), list(q2), und2), (i, lq, lr, bw)


def test_threshold_table_is_libms_quality():
    """the device never calls log: it searches 101 thresholds the host found with its libm.  100 000 seeded z in (0, 1] and
    both neighbours of every boundary give int(-4.343*log(z) + .499)"""
    L = _abi.lib()
    want = lambda z: min(baq_ref.quality_of(z), 101)  # noqa: E731
    rng = random.Random(7)
    for _ in range(100000):
        z = rng.random() if rng.random() < 0.5 else 10 ** (-rng.random() * 12)
        z = z if z > 0 else 1.0
        assert L.vb2_baq_quantise(z) == want(z), z
    assert L.vb2_baq_quantise(1.0) == 0
    for k in range(1, 102):
        lo, hi = 1e-300, 1.0      # the boundary of quality k by bisection here, with this side's libm
        for _ in range(1200):
            mid = math.sqrt(lo * hi) if lo < 1e-30 else (lo + hi) / 2
            if mid in (lo, hi):
                break
            if baq_ref.quality_of(mid) >= k:
                lo = mid
            else:
                hi = mid
        for z in (lo, hi, math.nextafter(lo, 0.0), math.nextafter(hi, 2.0), math.nextafter(lo, 2.0), math.nextafter(hi, 0.0)):
            assert L.vb2_baq_quantise(z) == want(z), (k, z)


def test_the_scenario_holds_its_cases(scenario):
    names = {r["name"] for r in scenario["recs"]}
    for n in ("len1", "len2", "len7", "len8", "len15", "len16", "len17", "len100", "len151", "long5k", "del12", "ins12", "soft_both",
              "hard_both", "pos0", "past_end", "outside", "n_op", "no_qual", "unmapped_placed", "tag_bq", "tag_zq", "tag_both",
              "ref_all_n", "query_all_n", "no_fasta_seq", "cap_drops", "pair_baq"):
        assert n in names, n
    adj = {r["name"]: a for r, a in zip(scenario["recs"], scenario["adjusted"]("defaults"))}
    assert adj["del12"]["shape"][1] == 15 and adj["ins12"]["shape"][1] == 15 and adj["len100"]["shape"][1] == 7
    assert adj["outside"]["outcome"] == baq_ref.OUTSIDE and adj["no_fasta_seq"]["outcome"] == baq_ref.NO_REFERENCE
    assert adj["cap_drops"]["outcome"] == baq_ref.CAP_DROPPED and 0 <= adj["cap_lowers"]["mapq"] < 60
    for n in ("n_op", "no_qual", "unmapped_placed", "tag_zq"):
        assert adj[n]["outcome"] == baq_ref.ALONE, n
    assert adj["tag_bq"]["outcome"] == baq_ref.TAG_APPLIED and adj["tag_both"]["outcome"] == baq_ref.TAG_APPLIED
    redo = {r["name"]: a for r, a in zip(scenario["recs"], scenario["adjusted"]("redo"))}
    assert redo["tag_bq"]["outcome"] == baq_ref.REALIGNED and redo["tag_both"]["outcome"] == baq_ref.ALONE
    assert adj["past_end"]["shape"][0] < 40 + 7 and adj["pos0"]["outcome"] == baq_ref.REALIGNED
    assert sum(a["undefined"] for a in adj.values()) == 0
    w, plain = scenario["want"]("defaults")["sites"], br.pileup_ref(scenario["recs"], sc.REFS, scenario["rows"], {})["sites"]
    at = scenario["at"]
    assert plain[at["pair_baq"]][0] == "G" and w[at["pair_baq"]][0] == "c"        # the overlap's winner changes
    assert at["cap_drops"] in plain and at["cap_drops"] not in w
    assert sum(1 for k in plain if k in w and len(w[k][0]) < len(plain[k][0])) >= 5      # bases BAQ moves under min-BQ


@pytest.mark.parametrize("name", sorted(sc.OPTION_SETS))
def test_host_core_equals_the_restatement_per_record(scenario, name):
    got = vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], mpileup=sc.OPTION_SETS[name] or None, where=0)
    want = scenario["adjusted"](name)
    assert len(got["mapq"]) == len(want) == len(scenario["recs"])
    for i, (r, a) in enumerate(zip(scenario["recs"], want)):
        q = list(got["qual"][int(got["qual_off"][i]):int(got["qual_off"][i + 1])])
        assert (int(got["outcome"][i]), int(got["mapq"][i]), list(got["cap4"][i]), q) == (a["outcome"], a["mapq"], a["cap4"], a["qual"]), r["name"]
    assert got["stats"]["undefined_rows"] == sum(a["undefined"] for a in want)
    assert got["stats"]["records_lds"] == 0 == got["stats"]["records_global"]      # no device was there


def test_device_stage_needs_a_device(scenario):
    if _abi.lib().vb2_device_count() > 0:
        return                # (with a device the stage runs: test_baq_gpu.py)
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], where=1)
    assert e.value.code == _abi.VB2_ERR_NO_DEVICE


# ---- the FASTA reader ----
def _fasta(tmp_path, width, genome, name="g.fa"):
    p = str(tmp_path / name)
    baq_ref.write_fasta(p, genome, width=width)
    return p


@pytest.mark.parametrize("width", [1, 60, 7])
def test_fasta_spans_whatever_the_line_width(tmp_path, width):
    rng = random.Random(width)
    genome = dict(a="".join(rng.choice("ACGT") for _ in range(137)), b="acgtnRYKMSWBDHVN-x*" * 3,
                  c="".join(rng.choice("ACGT") for _ in range(60 * 3 + 5)))      # (60: the last line is short)
    p = _fasta(tmp_path, width, genome)
    for name, seq in genome.items():
        codes, length = vb.api.fasta_fetch(p, name)
        assert length == len(seq) and list(codes) == [baq_ref.nt16_of(ch) for ch in seq]
        for beg, end in ((0, 1), (len(seq) - 1, len(seq)), (5, 5), (3, min(len(seq), 3 + 2 * width + 1))):
            assert list(vb.api.fasta_fetch(p, name, beg, end)[0]) == [baq_ref.nt16_of(ch) for ch in seq[beg:end]]
    # lower case is its upper case, IUPAC codes are themselves, anything else is N (htslib's seq_nt16_table)
    assert list(vb.api.fasta_fetch(p, "b", 0, 5)[0]) == [1, 2, 4, 8, 15] and list(vb.api.fasta_fetch(p, "b", 16, 19)[0]) == [15, 15, 15]
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.fasta_fetch(p, "not_there")
    assert e.value.code == _abi.VB2_ERR_INVALID


def test_fasta_index_missing_truncated_and_past_the_file(tmp_path):
    genome = dict(a="ACGT" * 50, b="GGCC" * 20)
    p = _fasta(tmp_path, 60, genome)
    fai = open(p + ".fai").read()
    os.remove(p + ".fai")
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.fasta_fetch(p, "a")
    assert e.value.code == _abi.VB2_ERR_IO and "samtools faidx" in str(e.value)
    for text in (fai[:len(fai) - 7], fai.replace("\t61\n", "\n", 1), "a\t200\t9999\t60\t61\n", "a\t99999\t3\t60\t61\n", "a\t200\t3\t0\t0\n",
                 "a\t200\tx\t60\t61\n"):
        open(p + ".fai", "w").write(text)
        with pytest.raises(_abi.Vb2Error) as e:
            vb.api.fasta_fetch(p, "a")
        assert e.value.code == _abi.VB2_ERR_INVALID, text
    gz = str(tmp_path / "z.fa")
    open(gz, "wb").write(b"\x1f\x8b\x08\x04" + b"\0" * 30)
    open(gz + ".fai", "w").write(fai)
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.fasta_fetch(gz, "a")
    assert e.value.code == _abi.VB2_ERR_INVALID and "compressed" in str(e.value)


# ---- plumbing ----
def test_the_switch_took_the_reserved_field_and_nothing_moved(scenario):
    L = _abi.lib()
    assert L.vb2_abi_version() == 7
    assert ctypes.sizeof(_abi.RunArgs) == 200          # read on the parent commit
    assert _abi.RunArgs.bam_adjust.offset == 124 and _abi.RunArgs.bam_adjust.size == 4      # where `reserved` was
    assert _abi.RunArgs.bam_path.offset == 128
    for s in ("vb2_flat_baq_stats", "vb2_baq_records", "vb2_baq_result_copy", "vb2_baq_result_stats", "vb2_baq_result_free", "vb2_baq_case",
              "vb2_baq_quantise", "vb2_baq_work_bytes", "vb2_fasta_fetch"):
        assert hasattr(L, s) and s in _abi.SYMBOLS
    assert _abi.get_tunable("baq_lds_kb") == 64
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.load_bam(scenario["pre"], scenario["bam"], apply_baq=2, reference_path=scenario["fasta"])
    assert e.value.code == _abi.VB2_ERR_INVALID and "bam_adjust" in str(e.value)
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], where=2)
    assert e.value.code == _abi.VB2_ERR_INVALID


@pytest.mark.parametrize("value", [-1, 2])
def test_refusals_that_need_neither_file_nor_device(scenario, value):
    """where and bam_adjust outside {0, 1}: text and code, before the BAM is opened (it does not exist).  vb2_flat_load
    refuses bam_adjust itself, so the reader's own "--BamFile: bam_adjust is ..." lies behind it and is never seen here."""
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.baq_records("no_such.bam", "no_such.bed", "no_such.fa", where=value)
    assert e.value.code == _abi.VB2_ERR_INVALID
    assert str(e.value).endswith("vb2_baq_records: where is 0 (host driver) or 1 (device stage)")
    with pytest.raises(_abi.Vb2Error) as e:
        vb.api.load_bam(scenario["pre"], "no_such.bam", apply_baq=value, reference_path="no_such.fa")
    assert e.value.code == _abi.VB2_ERR_INVALID
    assert str(e.value).endswith("vb2_flat_load: bam_adjust is %d; it is 0 (BAM records as they are) or 1 (--ApplyBAQ)" % value)


def test_command_line_refusals(scenario, tmp_path):
    base = [EXE, "--SVDPrefix", scenario["pre"], "--Reference", scenario["fasta"], "--ApplyBAQ"]
    r = subprocess.run(base + ["--PileupFile", str(tmp_path / "x.pileup")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--ApplyBAQ needs --BamFile, or a --PileupList with a .bam line" in r.stdout + r.stderr
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("%s\n" % (tmp_path / "a.pileup"))
    r = subprocess.run(base + ["--PileupList", lst], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--ApplyBAQ needs --BamFile, or a --PileupList with a .bam line" in r.stdout + r.stderr


def test_host_core_and_fasta_reader_under_the_sanitizers(scenario, tmp_path):
    """tests/baq_check_main.cpp + fasta_io.cpp + baq_host.cpp + bam_io.cpp built with -fsanitize=address,undefined and run
    directly: the fixture's cases, every record of the scenario (all wrapper edges) under two option sets, and mutilated
    FASTA files and indexes, which must end in an error code with a message."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "verifybamid_amd", "csrc")
    exe = str(tmp_path / "baq_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", src,
           os.path.join(ROOT, "tests", "baq_check_main.cpp"), os.path.join(src, "fasta_io.cpp"), os.path.join(src, "baq_host.cpp"),
           os.path.join(src, "bam_io.cpp"), "-lz", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    hexs = lambda a: bytes(a).hex() if len(a) else "-"  # noqa: E731
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        for c in _cases():
            f.write("%s %d %s %s %s %s %s\n" % (c["name"], c["bw"], hexs(c["ref"]), hexs(c["query"]), hexs(c["qual"]),
                                               b"".join((s & 0xffffffff).to_bytes(4, "little") for s in c["state"]).hex(), hexs(c["q"])))
    markers = str(tmp_path / "markers.txt")
    open(markers, "w").write("".join("%s %d\n" % (c, p) for c, p, _, _ in scenario["rows"]))
    # mutilated references
    fai = open(scenario["fasta"] + ".fai").read()
    broken = []
    for k, text in enumerate((fai[:len(fai) // 2], fai.replace("\t60\t61", "\t60", 1), fai.replace("\t30000\t", "\t99999999\t", 1),
                              "chr1\t30000\t999999999\t60\t61\n", fai.replace("\t60\t61", "\t0\t0", 1))):
        p = str(tmp_path / ("broken%d.fa" % k))
        shutil.copy(scenario["fasta"], p)
        open(p + ".fai", "w").write(text)
        broken += ["fail", p]
    p = str(tmp_path / "short.fa")                       # the index is whole, the file is not
    open(p, "wb").write(open(scenario["fasta"], "rb").read()[:5000])
    open(p + ".fai", "w").write(fai)
    broken += ["fail", p, "fail", str(tmp_path / "absent.fa")]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("defaults", "redo"):
        o = sc.full_opts(sc.OPTION_SETS[name])
        exp = str(tmp_path / ("expected_%s.txt" % name))
        with open(exp, "w") as f:
            for a in scenario["adjusted"](name):
                f.write("%d %d %d %d %d %d %s\n" % (a["outcome"], a["mapq"], *a["cap4"], hexs(a["qual"])))
        r = subprocess.run([exe, cases, markers, scenario["bam"], scenario["fasta"], str(o["incl_flags"]), str(o["adjust_mq"]), exp] + broken,
                           capture_output=True, text=True, timeout=300, env=env)
        print(r.stdout)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert lines[0] == "cases %d bad 0" % len(_cases()) and lines[1].startswith("records %d bad 0" % len(scenario["recs"]))
        assert sum(1 for ln in lines if ln.startswith("refused ")) == len(broken) // 2
