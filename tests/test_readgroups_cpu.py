"""CPU tests of --PerReadGroup's host side: the @RG lines of the header, the walk over a record's
auxiliary fields and its validation (verifybamid_amd/csrc/bam_io.cpp), the new symbols and the command line's refusals --
no GPU.  Files come from the writer of tests/bam_ref.py (blocks of 300 payload bytes: auxiliary fields straddle them);
a record's group is the test's own (tests/readgroup_ref.py's tag)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
import readgroup_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
REFS = [("chrA", 400000), ("chrB", 400000)]
MARKERS = [("chrA", 5000, "A", "C"), ("chrA", 16384, "G", "T"), ("chrB", 7000, "C", "T")]
GROUPS = [("lane1", "PL:ILLUMINA\tLB:libA", "PU:unit1"), ("lane2", "", ""), ("lane3", "DS:a description\tPL:x", "LB:libB"),
          ("unused", "", "")]
IDS = [g[0] for g in GROUPS]

NEW_SYMBOLS = ["vb2_bam_scan_ex", "vb2_bam_scan_num_group", "vb2_bam_scan_group_id", "vb2_bam_scan_record_groups",
               "vb2_flat_load_groups", "vb2_flat_groups_count", "vb2_flat_groups_id", "vb2_flat_groups_records",
               "vb2_flat_groups_status", "vb2_flat_groups_flat", "vb2_flat_groups_unassigned", "vb2_flat_groups_seconds",
               "vb2_flat_groups_free",
               "vb2_run_read_groups"]


def _write_panel(pre, rows):
    with open(pre + ".bed", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(pre + ".UD", "w") as fh:
        for i in range(len(rows)):
            fh.write("%g %g\n" % (0.01 * (i % 7 - 3), 0.02 * (i % 5 - 2)))
    with open(pre + ".mu", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s:%d_%s/%s 0.5\n" % (c, p, r, a))


def _read(name, tid, pos, n=40):
    return br.rec(name, tid, pos, "%dM" % n, "ACGT" * (n // 4), [30] * n)


def _records():
    """reads over the markers, each with another arrangement of auxiliary fields; r["rg"] is the group the test expects"""
    R, k = [], 0

    def add(tid, marker, group_id, before=b"", after=b"", truth="same"):
        nonlocal k
        R.append(rr.tag(_read("r%d" % k, tid, marker - 1 - (k * 3) % 35), group_id, before, after, truth))
        k += 1

    bare = _read("bare", 0, 4990)                       # no auxiliary bytes at all (not even the key)
    bare["rg"] = None
    R.append(bare)
    add(0, 5000, None)                                  # the key with empty bytes
    add(0, 5000, None, before=rr.AUX_FIELDS["i"] + rr.AUX_FIELDS["Z"])      # fields, but no RG
    for j, name in enumerate(sorted(rr.AUX_FIELDS)):    # RG behind one field of every type and every B subtype
        add(0, 5000 if j % 2 else 16384, IDS[j % 3], before=rr.AUX_FIELDS[name])
    everything = b"".join(rr.AUX_FIELDS[n] for n in sorted(rr.AUX_FIELDS))
    add(0, 16384, "lane2", before=everything)           # RG as the last field
    add(1, 7000, "lane3", after=everything)             # ... and as the first
    add(1, 7000, "lane1", before=rr.AUX_FIELDS["Bf"], after=rr.AUX_FIELDS["H"])
    add(1, 7000, None, before=b"RGA" + b"x", truth=None)                    # an RG of type A: no group
    add(1, 7000, None, before=b"RGH" + b"AB\0", truth=None)                 # ... of type H
    add(1, 7000, "lane9", truth=None)                   # an ID the header lacks
    add(1, 7000, "", truth=None)                        # an empty ID
    add(1, 7000, "lane", truth=None)                    # a prefix of one
    add(0, 5000, "lane1")
    R.sort(key=lambda r: (r["tid"], r["pos"]))
    return R


def _fixture(tmp_path, records=None, groups=GROUPS, name="s"):
    recs = _records() if records is None else records
    pre = str(tmp_path / "p")
    _write_panel(pre, MARKERS)
    bam = str(tmp_path / (name + ".bam"))
    vo, ve, blocks = br.write_indexed_bam(bam, REFS, recs, block_payload=300, text=rr.rg_header(REFS, groups))
    return recs, pre, bam, vo, blocks


def test_new_symbols_exist_and_the_abi_version_is_unchanged():
    L = _abi.lib()
    assert all(hasattr(L, s) for s in NEW_SYMBOLS) and set(NEW_SYMBOLS) <= set(_abi.SYMBOLS)
    assert L.vb2_abi_version() == 7


def test_group_ids_in_header_order_whatever_stands_before_the_id(tmp_path):
    recs, pre, bam, vo, _ = _fixture(tmp_path)
    got = vb.api.bam_scan(bam, pre + ".bed", groups=True)
    assert got["group_ids"] == IDS and got["sample"] == "S1"
    plain = vb.api.bam_scan(bam, pre + ".bed")
    assert "group_ids" not in plain and list(plain["voffsets"]) == list(got["voffsets"])


def test_record_groups_are_the_tests_own(tmp_path):
    recs, pre, bam, vo, blocks = _fixture(tmp_path)
    assert len(blocks) > 10                               # 300-byte blocks: auxiliary fields straddle them
    got = vb.api.bam_scan(bam, pre + ".bed", groups=True)
    index_of = {v: i for i, v in enumerate(vo)}
    fetched = [index_of[int(v)] for v in got["voffsets"]]
    assert len(fetched) == len(recs) == len(got["record_groups"])          # every read here covers a marker
    want = [IDS.index(recs[i]["rg"]) if recs[i]["rg"] is not None else _abi.VB2_BAM_NO_GROUP for i in fetched]
    assert [int(g) for g in got["record_groups"]] == want
    assert want.count(_abi.VB2_BAM_NO_GROUP) == 8 and {0, 1, 2} <= set(want) and 3 not in want
    # the same whatever the block size
    big = str(tmp_path / "big.bam")
    br.write_indexed_bam(big, REFS, recs, block_payload=60000, text=rr.rg_header(REFS, GROUPS))
    assert [int(g) for g in vb.api.bam_scan(big, pre + ".bed", groups=True)["record_groups"]] == want


def _scan_error(bam, bed, groups=True):
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.api.bam_scan(bam, bed, groups=groups)
    return ei.value.code, _abi.lib().vb2_last_error().decode()


def test_header_rules(tmp_path):
    recs, pre, bam, _, _ = _fixture(tmp_path, groups=["a", "b", "a"], name="dup")
    code, msg = _scan_error(bam, pre + ".bed")
    assert code == _abi.VB2_ERR_INVALID and "repeats the ID \"a\"" in msg
    assert len(vb.api.bam_scan(bam, pre + ".bed")["voffsets"]) == len(recs)        # ... and loads as ever when not asked
    # a header without @RG lines: no groups, every record unassigned
    nogroups = str(tmp_path / "none.bam")
    br.write_indexed_bam(nogroups, REFS, recs, block_payload=300)
    got = vb.api.bam_scan(nogroups, pre + ".bed", groups=True)
    assert got["group_ids"] == [] and set(int(g) for g in got["record_groups"]) == {_abi.VB2_BAM_NO_GROUP}
    # more than 65 535 lines
    many = str(tmp_path / "many.bam")
    br.write_indexed_bam(many, REFS, recs[:3], block_payload=60000, text=rr.rg_header(REFS, ["g%d" % i for i in range(65536)]))
    code, msg = _scan_error(many, pre + ".bed")
    assert code == _abi.VB2_ERR_INVALID and "more than 65535 @RG lines" in msg


MALFORMED = {
    "field_passes_the_end": rr.rg_field("lane1") + b"XIi" + b"\1\2",
    "unknown_type_byte": b"XXq" + b"\0\0\0\0" + rr.rg_field("lane1"),
    "z_without_terminator": rr.AUX_FIELDS["i"] + b"XZZ" + b"abc",
    "h_without_terminator": b"XHH" + b"1A",
    "b_count_passes_the_end": b"XBB" + b"i" + struct.pack("<I", 1000) + b"\0" * 8,
    "b_count_wraps": b"XBB" + b"I" + struct.pack("<I", 0xFFFFFFFF) + b"\0" * 4,
    "b_unknown_subtype": b"XBB" + b"Z" + struct.pack("<I", 0),
    "b_header_cut": rr.rg_field("lane2") + b"XBB" + b"i" + b"\1\0",
    "one_stray_byte": rr.rg_field("lane1") + b"x",
    "two_stray_bytes": rr.AUX_FIELDS["Bs"] + rr.rg_field("lane1") + b"xy",
}


def _malformed_files(tmp_path):
    """name -> (path, virtual offset of the record with the malformed field, the writer's offsets of all records)"""
    out = {}
    pre = str(tmp_path / "p")
    _write_panel(pre, MARKERS)
    for name, aux in MALFORMED.items():
        recs = _records()
        i = next(j for j, r in enumerate(recs) if r["name"] == "r5")
        recs[i]["aux"] = aux
        bam = str(tmp_path / (name + ".bam"))
        vo, _, _ = br.write_indexed_bam(bam, REFS, recs, block_payload=300, text=rr.rg_header(REFS, GROUPS))
        out[name] = (bam, vo[i], vo)
    return pre, out


def test_malformed_auxiliary_fields_name_the_record_and_load_as_ever_when_not_asked(tmp_path):
    pre, files = _malformed_files(tmp_path)
    for name, (bam, voff, vo) in files.items():
        code, msg = _scan_error(bam, pre + ".bed")
        assert code == _abi.VB2_ERR_INVALID, (name, code, msg)
        assert "record at virtual offset %d:" % voff in msg, (name, msg)
        assert [int(v) for v in vb.api.bam_scan(bam, pre + ".bed")["voffsets"]] == vo, name


def test_valid_and_malformed_files_under_the_sanitizers(tmp_path):
    """tests/bam_rg_check_main.cpp + bam_io.cpp built with -fsanitize=address,undefined and run directly over the valid
    fixtures and the malformed ones: a malformed field must end in an error code with a message, never in a read out of
    range (the sanitizers abort: -fno-sanitize-recover)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bam_rg_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "verifybamid_amd", "csrc"), os.path.join(ROOT, "tests", "bam_rg_check_main.cpp"),
           os.path.join(ROOT, "verifybamid_amd", "csrc", "bam_io.cpp"), "-lz", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    recs, pre, good, _, _ = _fixture(tmp_path, name="good")
    big = str(tmp_path / "bigblocks.bam")
    br.write_indexed_bam(big, REFS, recs, block_payload=60000, text=rr.rg_header(REFS, GROUPS))
    nogroups = str(tmp_path / "nogroups.bam")
    br.write_indexed_bam(nogroups, REFS, recs, block_payload=300)
    _, files = _malformed_files(tmp_path)
    markers = str(tmp_path / "markers.txt")
    open(markers, "w").write("".join("%s %d\n" % (c, p) for c, p, _, _ in MARKERS))
    args = [exe, markers, "4", "ok", good, "ok", big, "ok", nogroups]
    for name in sorted(files):
        args += ["aux", files[name][0]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * (3 + len(files)), (r.stdout, r.stderr[-2000:])
    want_none = sum(1 for x in recs if x["rg"] is None)
    want_sum = sum(IDS.index(x["rg"]) for x in recs if x["rg"] is not None)
    assert lines[0] == lines[2] == "groups ok %d %d %d %d" % (len(recs), want_none, len(IDS), want_sum)
    assert lines[4] == "groups ok %d %d 0 0" % (len(recs), len(recs))
    for name, first, second in zip(sorted(files), lines[6::2], lines[7::2]):
        f = first.split(" ", 3)
        assert f[:2] == ["groups", "error"] and int(f[2]) == _abi.VB2_ERR_INVALID and "virtual offset %d:" % files[name][1] in f[3], (name, first)
        assert second == "plain ok %d" % len(recs), (name, second)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])


REFUSALS = {
    "no_bam": (["--PileupFile", "absent.pileup"], "--PileupFile"),
    "no_input_bam": ([], "needs --BamFile"),
    "pileup_file": (["--BamFile", "absent.bam", "--PileupFile", "absent.pileup"], "--PileupFile"),
    "pileup_list": (["--BamFile", "absent.bam", "--PileupList", "absent.list"], "--PileupList"),
    "two_devices": (["--BamFile", "absent.bam", "--Devices", "0,1"], "more than one --Devices"),
    "confidence_interval": (["--BamFile", "absent.bam", "--ConfidenceInterval"], "--ConfidenceInterval"),
    "per_chromosome": (["--BamFile", "absent.bam", "--PerChromosome"], "--PerChromosome"),
    "bootstrap": (["--BamFile", "absent.bam", "--Bootstrap", "5"], "--Bootstrap"),
    "num_start": (["--BamFile", "absent.bam", "--NumStart", "4"], "--NumStart"),
    "line_search": (["--BamFile", "absent.bam", "--LineSearch"], "--LineSearch"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_command_line_refuses_before_any_file_is_read(case, tmp_path):
    extra, reason = REFUSALS[case]
    p = subprocess.run([EXE, "--SVDPrefix", str(tmp_path / "absent_panel"), "--Reference", "unread.fa", "--PerReadGroup",
                        "--Output", str(tmp_path / "o")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "FATAL ERROR" in p.stderr
    assert "--PerReadGroup" in p.stderr and reason in p.stderr, p.stderr
    assert "absent_panel" not in p.stderr and "absent.bam" not in p.stderr      # no file was opened
    assert not os.path.exists(str(tmp_path / "o.selfRG"))


def test_the_library_refuses_the_same_before_any_file_is_read(tmp_path):
    for kw, reason in ((dict(devices=[0, 1]), "one device"), (dict(num_start=4), "--NumStart"), (dict(line_search=True), "--LineSearch")):
        with pytest.raises(_abi.Vb2Error) as ei:
            vb.run_files(str(tmp_path / "absent_panel"), None, None, bam_path=str(tmp_path / "absent.bam"), per_read_group=True, **kw)
        assert ei.value.code == _abi.VB2_ERR_INVALID and reason in _abi.lib().vb2_last_error().decode()
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.run_files(str(tmp_path / "absent_panel"), str(tmp_path / "absent.pileup"), None, per_read_group=True)
    assert ei.value.code == _abi.VB2_ERR_INVALID and "needs --BamFile" in _abi.lib().vb2_last_error().decode()


def test_a_valid_bam_without_a_device_is_no_device(tmp_path):
    """The file, its index, its @RG lines and its records' groups are read first; then, without a GPU, both new calls end
    in VB2_ERR_NO_DEVICE, as vb2_flat_load does."""
    if _abi.lib().vb2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    recs, pre, bam, _, _ = _fixture(tmp_path)
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.api.load_bam_groups(pre, bam)
    assert ei.value.code == _abi.VB2_ERR_NO_DEVICE and b"no CPU fallback" in _abi.lib().vb2_last_error()
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.run_files(pre, None, str(tmp_path / "out"), bam_path=bam, disable_sanity=True, per_read_group=True)
    assert ei.value.code == _abi.VB2_ERR_NO_DEVICE
    # ... and a malformed header is found out before that
    dup = str(tmp_path / "dup.bam")
    br.write_indexed_bam(dup, REFS, recs, block_payload=300, text=rr.rg_header(REFS, ["a", "a"]))
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.api.load_bam_groups(pre, dup)
    assert ei.value.code == _abi.VB2_ERR_INVALID
