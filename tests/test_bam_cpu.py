"""CPU tests of the built-in BAM reader's host stage (verifybamid_amd/csrc/bam_io.cpp): BGZF, the
header, the .bai index, the record chain and their validation -- no GPU.  Files come from the writer of tests/bam_ref.py
(blocks of 300 payload bytes: records straddle them); expectations from its pileup_ref."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chrA", 400000), ("chrB", 400000), ("chrC", 400000)]


def _write_panel(pre, rows):
    """rows: (chr, pos1, ref, alt)"""
    with open(pre + ".bed", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(pre + ".UD", "w") as fh:
        for i in range(len(rows)):
            fh.write("%g %g\n" % (0.01 * (i % 7 - 3), 0.02 * (i % 5 - 2)))
    with open(pre + ".mu", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s:%d_%s/%s 0.5\n" % (c, p, r, a))


def _reads(rng, n_per_seq, seqs=(0, 1, 2), near=()):
    """simple reads of 20..120 bases scattered over the sequences, plus reads around the positions in `near`"""
    recs = []
    for t in seqs:
        starts = sorted(int(x) for x in rng.integers(0, 300000, size=n_per_seq))
        starts += [max(0, p - int(rng.integers(0, 90))) for p in near for _ in range(3)]
        for s in sorted(starts):
            n = int(rng.integers(20, 120))
            recs.append(br.rec("q%d_%d" % (t, len(recs)), t, s, "%dM" % n, "".join(rng.choice(list("ACGT"), size=n)),
                               [int(x) for x in rng.integers(0, 41, size=n)]))
    return recs


def _covering(records, refs, rows, opts=None):
    """indices of the records that pileup_ref's rules say span one of the rows' positions (read filters aside)"""
    tid_of = {name: t for t, (name, _) in reversed(list(enumerate(refs)))}
    want = set()
    for c, p, _, _ in rows:
        if c not in tid_of:
            continue
        for i, r in enumerate(records):
            if r["tid"] == tid_of[c] and r["pos"] >= 0 and br.covered(r, p - 1) is not None:
                want.add(i)
    return want


def test_writer_and_parser_agree(tmp_path):
    """The test side's own tools first: what write_bam reports as virtual offsets is what parse_bam finds."""
    rng = np.random.default_rng(1)
    recs = _reads(rng, 40)
    path = str(tmp_path / "a.bam")
    vo, ve, blocks = br.write_bam(path, REFS, recs)
    refs, text, parsed = br.parse_bam(path)
    assert refs == REFS and "@SQ\tSN:chrB" in text
    assert [p["voffset"] for p in parsed] == vo
    assert [(p["name"], p["pos"], p["seq"], p["qual"]) for p in parsed] == [(r["name"], r["pos"], r["seq"], r["qual"]) for r in recs]
    assert len(blocks) > 20                     # records straddle blocks: 300 payload bytes each
    assert vo == sorted(vo) and all(a < b for a, b in zip(vo, ve))


def test_scan_fetches_every_covering_record_once_and_uses_the_index(tmp_path):
    rng = np.random.default_rng(2)
    near = [16384, 16385, 32768, 131072, 131073, 262144, 5, 77777]
    recs = _reads(rng, 120, near=near)
    # records in higher-level bins: they cross multiples of 16 384 and of 131 072
    recs += [br.rec("span14", 1, 16380, "10M", "ACGTACGTAC", [30] * 10), br.rec("span17", 1, 131068, "3M2D5M", "ACGTACGT", [30] * 8),
             br.rec("long", 1, 120000, "6000M", "A" * 6000, [20] * 6000)]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    rows = [("chrB", p, "A", "C") for p in near + [16383, 131070, 125000, 250001]]
    pre = str(tmp_path / "p")
    _write_panel(pre, rows)
    bam = str(tmp_path / "s.bam")
    vo, ve, blocks = br.write_indexed_bam(bam, REFS, recs)
    got = vb.api.bam_scan(bam, pre + ".bed")
    fetched = [int(x) for x in got["voffsets"]]
    assert fetched == sorted(fetched) and len(set(fetched)) == len(fetched)
    want = _covering(recs, REFS, rows)
    assert len(want) > 20
    assert {vo[i] for i in want} <= set(fetched)
    # the index is used: nothing comes from a block that holds only records of another sequence
    tid_of_voffset = {v: r["tid"] for v, r in zip(vo, recs)}
    assert all(tid_of_voffset[v] == 1 for v in fetched)
    st = got["stats"]
    assert st["records_kept"] == len(fetched) and st["chunks"] >= 1
    assert st["records_seen"] < len(recs), "the reader walked the whole file"
    assert got["sample"] == "DefaultSampleName"


def test_sequence_of_the_bed_missing_from_the_header_and_empty_result(tmp_path):
    rng = np.random.default_rng(3)
    recs = _reads(rng, 30)
    pre = str(tmp_path / "p")
    _write_panel(pre, [("chrZ", 100, "A", "C"), ("chrA", 399999, "G", "T")])
    bam = str(tmp_path / "s.bam")
    br.write_indexed_bam(bam, REFS, recs)
    got = vb.api.bam_scan(bam, pre + ".bed")
    assert len(got["voffsets"]) == 0


def test_index_beside_the_stem(tmp_path):
    rng = np.random.default_rng(4)
    recs = _reads(rng, 30, near=[5000])
    pre = str(tmp_path / "p")
    _write_panel(pre, [("chrA", 5000, "A", "C")])
    bam = str(tmp_path / "s.bam")
    vo, ve, _ = br.write_bam(bam, REFS, recs)
    br.write_bai(str(tmp_path / "s.bai"), len(REFS), recs, vo, ve)
    assert len(vb.api.bam_scan(bam, pre + ".bed")["voffsets"]) >= 3


def _scan_error(bam, bed):
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.api.bam_scan(bam, bed)
    return ei.value.code, _abi.lib().vb2_last_error().decode()


def test_sample_name_rules(tmp_path):
    rng = np.random.default_rng(5)
    recs = _reads(rng, 10, near=[5000])
    pre = str(tmp_path / "p")
    _write_panel(pre, [("chrA", 5000, "A", "C")])
    sq = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
    one = str(tmp_path / "one.bam")
    br.write_indexed_bam(one, REFS, recs, text="@HD\tVN:1.6\n" + sq + "@RG\tID:a\tSM:NA12878\tPL:x\n@RG\tID:b\tSM:NA12878\n")
    assert vb.api.bam_scan(one, pre + ".bed")["sample"] == "NA12878"
    two = str(tmp_path / "two.bam")
    br.write_indexed_bam(two, REFS, recs, text=sq + "@RG\tID:a\tSM:NA12878\n@RG\tID:b\tSM:NA12891\n")
    code, msg = _scan_error(two, pre + ".bed")
    assert code == _abi.VB2_ERR_INVALID and "contains more than 1 sample" in msg


def test_missing_index_and_cram_and_unreadable(tmp_path):
    rng = np.random.default_rng(6)
    recs = _reads(rng, 10, near=[5000])
    pre = str(tmp_path / "p")
    _write_panel(pre, [("chrA", 5000, "A", "C")])
    bam = str(tmp_path / "noidx.bam")
    br.write_bam(bam, REFS, recs)
    code, msg = _scan_error(bam, pre + ".bed")
    assert code == _abi.VB2_ERR_IO and "fail to load index for " + bam in msg
    cram = str(tmp_path / "x.cram")
    open(cram, "wb").write(b"CRAM\x03\x00" + b"\0" * 64)
    code, msg = _scan_error(cram, pre + ".bed")
    assert code != 0 and "CRAM" in msg
    code, msg = _scan_error(str(tmp_path / "absent.bam"), pre + ".bed")
    assert code == _abi.VB2_ERR_IO
    assert "cannot open " + str(tmp_path / "absent.bam") + " (built-in BAM reader; this build has no htslib: no CRAM, no BAQ, no mapQ cap)" in msg


def test_long_cigar_placeholder_is_skipped_and_counted(tmp_path):
    recs = [br.rec("plain", 0, 4990, "20M", "A" * 20, [30] * 20),
            br.rec("huge", 0, 4995, "30S40N", "C" * 30, [30] * 30)]          # "<l_seq>S<reference length>N": the CIGAR is in CG
    pre = str(tmp_path / "p")
    _write_panel(pre, [("chrA", 5000, "A", "C")])
    bam = str(tmp_path / "s.bam")
    vo, _, _ = br.write_indexed_bam(bam, REFS, recs)
    got = vb.api.bam_scan(bam, pre + ".bed")
    assert [int(v) for v in got["voffsets"]] == [vo[0]] and got["stats"]["long_cigar_skipped"] == 1


# ------------------------------------------------------------------ malformed input, under the host sanitizers

def _mutilated(tmp, good_bam, recs, vo, ve):
    """name -> path of a broken copy (its index beside it).  Every one must end in an error code with a message."""
    raw = open(good_bam, "rb").read()
    bai = open(good_bam + ".bai", "rb").read()
    out = {}

    def put(name, bam_bytes=None, bai_bytes=None):
        p = os.path.join(tmp, name + ".bam")
        open(p, "wb").write(raw if bam_bytes is None else bam_bytes)
        open(p + ".bai", "wb").write(bai if bai_bytes is None else bai_bytes)
        out[name] = p

    # block table of the good file
    offs, o = [], 0
    while o < len(raw):
        offs.append(o)
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1
    first_data = vo[0] >> 16                                   # the block of the first record
    k = offs.index(first_data)
    blk = lambda i: (offs[i], offs[i + 1] if i + 1 < len(offs) else len(raw))

    def patch(at, data):
        b = bytearray(raw)
        b[at:at + len(data)] = data
        return bytes(b)

    put("truncated_mid_block", raw[:offs[k + 3] + 11])
    put("truncated_in_header", raw[:9])
    # ... and inside the last chunk that is read, behind the block it starts in (chrC's marker is 131 073)
    cov = [j for j, r in enumerate(recs) if r["tid"] == 2 and r["pos"] <= 131072 < br.record_end(r)]
    assert len(cov) >= 3 and (ve[cov[-1]] >> 16) > (vo[cov[0]] >> 16)
    put("truncated_in_last_chunk", raw[:(ve[cov[-1]] >> 16) - 9])
    put("bsize_beyond_eof", patch(offs[k + 1] + 16, struct.pack("<H", 65535)))
    put("bad_gzip_magic", patch(offs[k + 1], b"\x1f\x8c"))
    put("no_extra_field", patch(offs[k + 1] + 3, b"\x00"))
    put("no_bc_subfield", patch(offs[k + 1] + 12, b"XY"))
    put("bc_wrong_length", patch(offs[k + 1] + 14, struct.pack("<H", 3)))
    put("bsize_too_small", patch(offs[k + 1] + 16, struct.pack("<H", 10)))
    b0, b1 = blk(k + 1)
    put("crc_mismatch", patch(b1 - 8, struct.pack("<I", (struct.unpack_from("<I", raw, b1 - 8)[0] ^ 0x5a5a) & 0xffffffff)))
    put("isize_too_large", patch(b1 - 4, struct.pack("<I", struct.unpack_from("<I", raw, b1 - 4)[0] + 7)))
    put("isize_too_small", patch(b1 - 4, struct.pack("<I", struct.unpack_from("<I", raw, b1 - 4)[0] - 7)))
    put("isize_huge", patch(b1 - 4, struct.pack("<I", 1 << 20)))
    put("deflate_garbage", patch(b0 + 18, b"\xff" * 24))
    put("bam_magic", br.bgzf_block(b"BAX\1" + b"\0" * 40) + raw[offs[1]:])
    put("negative_l_text", br.bgzf_block(b"BAM\1" + struct.pack("<i", -5) + b"\0" * 40) + raw[offs[1]:])
    put("header_n_ref_mismatch", None, bai[:4] + struct.pack("<i", len(REFS) + 1) + bai[8:])
    put("bai_magic", None, b"BAJ\1" + bai[4:])
    put("bai_truncated", None, bai[:len(bai) // 2])
    put("bai_truncated_in_counts", None, bai[:10])
    put("bai_negative_bins", None, bai[:8] + struct.pack("<i", -3) + bai[12:])
    # chunk offsets beyond the file: every chunk of the index moved up by 2^40
    moved = bytearray(bai)
    p = 8
    for _ in range(len(REFS)):
        n_bin = struct.unpack_from("<i", bai, p)[0]
        p += 4
        for _ in range(n_bin):
            n_chunk = struct.unpack_from("<i", bai, p + 4)[0]
            p += 8
            for _ in range(n_chunk):
                a, e = struct.unpack_from("<QQ", bai, p)
                struct.pack_into("<QQ", moved, p, a + (1 << 56), e + (1 << 56))
                p += 16
        n_intv = struct.unpack_from("<i", bai, p)[0]
        p += 4 + 8 * n_intv
    put("chunks_beyond_the_file", None, bytes(moved))

    # records rewritten: the file is built again with one field of one covering record forced
    def rewrite(name, mutate):
        enc = [br.encode_record(r) for r in recs]
        i = next(j for j, r in enumerate(recs) if r["tid"] == 0 and r["pos"] <= 4999 < br.record_end(r))
        e = bytearray(enc[i])
        mutate(e)
        enc[i] = bytes(e)
        p = os.path.join(tmp, name + ".bam")
        vo2, ve2, _ = br.write_bam(p, REFS, recs, encoded=enc)
        br.write_bai(p + ".bai", len(REFS), recs, vo2, ve2)
        out[name] = p

    rewrite("block_size_negative", lambda e: struct.pack_into("<i", e, 0, -8))
    rewrite("block_size_below_fixed_part", lambda e: struct.pack_into("<i", e, 0, 20))
    rewrite("block_size_oversized", lambda e: struct.pack_into("<i", e, 0, 0x7ffffff0))
    rewrite("l_read_name_zero", lambda e: struct.pack_into("<B", e, 12, 0))
    rewrite("n_cigar_exceeds_record", lambda e: struct.pack_into("<H", e, 16, 60000))
    rewrite("l_seq_exceeds_record", lambda e: struct.pack_into("<i", e, 20, 100000))
    rewrite("l_seq_negative", lambda e: struct.pack_into("<i", e, 20, -1))
    rewrite("tid_outside_header", lambda e: struct.pack_into("<i", e, 4, 7))
    return out


def test_malformed_files_end_in_error_codes_under_the_sanitizers(tmp_path):
    """tests/bam_io_check_main.cpp + bam_io.cpp built with -fsanitize=address,undefined and run directly over the valid
    fixtures and 31 broken ones: every broken file must give an error code with a message; a sanitizer report (the
    sanitizers abort: -fno-sanitize-recover) fails the test."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bam_io_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "verifybamid_amd", "csrc"), os.path.join(ROOT, "tests", "bam_io_check_main.cpp"),
           os.path.join(ROOT, "verifybamid_amd", "csrc", "bam_io.cpp"), "-lz", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    rng = np.random.default_rng(7)
    recs = _reads(rng, 60, near=[5000, 16384, 131072])
    recs.append(br.rec("noqual", 0, 4980, "10M5I10M2D10M", "ACGTN" * 7, None))
    recs.append(br.rec("empty", 0, 4990, "20M", "", []))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    good = str(tmp_path / "good.bam")
    vo, ve, _ = br.write_indexed_bam(good, REFS, recs)
    markers = str(tmp_path / "markers.txt")
    open(markers, "w").write("chrA 5000\nchrA 16384\nchrB 131072\nchrC 131073\nchrZ 9\n")
    big = str(tmp_path / "bigblocks.bam")
    br.write_indexed_bam(big, REFS, recs, block_payload=60000)
    broken = _mutilated(str(tmp_path), good, recs, vo, ve)
    assert len(broken) >= 20
    args = [exe, markers, "4", "ok", good, "ok", big]
    for name in sorted(broken):
        args += ["fail", broken[name]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 + len(broken), (r.stdout, r.stderr[-2000:])
    assert lines[0].startswith("ok ") and lines[1].startswith("ok ")
    assert lines[0].split()[1:4] == lines[1].split()[1:4], "the same records whatever the block size"
    for name, line in zip(sorted(broken), lines[2:]):
        f = line.split(" ", 2)
        assert f[0] == "error" and int(f[1]) in (_abi.VB2_ERR_IO, _abi.VB2_ERR_INVALID) and len(f) == 3 and f[2].strip(), (name, line)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])


def test_a_valid_bam_without_a_device_is_no_device(tmp_path):
    """The file and its index are read first; then, without a GPU, the load ends in VB2_ERR_NO_DEVICE -- there is no CPU
    pileup to fall back to."""
    if _abi.lib().vb2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    rng = np.random.default_rng(8)
    recs = _reads(rng, 10, near=[5000])
    pre = str(tmp_path / "p")
    _write_panel(pre, [("chrA", 5000, "A", "C"), ("chrB", 7000, "G", "T")])
    bam = str(tmp_path / "s.bam")
    br.write_indexed_bam(bam, REFS, recs)
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.api.load_bam(pre, bam)
    assert ei.value.code == _abi.VB2_ERR_NO_DEVICE
    assert b"no CPU fallback" in _abi.lib().vb2_last_error()
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.run_files(pre, None, str(tmp_path / "out"), bam_path=bam, disable_sanity=True)
    assert ei.value.code == _abi.VB2_ERR_NO_DEVICE
