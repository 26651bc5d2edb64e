"""CPU tests of .bam lines in a cohort's list and of the BlockInflater hook: how a line is
classified, the host-thread arithmetic, and tests/bam_inflater_check_main.cpp -- the hook, the zlib fallback and the identity
of the errors with a host-side inflater that calls the device decoder's core -- under ASan and UBSan.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
from test_bam_cpu import REFS, _mutilated, _reads  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_lines_are_classified_by_name_and_cram_magic(tmp_path):
    kind = _abi.lib().vb2_debug_list_entry_kind
    text, bam, cram = 0, 1, 2
    for name, want in (("a.bam", bam), ("/x/y.z/s.bam", bam), ("a.cram", cram), ("a.Pileup", text), ("a.pileup.gz", text),
                       ("a.bam.txt", text), ("bam", text), (".bam", text), ("a.BAM", text), ("a.bai", text)):
        assert kind(name.encode()) == want, name           # (by name alone: none of these exists)
    disguised = tmp_path / "looks_like_text.Pileup"
    disguised.write_bytes(b"CRAM\x03\x00" + b"\0" * 64)
    assert kind(str(disguised).encode()) == cram
    plain = tmp_path / "s.Pileup"
    plain.write_text("20\t100\tA\t1\t.\tI\n")
    assert kind(str(plain).encode()) == text
    # a mixed list keeps every line's own kind
    names = ["a.bam", str(plain), "c.cram", "d.bam"]
    assert [kind(n.encode()) for n in names] == [bam, text, cram, bam]


def test_a_bam_loads_pool_times_the_readers_stays_within_16():
    pool = _abi.lib().vb2_debug_cohort_bam_pool
    for t in range(1, 65):
        p = pool(t)
        assert p >= 1 and p == max(1, 16 // t)
        assert p * min(t, 16) <= 16            # (beyond 16 readers the pool is the one thread the reader itself is)


def test_tunables_of_the_feature_and_their_defaults():
    assert _abi.get_tunable("bam_inflate") == 0            # --BamFile and vb2_flat_load keep zlib on the host pool
    assert _abi.get_tunable("cohort_bam_inflight") == 4
    assert _abi.lib().vb2_abi_version() == 7


def test_device_entry_points_without_a_device_fail_loudly(tmp_path):
    if _abi.lib().vb2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import verifybamid_amd as vb
    blk = br.bgzf_block(b"hello")
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.api.bgzf_inflate(blk)
    assert ei.value.code == _abi.VB2_ERR_NO_DEVICE
    st = _abi.BamStats()
    assert _abi.lib().vb2_cohort_bam_stats(0, C.byref(st)) == _abi.VB2_ERR_INVALID


def test_hook_fallback_and_error_identity_under_the_sanitizers(tmp_path):
    """bam_io.cpp's scan with a BlockInflater that runs bgzf_inflate_core.h on the host: the same chunks, records, codes and
    messages as without one over two valid files and the 31 broken ones of tests/test_bam_cpu.py; a block the inflater
    refuses goes through zlib, and so does one it accepted with spoilt bytes: its CRC32 finds it out."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bam_inflater_check")
    csrc = os.path.join(ROOT, "verifybamid_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
           os.path.join(ROOT, "tests", "bam_inflater_check_main.cpp"), os.path.join(csrc, "bam_io.cpp"), "-lz", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    rng = np.random.default_rng(7)
    recs = _reads(rng, 60, near=[5000, 16384, 131072])
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    good = str(tmp_path / "good.bam")
    vo, ve, _ = br.write_indexed_bam(good, REFS, recs)
    big = str(tmp_path / "bigblocks.bam")
    br.write_indexed_bam(big, REFS, recs, block_payload=60000)
    markers = str(tmp_path / "markers.txt")
    open(markers, "w").write("chrA 5000\nchrA 16384\nchrB 131072\nchrC 131073\nchrZ 9\n")
    broken = _mutilated(str(tmp_path), good, recs, vo, ve)
    files = [good, big] + [broken[k] for k in sorted(broken)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, markers, "4"] + files, capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(files) and all(l.startswith("same ") for l in lines), (r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    f0, f1 = lines[0].split(), lines[1].split()
    assert f0[1] == "0" and int(f0[2]) > 10 and f0[3] == "0" and int(f0[4]) == int(f0[2]) // 2 and f0[5] == "ok"
    assert f1[1] == "0" and f1[5:] == f0[5:]                          # the same records whatever the block size
    by_name = dict(zip(sorted(broken), lines[2:]))
    # the core refuses what it cannot inflate to ISIZE bytes, and zlib's message stands
    for name, word in (("deflate_garbage", "corrupt deflate stream"), ("isize_too_large", "ISIZE says"), ("isize_too_small", "more than its ISIZE"),
                       ("crc_mismatch", "CRC32 mismatch")):
        f = by_name[name].split(" ", 5)
        assert int(f[1]) == _abi.VB2_ERR_INVALID and word in f[5], by_name[name]
        assert (int(f[3]) >= 1) == (name != "crc_mismatch"), by_name[name]       # a wrong CRC32 field is not the decoder's to see
