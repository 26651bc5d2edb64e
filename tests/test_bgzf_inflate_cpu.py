"""The DEFLATE decoder of the device inflate on the CPU (verifybamid_amd/csrc/bgzf_inflate_core.h): the
program tests/bgzf_inflate_check_main.cpp built with -fsanitize=address,undefined and run over a corpus it makes with zlib,
against zlib; and the kernel's budget from the code object's notes.  No GPU."""
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
import bgzf_ref as bz  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "verifybamid_amd", "csrc")


def bam_record_bytes():
    """a few hundred BAM records back to back, as the writer of tests/bam_ref.py encodes them"""
    rng = np.random.default_rng(1)
    out = b""
    for i in range(300):
        n = int(rng.integers(20, 120))
        out += br.encode_record(br.rec("q%d" % i, 0, 1000 + 7 * i, "%dM" % n, "".join(rng.choice(list("ACGT"), size=n)),
                                       [int(x) for x in rng.integers(0, 41, size=n)]))
    return out


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("bgzf_check")
    exe = str(tmp / "bgzf_inflate_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "bgzf_inflate_check_main.cpp"), "-lz", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    rec = str(tmp / "records.bin")
    open(rec, "wb").write(bam_record_bytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, rec], capture_output=True, text=True, timeout=600, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def test_corpus_equals_zlib_within_the_step_budget(check_run):
    lines = [l.split() for l in check_run.stdout.splitlines() if l.startswith("stream ")]
    assert len(lines) == 5 * 11 * 4 * 4 * 3 + 3
    seen = set()
    for f in lines:
        _, content, n, level, strategy, flush, raw_len, status, steps, budget, equal = f
        assert int(status) == 0 and int(equal) == 1 and int(steps) <= int(budget), f
        assert int(budget) == 8 * int(raw_len) + int(n) + 64
        seen.add((content, int(n), int(level), strategy, flush))
    assert {s[0] for s in seen} == set(bz.CONTENTS) | {"hand_dist32768", "hand_one_dist", "hand_empty_dist"}
    assert {s[1] for s in seen if s[0] in bz.CONTENTS} == set(bz.LENGTHS)
    assert {s[2] for s in seen if s[0] in bz.CONTENTS} == set(bz.LEVELS)
    assert check_run.stdout.splitlines()[-1] == "bad 0" and check_run.returncode == 0


def test_the_corpus_reaches_every_case_the_decoder_has(check_run):
    """A condition on the inputs, not on the code.  With zlib 1.2.11 alone: every block type, an empty stored block that
    starts off a byte boundary (the flushes), the longest match, overlapping copies, all three repeat symbols.  zlib's
    deflate keeps its matches within 32 768 - 262 bytes and gives every distance tree two codes at least, so distance
    32 768, a distance tree of one code and one of none come from the three hand-assembled streams."""
    line = next(l for l in check_run.stdout.splitlines() if l.startswith("census "))
    f = line.split()
    c = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
    print(line)
    assert c["stored"] > 0 and c["fixed"] > 0 and c["dynamic"] > 0
    assert c["empty_stored_off_byte"] > 0
    assert c["longest_match"] == 258 and c["largest_distance"] == 32768 and c["overlapping"] > 0
    assert c["rep16"] > 0 and c["rep17"] > 0 and c["rep18"] > 0
    assert c["one_code_dist"] > 0 and c["empty_dist"] > 0


def test_mutilated_streams_stay_within_bounds_and_budget(check_run):
    out = check_run.stdout.splitlines()
    smalls = {l.split()[1]: l.split() for l in out if l.startswith("small ")}
    mine = bz.small_streams()
    kinds = {"stored": "stored", "fixed": "fixed", "dynamic": "dynamic"}
    for name, f in smalls.items():
        assert int(f[2]) <= 200 and int(f[3]) == 0
        types = {f[4]: int(f[5]), f[6]: int(f[7]), f[8]: int(f[9])}
        assert types == {k: int(k == kinds[name]) for k in types}, (name, types)       # one block, of its own kind
        assert f[10] == mine[name][0].hex(), "tests/bgzf_ref.py builds another %s stream than the check program" % name
    muts = [l.split() for l in out if l.startswith("mut ")]
    assert len(muts) == sum(9 * len(raw) for raw, _ in mine.values())                    # every bit flipped, every prefix
    table = {}
    for _, name, kind, index, status, steps, budget, zok, equal in muts:
        assert int(steps) <= int(budget), (name, kind, index)
        assert int(equal) != 0, (name, kind, index)       # status 0 and zlib succeeds too: the same bytes
        table[(name, kind, int(index))] = int(status)
    # what the GPU test gives the kernel as broken input is decided here
    for name, kind, index, status in bz.MUTILATED:
        assert status != 0 and table[(name, kind, index)] == status, (name, kind, index, table[(name, kind, index)])
    assert len(bz.MUTILATED) == 20 and len({m[3] for m in bz.MUTILATED}) == 9


def test_python_side_streams_are_what_they_claim():
    """tests/bgzf_ref.py on its own: zlib inflates its hand-assembled streams to their plain bytes, and a wrapped block is BGZF."""
    for name, raw, plain in bz.handmade():
        assert zlib.decompress(raw, -15) == plain, name
    for name, (raw, plain) in bz.small_streams().items():
        assert zlib.decompress(raw, -15) == plain and len(raw) <= 200
    blk = bz.bgzf_wrap(*bz.small_streams()["dynamic"])
    assert zlib.decompress(blk, 31) == bz.small_streams()["dynamic"][1]
    assert bz.bgzf_wrap(bz.deflate_raw(bz.lcg(5, 65536), 0, zlib.Z_DEFAULT_STRATEGY), bz.lcg(5, 65536)) is None


def test_inflate_kernel_uses_no_scratch():
    """bgzf_inflate_kernel from the code object's notes: no scratch memory (the decoder keeps what it indexes in LDS), its
    window and tables in 66 616 bytes of LDS -- two workgroups per CU --; VGPRs printed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_diff
    import re
    import tempfile
    lib = os.path.join(ROOT, "verifybamid_amd", "libvb2.so")
    if not os.path.exists(lib):
        pytest.skip("libvb2.so is not built")
    readelf = isa_diff.LLVM + "llvm-readelf"
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    found = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa_diff.code_object(lib, tmp):
            txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
            for entry in re.split(r"\n  - ", txt):
                if "bgzf_inflate_kernel" not in entry or ".vgpr_count" not in entry:
                    continue
                found.append({k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|"
                                                                r"vgpr_spill_count|sgpr_spill_count):\s*(\d+)", entry)})
    assert len(found) == 1, found
    print(found[0])
    assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0
    assert found[0]["group_segment_fixed_size"] == 65536 + 1080
    assert 2 * found[0]["group_segment_fixed_size"] <= 160 * 1024
