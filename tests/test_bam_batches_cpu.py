"""The batch cutter of the built-in BAM reader (csrc/bam_batches.cpp) without a device: a stand-alone
program (tests/bam_batches_check_main.cpp) built with -fsanitize=address,undefined cuts hand-made scans, and every batch's
(nr, nb), every record's rebased offset and group, and under --ApplyBAQ the tasks' bq_off and the extra bytes are compared
with the restatement of the cutting rule below.  The same rule is held against a load's stats["batches"] in
tests/test_bam_gpu.py.  Expected values never come from the code under test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "verifybamid_amd", "csrc")
LIMIT = 0xfff00000
NO_GROUP, NO_BQ = 0xFFFF, 0xFFFFFFFF


def var_bytes(l_read_name, n_cigar, l_seq):
    return l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq


def cut(kb, sizes):
    """the cutting rule: (batch_bytes, batch_rec, batches as lists of sizes)"""
    batch_bytes = max(max(kb, 1) << 10, max(sizes, default=0))
    batch_rec = min(max(len(sizes), 1), max(batch_bytes // 32, 1))
    out = []
    for v in sizes:
        if not out or sum(out[-1]) + v > batch_bytes or len(out[-1]) >= batch_rec:
            out.append([])
        out[-1].append(v)
    return batch_bytes, batch_rec, out


K = 1024
R1 = "1:0:0"                       # a record of one byte
CUT_CASES = {                      # name: (kb, chunks)
    "no_chunk": (1, []),
    "all_empty": (1, [[], [], []]),
    "one_record": (1, [[(10, 2, 30)]]),
    "empty_first_last_between": (1, [[], [(10, 1, 100), (10, 1, 100)], [], [(9, 0, 7)], []]),
    # 24 + 4 * 250 = 1024: alone in its batch, the next record opens a new one
    "exactly_full_alone": (1, [[(5, 0, 2), (24, 250, 0), (5, 0, 2)]]),
    # 12 + 4 * 125 = 512, twice: they share one batch, the third record does not fit
    "two_fill_exactly": (1, [[(12, 125, 0), (12, 125, 0)], [(1, 0, 0)]]),
    # 10 + 8 + 1000 + 2000 = 3018 > 1 KiB: batch_bytes is the record's own size
    "larger_than_kb": (1, [[(10, 1, 60)], [(10, 2, 2000), (10, 1, 60)], [(10, 2, 2000)]]),
    # one byte each: 1 KiB / 32 = 32 descriptors close a batch long before 1024 bytes do
    "one_byte_records": (1, [[(1, 0, 0)] * 40, [(1, 0, 0)] * 30]),
    "fewer_records_than_the_bound": (1, [[(1, 0, 0)] * 5]),
    "kb_zero_is_one": (0, [[(20, 1, 600)] * 3]),
    "two_kb": (2, [[(20, 1, 600)] * 5, [(20, 1, 601)] * 2]),
}


def _spec(chunks):
    return "|".join(",".join("%d:%d:%d" % r for r in ch) if ch else "e" for ch in chunks) if chunks else "-"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("batches") / "bam_batches_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", SRC,
           os.path.join(ROOT, "tests", "bam_batches_check_main.cpp"), os.path.join(SRC, "bam_batches.cpp"), os.path.join(SRC, "baq_host.cpp"),
           os.path.join(SRC, "fasta_io.cpp"), os.path.join(SRC, "bam_io.cpp"), "-lz", "-lpthread", "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    return out


def _run(exe, tmp_path, lines):
    cases = str(tmp_path / "cases.txt")
    open(cases, "w").write("".join(ln + "\n" for ln in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        t = ln.split(" ")
        if t[0] == "case":
            cur = out[t[1]] = dict(rc=int(t[3]), bytes=int(t[5]), rec=int(t[7]), err=" ".join(t[9:]), batches=[], copied=[])
        elif t[0] == "batch":
            keys = ("off", "grp", "kind", "bq", "extra")      # each followed by its value, or by nothing
            f = {t[k]: t[k + 1] if k + 1 < len(t) and t[k + 1] not in keys else "" for k in range(3, len(t)) if t[k] in keys}
            nums = lambda s: [int(x) for x in s.split(",")] if s else []  # noqa: E731
            cur["batches"].append(dict(nr=int(t[1]), nb=int(t[2]), off=nums(f["off"]), grp=nums(f["grp"]), kind=nums(f.get("kind", "")),
                                       bq=nums(f.get("bq", "")), extra=f.get("extra", "")))
        elif t[0] == "copied":
            cur["copied"].append(int(t[1]))
    return out


def test_the_cases_are_what_they_say():
    def shape(name):
        kb, chunks = CUT_CASES[name]
        return cut(kb, [var_bytes(*r) for ch in chunks for r in ch])

    assert shape("no_chunk")[2] == [] and shape("all_empty")[2] == []
    assert [len(b) for b in shape("exactly_full_alone")[2]] == [1, 1, 1] and sum(shape("exactly_full_alone")[2][1]) == K
    assert [len(b) for b in shape("two_fill_exactly")[2]] == [2, 1] and sum(shape("two_fill_exactly")[2][0]) == K
    bb, br, b = shape("larger_than_kb")
    assert bb == 3018 and [len(x) for x in b] == [1, 1, 1, 1]
    bb, br, b = shape("one_byte_records")
    assert (bb, br) == (K, 32) and [len(x) for x in b] == [32, 32, 6] and all(sum(x) < K for x in b)
    assert shape("fewer_records_than_the_bound")[1] == 5 and shape("kb_zero_is_one")[0] == K


def test_cutter_equals_the_restatement_under_the_sanitizers(exe, tmp_path):
    got = _run(exe, tmp_path, ["cut %s %d --BamFile %s" % (name, kb, _spec(chunks)) for name, (kb, chunks) in sorted(CUT_CASES.items())])
    assert sorted(got) == sorted(CUT_CASES)
    for name, (kb, chunks) in CUT_CASES.items():
        recs = [(var_bytes(*r), NO_GROUP if ci == 0 else ri % 3) for ci, ch in enumerate(chunks) for ri, r in enumerate(ch)]
        bb, br, want = cut(kb, [v for v, _ in recs])
        g = got[name]
        assert (g["rc"], g["bytes"], g["rec"], g["err"]) == (0, bb, br, "-"), name
        assert [(b["nr"], b["nb"]) for b in g["batches"]] == [(len(b), sum(b)) for b in want], name
        assert [b["off"] for b in g["batches"]] == [[sum(b[:i]) for i in range(len(b))] for b in want], name
        groups = iter(grp for _, grp in recs)
        assert [b["grp"] for b in g["batches"]] == [[next(groups) for _ in b] for b in want], name
        assert g["copied"] == [1] * len(want), name


@pytest.mark.parametrize("who", ["--BamFile", "vb2_baq_records"])
def test_a_record_that_passes_its_chunk_is_refused_with_the_callers_prefix(exe, tmp_path, who):
    got = _run(exe, tmp_path, ["pass short 1 %s %s" % (who, _spec([[(10, 1, 50)], [(10, 1, 50), (10, 1, 51)]]))])["short"]
    assert (got["rc"], got["err"]) == (-1, who + ": internal error: a record passes its chunk")
    assert [(b["nr"], b["nb"]) for b in got["batches"]] == []      # (all three records would have shared the one batch)


def test_four_gib_is_refused_by_the_plan_alone(exe, tmp_path):
    """batch_bytes at 0xfff00000 passes, above it is refused.  The plan alone: nothing is allocated.  A record's variable
    part is at most 255 + 4 * 65535 + 1.5 * (2^31 - 1) < 0xfff00000, so only bam_batch_kb can reach the limit, in steps of
    1 KiB: the first value above it is one KiB above."""
    assert LIMIT % K == 0 and var_bytes(255, 65535, 2 ** 31 - 1) < LIMIT
    got = _run(exe, tmp_path, ["plan at %d" % (LIMIT // K), "plan above %d" % (LIMIT // K + 1)])
    assert (got["at"]["rc"], got["at"]["bytes"], got["at"]["rec"], got["at"]["err"]) == (0, LIMIT, 1, "-")
    assert (got["above"]["rc"], got["above"]["err"]) == (-1, "--BamFile: bam_batch_kb asks for batches of 4 GiB or more")
    got = _run(exe, tmp_path, ["cut above %d vb2_baq_records %s" % (LIMIT // K + 1, _spec([[(10, 1, 50)]]))])["above"]
    assert (got["rc"], got["err"], got["batches"]) == (-1, "vb2_baq_records: bam_batch_kb asks for batches of 4 GiB or more", [])


def test_tasks_and_extra_bytes_of_a_batch(exe, tmp_path):
    """--ApplyBAQ's hook: a record with a usable BQ tag is a kind-1 task whose bq_off points at its l_seq tag bytes in the
    batch's extra bytes, in batch order and from 0 in every batch; a record without the tag, or with one that is too
    short to use, is the HMM's (kind 2) and has no bq_off.  (make_task never gives a kind-1 task without its bytes.)"""
    def bq(l_seq, r):
        return bytes(0x40 + (k + r) % 5 for k in range(l_seq)).hex()

    got = _run(exe, tmp_path, ["baq one_batch 8 5:b,4:n,3:b,6:s", "baq per_record 1 400:b,400:n,400:b"])
    one = got["one_batch"]["batches"]
    sizes = [var_bytes(200, 1, n) for n in (5, 4, 3, 6)]
    assert [(b["nr"], b["nb"]) for b in one] == [(4, sum(sizes))] and one[0]["off"] == [sum(sizes[:i]) for i in range(4)]
    assert one[0]["kind"] == [1, 2, 1, 2] and one[0]["bq"] == [0, NO_BQ, 5, NO_BQ] and one[0]["extra"] == bq(5, 0) + bq(3, 2)
    per = got["per_record"]["batches"]
    assert var_bytes(200, 1, 400) == 804 and [(b["nr"], b["nb"]) for b in per] == [(1, 804)] * 3
    assert [(b["kind"], b["bq"], b["extra"]) for b in per] == [([1], [0], bq(400, 0)), ([2], [NO_BQ], ""), ([1], [0], bq(400, 2))]
    assert got["one_batch"]["copied"] == [1] and got["per_record"]["copied"] == [1, 1, 1]
