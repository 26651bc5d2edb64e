"""GPU tests of .bam lines in a cohort's list and of the device inflate inside the BAM reader (tunable bam_inflate;
DESIGN.md section 21).  What a BAM line must give is what the same sample gives as its --OutputPileup text -- bitwise --
and the reference's golden files; what bam_inflate = 1 must give is what bam_inflate = 0 gives."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
from test_bam_gpu import REFS, _scenario  # noqa: E402

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
HAPMAP = os.path.join("hapmap", "hapmap_3.3.b37.dat")
COUNTERS = ("blocks", "bytes_inflated", "chunks", "records_seen", "records_kept", "long_cigar_skipped", "batches", "entries", "sites",
            "empty_sites", "pairs_resolved", "capped_sites")


# ------------------------------------------------------------------ --BamFile with the tunable

@pytest.fixture(scope="module")
def scenario458(tmp_path_factory):
    """the 458-read file of tests/test_bam_gpu.py's recipe, in blocks of 300 bytes"""
    d = tmp_path_factory.mktemp("bam458")
    recs, rows, _ = _scenario()
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
    br.write_indexed_bam(bam, REFS, recs, block_payload=300)
    return dict(pre=pre, bam=bam, dir=str(d), recs=recs, rows=rows)


def _load_both(pre, bam, tunable, **kw):
    tunable("bam_inflate", 0)
    host = vb.api.load_bam(pre, bam, **kw)
    tunable("bam_inflate", 1)
    vb.api.bgzf_inflate_stats(reset=True)
    dev = vb.api.load_bam(pre, bam, **kw)
    return host, dev, vb.api.bgzf_inflate_stats(reset=True)


def _same_load(host, dev):
    assert list(host["read_off"]) == list(dev["read_off"]) and host["bases"] == dev["bases"] and host["quals"] == dev["quals"]
    assert (host["num_site"], host["num_bases"], host["avg_depth"]) == (dev["num_site"], dev["num_bases"], dev["avg_depth"])
    assert {k: host["stats"][k] for k in COUNTERS} == {k: dev["stats"][k] for k in COUNTERS}


@gpu
def test_load_with_device_inflate_equals_host_inflate(scenario458, tunable):
    host, dev, st = _load_both(scenario458["pre"], scenario458["bam"], tunable)
    print(st)
    _same_load(host, dev)
    assert host["num_bases"] == br.pileup_ref(scenario458["recs"], REFS, scenario458["rows"], {})["num_bases"] > 300
    # the planned blocks went through the kernel, and it refused none of them
    assert st["blocks"] > 100 and st["refused"] == 0 and st["bytes_inflated"] > 0


def _pileup_lines(golden_dir, name, ref_of):
    from oracle import refio
    lines = []
    for line in open(os.path.join(golden_dir, name)):
        t = line.split()
        if not t or (t[0], int(t[1])) not in ref_of:
            continue
        b, q = refio.parse_pileup_seq(t[4] if len(t) > 4 else "", t[5] if len(t) > 5 else "")
        lines.append((t[0], int(t[1]), b, q))
    return lines


def _bam_from_lines(path, lines, ref_of, payload, sample=None):
    """one read per parsed base (bam_ref.records_from_pileup), in blocks of `payload` bytes; sample: an @RG line with that SM:"""
    chroms = sorted({c for c, _, _, _ in lines})
    refs = [(c, 1 << 28) for c in chroms]
    recs = br.records_from_pileup(lines, ref_of, {c: i for i, c in enumerate(chroms)})
    text = None
    if sample is not None:
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@RG\tID:rg1\tSM:%s\tPL:x\n" % sample
    br.write_indexed_bam(path, refs, recs, block_payload=payload, text=text)
    return path


@gpu
@pytest.mark.parametrize("payload", [300, 60000])
def test_golden_pileup_as_bam_with_device_inflate(golden_dir, tmp_path, tunable, payload):
    hap = os.path.join(golden_dir, HAPMAP)
    ref_of = {(c, p): ref for c, p, ref, _ in br.read_bed_rows(hap + ".bed")}
    lines = _pileup_lines(golden_dir, os.path.join("expected", "result.Pileup"), ref_of)
    bam = _bam_from_lines(str(tmp_path / "g.bam"), lines, ref_of, payload)
    host, dev, st = _load_both(hap, bam, tunable)
    _same_load(host, dev)
    assert host["num_bases"] == 71 and st["blocks"] >= 1 and st["refused"] == 0


def _blocks(raw):
    offs, o = [], 0
    while o < len(raw):
        offs.append(o)
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1
    return offs + [len(raw)]


@gpu
@pytest.mark.parametrize("what", ["crc", "deflate"])
def test_a_corrupt_block_ends_in_the_same_code_and_message(scenario458, tmp_path, tunable, what):
    raw = bytearray(open(scenario458["bam"], "rb").read())
    offs = _blocks(raw)
    k = len(offs) // 2                                   # a block in the middle of the records
    if what == "crc":
        raw[offs[k + 1] - 8] ^= 0x5A
    else:
        raw[offs[k] + 18 + 7] ^= 0x10
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    open(bad + ".bai", "wb").write(open(scenario458["bam"] + ".bai", "rb").read())
    seen = []
    for setting in (0, 1):
        tunable("bam_inflate", setting)
        with pytest.raises(_abi.Vb2Error) as ei:
            vb.api.load_bam(scenario458["pre"], bad)
        seen.append((ei.value.code, _abi.lib().vb2_last_error().decode()))
    print(seen)
    assert seen[0] == seen[1] and seen[0][0] == _abi.VB2_ERR_INVALID
    assert ("BGZF block at %d: " % offs[k]) in seen[0][1]


# ------------------------------------------------------------------ the cohort

@pytest.fixture(scope="module")
def trio(tmp_path_factory):
    """Three samples from records_from_pileup against the hapmap panel: a = the golden result.Pileup (300-byte blocks, @RG
    SM:SampleA), b = the golden long-read pileup (300), c = a's lines with bases and qualities reversed and every third base
    an alternate T (60 000-byte blocks); each also as the text its --BamFile --OutputPileup run writes."""
    golden = os.path.join(ROOT, "tests", "golden")
    d = tmp_path_factory.mktemp("trio")
    hap = os.path.join(golden, HAPMAP)
    ref_of = {(c, p): ref for c, p, ref, _ in br.read_bed_rows(hap + ".bed")}
    la = _pileup_lines(golden, os.path.join("expected", "result.Pileup"), ref_of)
    lb = _pileup_lines(golden, "test.LongRead.pileup", ref_of)
    lc = []
    for c, p, b, q in la:
        bb = "".join("T" if i % 3 == 2 else x for i, x in enumerate(b[::-1]))
        lc.append((c, p, bb, q[::-1]))
    out = dict(dir=str(d), hap=hap, bam={}, text={}, single={}, lines=dict(a=la, b=lb, c=lc))
    for name, lines, payload in (("a", la, 300), ("b", lb, 300), ("c", lc, 60000)):
        out["bam"][name] = _bam_from_lines(str(d / (name + ".bam")), lines, ref_of, payload, sample="Sample" + name.upper())
    return out


@pytest.fixture(scope="module")
def trio_runs(trio):
    """the three --BamFile --OutputPileup runs (their .Pileup is the text form of the samples), then the cohort over the three
    text files: what every BAM line must reproduce"""
    d = trio["dir"]
    for name in "abc":
        pre = os.path.join(d, "single_" + name)
        trio["single"][name] = vb.run_files(trio["hap"], None, pre, num_pc=2, disable_sanity=True, output_pileup=True, bam_path=trio["bam"][name])
        trio["text"][name] = pre + ".Pileup"
    outs = [os.path.join(d, "text_" + n) for n in "abc"]
    res = vb.run_cohort_files(trio["hap"], [trio["text"][n] for n in "abc"], outs, num_pc=2, disable_sanity=True)
    assert [r["status"] for r in res] == [0, 0, 0]
    trio["text_res"], trio["text_outs"] = res, outs
    return trio


def _same_estimate(x, y):
    for k in ("alpha", "llk0", "llk1", "num_eval", "converged", "num_site", "num_bases", "avg_depth", "num_marker"):
        assert x[k] == y[k], (k, x[k], y[k])
    assert np.array_equal(x["pc"], y["pc"]) and np.array_equal(x["pc2"], y["pc2"])


@gpu
@pytest.mark.parametrize("inflate", [0, 1])
def test_mixed_list_equals_the_text_cohort_bitwise(trio_runs, golden_dir, tunable, inflate):
    t = trio_runs
    tunable("bam_inflate", inflate)
    vb.api.bgzf_inflate_stats(reset=True)
    outs = [os.path.join(t["dir"], "mixed%d_%s" % (inflate, n)) for n in "abc"]
    res = vb.run_cohort_files(t["hap"], [t["bam"]["a"], t["text"]["b"], t["bam"]["c"]], outs, num_pc=2, disable_sanity=True, output_pileup=True)
    st = vb.api.bgzf_inflate_stats(reset=True)
    assert [r["status"] for r in res] == [0, 0, 0]
    for got, want in zip(res, t["text_res"]):
        _same_estimate(got, want)
    assert (st["blocks"] > 0) == (inflate == 1) and st["refused"] == 0
    # the golden files, and what only a BAM knows
    assert open(outs[0] + ".Ancestry").read() == open(os.path.join(golden_dir, "expected", "result.Ancestry")).read()
    row = open(outs[0] + ".selfSM").read().splitlines()[1].split("\t")
    assert row[0] == "SampleA" and row[4] == "71"
    row_c = open(outs[2] + ".selfSM").read().splitlines()[1].split("\t")
    assert row_c[0] == "SampleC" and row_c[4] == str(res[2]["num_bases"])
    # the text sample's files are what they are in a cohort of text files
    for ext in (".selfSM", ".Ancestry"):
        assert open(outs[1] + ext).read() == open(t["text_outs"][1] + ext).read()
    assert open(outs[1] + ".selfSM").read().splitlines()[1].split("\t")[:5:4] == ["DefaultSampleName", "NA"]
    # <prefix>.Pileup of a BAM sample is the --BamFile --OutputPileup file
    for i, n in ((0, "a"), (2, "c")):
        assert open(outs[i] + ".Pileup").read() == open(t["text"][n]).read()
        assert open(outs[i] + ".Ancestry").read() == open(t["text_outs"][i] + ".Ancestry").read()
    # the load's statistics, for the BAM lines alone
    assert "bam" not in res[1] and res[0]["bam"]["records_kept"] == 71 and res[2]["bam"]["records_kept"] == 71


@gpu
def test_a_bad_line_is_its_own_status_and_the_others_run_on(trio_runs, tmp_path, capfd):
    t = trio_runs
    raw = bytearray(open(t["bam"]["b"], "rb").read())
    offs = _blocks(raw)
    raw[offs[len(offs) // 2 + 1] - 8] ^= 0x5A                       # a CRC32 field in the middle
    corrupt = str(tmp_path / "corrupt.bam")
    open(corrupt, "wb").write(bytes(raw))
    open(corrupt + ".bai", "wb").write(open(t["bam"]["b"] + ".bai", "rb").read())
    noindex = str(tmp_path / "noindex.bam")
    open(noindex, "wb").write(open(t["bam"]["b"], "rb").read())
    cram = str(tmp_path / "s.cram")
    open(cram, "wb").write(b"CRAM\x03\x00" + b"\0" * 64)
    for middle, code, word in ((corrupt, _abi.VB2_ERR_INVALID, "CRC32 mismatch"), (noindex, _abi.VB2_ERR_IO, "fail to load index for " + noindex),
                               (cram, _abi.VB2_ERR_INVALID, "is a CRAM file")):
        capfd.readouterr()
        res = vb.run_cohort_files(t["hap"], [t["bam"]["a"], middle, t["bam"]["c"]], None, num_pc=2, disable_sanity=True)
        err = capfd.readouterr().err
        assert [r["status"] for r in res] == [0, code, 0], (middle, [r["status"] for r in res])
        assert word in err and "cohort sample 1" in err, err
        _same_estimate(res[0], t["text_res"][0])
        _same_estimate(res[2], t["text_res"][2])


@gpu
def test_related_and_matched_normal_over_bam_lines_equal_the_text_runs(trio_runs):
    t = trio_runs
    outs = [os.path.join(t["dir"], "stage_" + n) for n in "abc"]
    run = os.path.join(t["dir"], "run")
    kw = dict(num_pc=2, disable_sanity=True, sources_prefix=run)
    got = {}
    for kind, piles in (("text", [t["text"][n] for n in "abc"]), ("bam", [t["bam"][n] for n in "abc"])):
        res, rel = vb.run_cohort_files(t["hap"], piles, outs, find_related=True, **kw)
        related = open(run + ".Related").read()
        res2, fits = vb.run_cohort_files(t["hap"], piles, outs, matched_normal=[(0, 1), (2, 1)], **kw)
        pairfit = open(run + ".PairFit").read()
        got[kind] = (res, rel, related, res2, fits, pairfit)
    a, b = got["text"], got["bam"]
    assert np.array_equal(a[1]["llr"], b[1]["llr"], equal_nan=True) and np.array_equal(a[1]["shared"], b[1]["shared"])
    assert a[2] == b[2]                                              # .Related names the samples by their output prefixes
    for x, y in zip(a[0] + a[3], b[0] + b[3]):
        assert x["status"] == y["status"] == 0
        _same_estimate(x, y)
    for fx, fy in zip(a[4], b[4]):
        assert set(fx) == set(fy)
        for k in fx:
            assert fx[k] == fy[k] or (fx[k] != fx[k] and fy[k] != fy[k]), (k, fx[k], fy[k])
    # .PairFit names the samples as in the list: byte for byte once "<dir>/single_a.Pileup" reads "<dir>/a.bam"
    renamed = a[5]
    for n in "abc":
        renamed = renamed.replace(t["text"][n], t["bam"][n])
    assert renamed == b[5] and a[5] != b[5]


@gpu
def test_command_line_list_with_bam_lines_and_min_bq(trio_runs, tmp_path):
    t = trio_runs
    lst = str(tmp_path / "list.txt")
    outs = [str(tmp_path / ("cli_" + n)) for n in "abc"]
    with open(lst, "w") as fh:
        fh.write("%s\t%s\n%s\t%s\n%s\t%s\n" % (t["bam"]["a"], outs[0], t["text"]["b"], outs[1], t["bam"]["c"], outs[2]))
    p = subprocess.run([EXE, "--DisableSanityCheck", "--SVDPrefix", t["hap"], "--Reference", "unread.fa", "--NumPC", "2", "--PileupList", lst,
                        "--min-BQ", "20", "--Output", str(tmp_path / "run")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    # the pileup options reach the BAM lines: #READS counts the bases of quality 20 and more
    want = sum(1 for _, _, b, q in t["lines"]["a"] for ch in q if ord(ch) - 33 >= 20)
    assert 0 < want < 71
    row = open(outs[0] + ".selfSM").read().splitlines()[1].split("\t")
    assert row[0] == "SampleA" and row[4] == str(want)
    assert open(outs[1] + ".selfSM").read().splitlines()[1].split("\t")[4] == "NA"
    # said once per run, not once per BAM line; and the options are no longer "for --BamFile input only"
    assert p.stderr.count("REF allele") == 1 and p.stderr.count("base alignment quality") == 1
    assert "apply to --BamFile input only" not in p.stderr


@gpu
def test_in_flight_cap_of_bam_lines(trio_runs, tunable):
    t = trio_runs
    piles = [t["bam"]["a"], t["bam"]["c"]] * 3
    peak = _abi.lib().vb2_debug_cohort_bam_peak
    tunable("cohort_bam_inflight", 1)
    res = vb.run_cohort_files(t["hap"], piles, None, num_pc=2, disable_sanity=True, num_host_thread=4)
    assert [r["status"] for r in res] == [0] * 6 and peak() == 1
    tunable("cohort_bam_inflight", 4)
    res = vb.run_cohort_files(t["hap"], piles, None, num_pc=2, disable_sanity=True, num_host_thread=8)
    assert [r["status"] for r in res] == [0] * 6 and 1 <= peak() <= 4
    for r in res[::2]:
        _same_estimate(r, t["text_res"][0])
