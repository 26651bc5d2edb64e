"""--RefVCF without a device: the VCF reader (SVDcalculator::ReadVcf, SVDcalculator.cpp:22-228, restated rule by rule
below), the command line's checks that come before any device call, and the layouts of the new ABI structs."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
HEADER = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def _vcf(tmp_path, rows, samples=("A", "B", "C"), name="t.vcf"):
    p = tmp_path / name
    text = HEADER + "\t" + "\t".join(samples) + "\n" + "".join("\t".join(r) + "\n" for r in rows)
    if name.endswith(".gz"):
        with gzip.open(p, "wt") as f:
            f.write(text)
    else:
        p.write_text(text)
    return str(p)


def _row(chrom, pos, fmt, *vals, ref="A", alt="C", flt="PASS"):
    return [chrom, str(pos), ".", ref, alt, ".", flt, ".", fmt] + list(vals)


def test_reference_testreadvcf_restated(golden_dir):
    """TestReadVcf.cpp: every PASS row is kept with the missing count and the AF over non-missing samples that its
    INFO column states."""
    path = os.path.join(golden_dir, "panel", "test_readvcf.vcf")
    d = vb.read_vcf(path, include_chr=[])
    expected = []
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        cols = line.rstrip("\n").split("\t")
        if cols[6] != "PASS":
            continue
        info = dict(kv.split("=", 1) for kv in cols[7].split(";") if "=" in kv)
        expected.append((info.get("TESTDESC"), float(info["EXPECTED_AF"]), int(info["EXPECTED_N_MISSING"])))
    g = d["genotypes"]
    assert g.shape[0] == len(expected)
    for m, (desc, af, nmiss) in enumerate(expected):
        row = g[m]
        ok = row >= 0
        assert int((~ok).sum()) == nmiss, desc
        got = row[ok].sum() / (2.0 * ok.sum()) if ok.any() else 0.0
        assert abs(got - af) <= 1e-3, (desc, got, af)


def test_filter_must_be_exactly_pass(tmp_path):
    p = _vcf(tmp_path, [_row("1", 10, "GT", "0/0", "0/1", "1/1", flt="."),
                        _row("1", 20, "GT", "0/0", "0/1", "1/1", flt="q10"),
                        _row("1", 30, "GT", "0/0", "0/1", "1/1", flt="PASS;q10"),
                        _row("1", 40, "GT", "0/0", "0/1", "1/1")])
    d = vb.read_vcf(p, include_chr=[])
    assert list(d["pos"]) == [40]


def test_multiallelic_and_indels_skipped(tmp_path):
    p = _vcf(tmp_path, [_row("1", 10, "GT", "0/0", "0/1", "1/1", alt="C,G"),
                        _row("1", 20, "GT", "0/0", "0/1", "1/1", ref="AT"),
                        _row("1", 30, "GT", "0/0", "0/1", "1/1", alt="CT"),
                        _row("1", 40, "GT", "0/0", "0/1", "1/1", ref="g", alt="t")])
    d = vb.read_vcf(p, include_chr=[])
    assert list(d["pos"]) == [40]
    assert d["ref"] == ["G"] and d["alt"] == ["T"]      # libVcf upper-cases the alleles


def test_default_include_set_is_the_autosomes(tmp_path):
    rows = [_row(c, 10 * (i + 1), "GT", "0/0", "0/1", "1/1") for i, c in enumerate(["5", "chr5", "X", "chrX", "MT", "22"])]
    p = _vcf(tmp_path, rows)
    d = vb.read_vcf(p)
    assert d["chr"] == ["5", "chr5", "22"]
    assert vb.read_vcf(p, include_chr=["X", "MT"])["chr"] == ["X", "MT"]
    assert len(vb.read_vcf(p, include_chr=[])["chr"]) == 6


def test_duplicate_marker_is_fatal(tmp_path):
    p = _vcf(tmp_path, [_row("1", 10, "GT", "0/0", "0/1", "1/1"), _row("1", 10, "GT", "0/0", "0/1", "1/1", flt="q10")])
    with pytest.raises(_abi.Vb2Error, match="Duplicated Marker: 1:10"):
        vb.read_vcf(p, include_chr=[])
    # only the previous KEPT marker counts: a filtered row in between hides nothing, a skipped first copy is no duplicate
    p2 = _vcf(tmp_path, [_row("1", 10, "GT", "0/0", "0/1", "1/1", flt="q10"), _row("1", 10, "GT", "0/0", "0/1", "1/1")],
              name="u.vcf")
    assert list(vb.read_vcf(p2, include_chr=[])["pos"]) == [10]


def test_pl_then_gl_then_gt_per_sample(tmp_path):
    # sample A: PL says 2, GL says 1, GT says 0 -> 2; B: PL missing -> GL (1); C: PL and GL missing -> GT (0)
    p = _vcf(tmp_path, [_row("1", 10, "GT:GL:PL", "0/0:-5,0,-5:50,30,0", "0/0:-5,0,-5:.", "0/0:.:.")])
    assert vb.read_vcf(p, include_chr=[])["genotypes"].tolist() == [[2, 1, 0]]
    # GL is converted with static_cast<int>(-10 x): -0.09 -> 0 ties with 0 -> the first (strict <) wins
    p = _vcf(tmp_path, [_row("1", 10, "GL", "-0.09,0,-1", "-1,-0.05,0", "-3,-0.2,-3")], name="gl.vcf")
    assert vb.read_vcf(p, include_chr=[])["genotypes"].tolist() == [[0, 1, 1]]
    # GT: 1/0 and 0|1 are heterozygous; 1/2 sums to 3: homozygous alt
    p = _vcf(tmp_path, [_row("1", 10, "GT", "1/0", "0|1", "1/2")], name="gt.vcf")
    assert vb.read_vcf(p, include_chr=[])["genotypes"].tolist() == [[1, 1, 2]]


def test_positive_gl_or_negative_pl_is_fatal(tmp_path):
    p = _vcf(tmp_path, [_row("1", 10, "GL", "0.5,0,-1", "0,-1,-2", "0,-1,-2")])
    with pytest.raises(_abi.Vb2Error, match="Negative PL or Positive GL observed"):
        vb.read_vcf(p, include_chr=[])
    p = _vcf(tmp_path, [_row("1", 10, "PL", "0,-3,50", "0,30,50", "0,30,50")], name="pl.vcf")
    with pytest.raises(_abi.Vb2Error, match="Negative PL"):
        vb.read_vcf(p, include_chr=[])


def test_phreds_at_or_above_255_give_minus_one_not_missing(tmp_path):
    # 5 samples: one all-high (-1, not missing), one missing: 1/5 = 0.2 -> kept (the all-high one does not count)
    p = _vcf(tmp_path, [_row("1", 10, "PL", "255,300,999", ".", "0,30,50", "0,30,50", "0,30,50")],
             samples=("A", "B", "C", "D", "E"))
    d = vb.read_vcf(p, include_chr=[])
    assert d["genotypes"].tolist() == [[-1, -1, 0, 0, 0]]
    # 254 < 255: a genotype
    p = _vcf(tmp_path, [_row("1", 10, "PL", "255,254,999", "0,30,50", "0,30,50")], name="b.vcf")
    assert vb.read_vcf(p, include_chr=[])["genotypes"].tolist() == [[1, 0, 0]]


def test_missing_rate_threshold(tmp_path):
    samples = tuple("S%d" % i for i in range(10))
    two = ["./.", "."] + ["0/1"] * 8            # 0.2: kept
    three = ["./.", ".", "./."] + ["0/1"] * 7   # 0.3: skipped
    p = _vcf(tmp_path, [_row("1", 10, "GT", *two), _row("1", 20, "GT", *three)], samples=samples)
    d = vb.read_vcf(p, include_chr=[])
    assert list(d["pos"]) == [10]
    assert d["genotypes"][0].tolist() == [-1, -1] + [1] * 8
    # 1 of 5 (0.2f) kept; 2 of 9 (0.222) skipped
    p = _vcf(tmp_path, [_row("1", 10, "GT", ".", "0/0", "0/0", "0/0", "0/0")], samples=samples[:5], name="f.vcf")
    assert vb.read_vcf(p, include_chr=[])["genotypes"].shape == (1, 5)
    p = _vcf(tmp_path, [_row("1", 10, "GT", ".", ".", *["0/0"] * 7)], samples=samples[:9], name="n.vcf")
    assert vb.read_vcf(p, include_chr=[])["genotypes"].shape == (0, 9)


def test_field_count_mismatch_is_fatal(tmp_path):
    p = _vcf(tmp_path, [_row("1", 10, "GT:PL", "0/0:0,30,50", "0/1", "1/1:50,30,0")])
    with pytest.raises(_abi.Vb2Error, match="do not match with # fields in FORMAT"):
        vb.read_vcf(p, include_chr=[])
    # ... even on a row that is filtered: libVcf parses the values before ReadVcf looks at FILTER
    p = _vcf(tmp_path, [_row("1", 10, "GT:PL", "0/0:0,30,50", "0/1", "1/1:50,30,0", flt="q10")], name="q.vcf")
    with pytest.raises(_abi.Vb2Error, match="do not match"):
        vb.read_vcf(p, include_chr=[])


def test_gz_reads_like_plain_text(tmp_path):
    info = vb.synth.write_structured_vcf(str(tmp_path / "s.vcf.gz"), 700, 40, seed=5, skipped_every=60)
    vb.synth.write_structured_vcf(str(tmp_path / "s.vcf"), 700, 40, seed=5, skipped_every=60)
    a = vb.read_vcf(str(tmp_path / "s.vcf.gz"), num_thread=3)
    b = vb.read_vcf(str(tmp_path / "s.vcf"), num_thread=1)
    assert np.array_equal(a["genotypes"], b["genotypes"])
    assert a["chr"] == b["chr"] and np.array_equal(a["pos"], b["pos"]) and a["samples"] == b["samples"]
    assert np.array_equal(a["genotypes"], info["genotypes"])
    assert np.array_equal(a["pos"], info["pos"])


def test_parser_threads_keep_marker_order(tmp_path):
    """Blocks of 4 MB are parsed in parallel; a panel of several blocks comes out in file order whatever the pool."""
    p = str(tmp_path / "big.vcf")
    info = vb.synth.write_structured_vcf(p, 5000, 700, formats="GT", seed=9)
    assert os.path.getsize(p) > 3 * (4 << 20)
    ref = vb.read_vcf(p, num_thread=1)
    for t in (2, 7):
        d = vb.read_vcf(p, num_thread=t)
        assert np.array_equal(d["genotypes"], ref["genotypes"]) and np.array_equal(d["pos"], ref["pos"])
    assert np.array_equal(ref["genotypes"], info["genotypes"])


def _cli(args, timeout=300):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=timeout)


def test_cli_refvcf_too_few_markers(tmp_path):
    p = str(tmp_path / "few.vcf")
    vb.synth.write_structured_vcf(p, 300, 20, formats="GT", seed=2)
    r = _cli(["--RefVCF", p, "--NumSVDPCs", "4", "--IncludeChr", "1,2,3", "--GramSVD", "--SkipMinSampleCountCheck",
              "--NumThread", "2"])
    assert r.returncode != 0
    assert "Insufficient number of markers (need >= 5000, have 300)" in r.stderr, r.stderr
    assert "unknown option" not in r.stderr
    assert "--UDPath is required" not in r.stderr and "--Reference is required" not in r.stderr
    assert not os.path.exists(p + ".UD")


def test_cli_refvcf_too_few_individuals(tmp_path):
    p = str(tmp_path / "ind.vcf.gz")
    vb.synth.write_structured_vcf(p, 5000, 999, formats="GT", missing=0.0, seed=4)
    r = _cli(["--RefVCF", p])
    assert r.returncode != 0
    assert "Insufficient number of individuals (need >= 1000, have 999)" in r.stderr, r.stderr
    assert "--SkipMinSampleCountCheck" in r.stderr
    assert "Number of Markers after filtering: 5000" in r.stderr


def test_cli_refvcf_without_a_device_fails_loudly(tmp_path):
    if _abi.lib().vb2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    p = str(tmp_path / "ok.vcf")
    vb.synth.write_structured_vcf(p, 5000, 30, formats="GT", seed=6)
    r = _cli(["--RefVCF", p, "--SkipMinSampleCountCheck"])
    assert r.returncode != 0 and "no gfx950 device" in r.stderr, r.stderr


def test_panel_abi_structs_match_the_binding(tmp_path):
    src = tmp_path / "panel_abi.c"
    names = {"vb2_panel_args": _abi.PanelArgs, "vb2_vcf_view": _abi.VcfView, "vb2_panel_view": _abi.PanelView}
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vb2_abi.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   "".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f)
                           for n, cls in names.items() for f, _ in cls._fields_) +
                   "  return 0;\n}\n")
    exe = tmp_path / "panel_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for n, cls in names.items():
        assert int(got[n]) == C.sizeof(cls), n
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (n, f)]) == getattr(cls, f).offset, (n, f)
