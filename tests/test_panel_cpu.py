"""--RefVCF without a device: the VCF reader (SVDcalculator::ReadVcf, SVDcalculator.cpp:22-228, restated rule by rule
below), the command line's checks that come before any device call, the layouts of the new ABI structs, and the
a-posteriori checker of the decomposition (tests/panel_ref.py) on a float64 numpy restatement with and without planted
faults."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_ref as pr  # noqa: E402

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


# ---- the a-posteriori checker (tests/panel_ref.py): inside every bound on the float64 restatement alone, and each planted
# ---- fault caught by the quantity that points at its stage

PANEL_SHAPES = [(300, 80, 33), (257, 129, 17)]


@pytest.fixture(scope="module", params=PANEL_SHAPES, ids=lambda p: "%dx%d_k%d" % p)
def restated(request):
    M, N, k = request.param
    G = pr.structured_geno(M, N, seed=M + N)
    mu, S, c, tau = pr.restate_gram(G)
    sigma, V, raw = pr.restate_eig(pr.centre(S, c, tau), k)
    r = pr.restate(G, k)
    assert np.array_equal(r["v"], V) and np.array_equal(r["sigma"], sigma)
    return dict(G=G, k=k, r=r, mu=mu, S=S, c=c, tau=tau, sigma=sigma, V=V, raw=raw)


def test_checker_is_longdouble():
    G = pr.structured_geno(40, 9, seed=1)
    mu, C, S = pr.exact_centred_gram(G)
    assert C.dtype == np.longdouble and S.dtype == np.int64 and mu.dtype == np.float64
    assert np.array_equal(mu, mu.astype(np.float32).astype(np.float64))            # binary32 values
    assert np.array_equal(mu.astype(np.float32), G.sum(axis=1).astype(np.float32) / np.float32(9))
    # C against exact rationals (mu is a dyadic rational): within the 80-bit rounding of sums of M terms of <= 4 M in all,
    # M 4M 2^-64, which is below half a binary64 ulp of the entries here
    from fractions import Fraction
    muq = [Fraction(float(m)) for m in mu]
    Gi = G.astype(np.int64)

    def exact(x):                                   # a longdouble as a Fraction: two binary64 pieces
        hi = float(x)
        return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))
    for i, j in ((0, 0), (3, 7), (8, 2)):
        want = sum(int(Gi[m, i] * Gi[m, j]) - muq[m] * int(Gi[m, i]) - muq[m] * int(Gi[m, j]) + muq[m] * muq[m]
                   for m in range(40))
        assert abs(exact(C[i, j]) - want) <= Fraction(40 * 160, 2 ** 64), (i, j)
        assert Fraction(40 * 160, 2 ** 64) < Fraction(float(np.spacing(np.float64(abs(C[i, j]))))) / 2
    ref, cond = pr.projection_reference(G, mu, np.eye(9)[:, :2])
    assert ref.dtype == np.longdouble and cond.dtype == np.longdouble


def test_checker_passes_the_restatement(restated):
    rec = pr.check_panel(restated["G"], restated["r"], restated["k"])
    print(pr.ratios_line(rec))
    pr.assert_inside(rec)
    assert all(rec[n] <= 1.0 for n in pr.RATIOS)
    # by construction: the restatement is its own yardstick
    for n in ("resid", "ortho", "trace", "spec"):
        assert rec["value"][n] == rec["ref"][n] and rec[n] <= 1.0 / pr.MARGIN + 1e-12, n


def _with(restated, **kw):
    r = dict(restated["r"])
    r.update(kw)
    return r


def _caught_by(restated, r, quantity):
    """The quantity named raises, or its ratio is above 1; the exact checks come first, so a raise names the first."""
    try:
        rec = pr.check_panel(restated["G"], r, restated["k"])
    except pr.PanelMismatch as e:
        assert e.quantity == quantity, str(e)
        return None
    assert quantity in pr.RATIOS and rec[quantity] > 1.0, (quantity, pr.ratios_line(rec))
    with pytest.raises(pr.PanelMismatch):
        pr.assert_inside(rec)
    return rec


def test_fault_last_sample_left_out_of_the_projection(restated):
    G, V, mu = restated["G"], restated["V"], restated["mu"]
    ud = pr.project_in_kernel_order(G, mu, V, samples=G.shape[1] - 1)
    _caught_by(restated, _with(restated, ud=ud), "proj")


def test_fault_col0_offset_lost(restated):
    G, V, mu, k = restated["G"], restated["V"], restated["mu"], restated["k"]
    vsum = pr.column_sums(V)
    ud = restated["r"]["ud"].copy()
    for col0 in range(16, k, 16):
        kc = min(16, k - col0)
        ud[:, col0:col0 + kc] = pr.project_in_kernel_order(G, mu, V[:, :kc], vsum=vsum[col0:col0 + kc])
    rec = _caught_by(restated, _with(restated, ud=ud), "proj")
    assert rec["where"]["proj"][1] >= 16          # the first pass is right


def test_fault_vsum_before_the_sign_flip(restated):
    G, V, mu, raw = restated["G"], restated["V"], restated["mu"], restated["raw"]
    assert (np.sign(raw[0]) != np.sign(V[0])).any()             # some column was flipped
    ud = pr.project_in_kernel_order(G, mu, V, vsum=pr.column_sums(raw))
    _caught_by(restated, _with(restated, ud=ud), "proj")


def test_fault_float32_accumulation(restated):
    ud = pr.project_in_kernel_order(restated["G"], restated["mu"], restated["V"], dtype=np.float32)
    _caught_by(restated, _with(restated, ud=ud), "proj")


def test_fault_float64_mean(restated):
    G, k = restated["G"], restated["k"]
    mu = G.astype(np.int64).sum(axis=1) / np.float64(G.shape[1])
    _, S, c, tau = pr.restate_gram(G, mu=mu)
    sigma, V, _ = pr.restate_eig(pr.centre(S, c, tau), k)
    r = _with(restated, mu=mu, sigma=sigma, v=V, ud=pr.project_in_kernel_order(G, mu, V))
    _caught_by(restated, r, "mu")


def test_fault_one_column_sign_reversed(restated):
    V = restated["V"].copy()
    V[:, 3] = -V[:, 3]
    _caught_by(restated, _with(restated, v=V), "sign")


def test_fault_ascending_eigenpairs(restated):
    G, mu, k = restated["G"], restated["mu"], restated["k"]
    w, Uu = np.linalg.eigh(pr.centre(restated["S"], restated["c"], restated["tau"]))
    sigma = np.sqrt(np.maximum(w, 0.0))
    V = Uu[:, :k].copy()
    for q in range(k):
        if V[int(np.argmax(np.abs(V[:, q]))), q] < 0:
            V[:, q] = -V[:, q]
    _caught_by(restated, _with(restated, sigma=sigma, v=V, ud=pr.project_in_kernel_order(G, mu, V)), "sigma")
    # ... and with a sigma that looks right, the columns are still not those of the k largest eigenvalues
    _caught_by(restated, _with(restated, v=V, ud=pr.project_in_kernel_order(G, mu, V)), "order")


def test_fault_unmirrored_upper_tile(restated):
    G, mu, k = restated["G"], restated["mu"], restated["k"]
    S = restated["S"].copy()
    S[0:64, 64:128] = 0.0                    # the device writes lower tiles only: an upper tile read as it is ...
    sigma, V, _ = pr.restate_eig(pr.centre(S, restated["c"], restated["tau"]), k, uplo="U")    # ... by a solver that reads it
    r = _with(restated, sigma=sigma, v=V, ud=pr.project_in_kernel_order(G, mu, V))
    _caught_by(restated, r, "resid")


def test_fault_neighbours_eigenvector(restated):
    G, mu = restated["G"], restated["mu"]
    V = restated["V"].copy()
    V[:, 4] = V[:, 5]
    rec = _caught_by(restated, _with(restated, v=V, ud=pr.project_in_kernel_order(G, mu, V)), "resid")
    assert rec["where"]["resid"] == (4,) and rec["proj"] <= 1.0        # the projection of that V is still right
