"""--RefVCF on the device: the exact int8-MFMA Gram, the panel against a numpy restatement of ProcessRefVCF (float32
mu, FP64 centred Gram, eigh), --NumSVDPCs, and an end-to-end estimate against a GPU-built panel."""
import os
import subprocess

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if _abi.lib().vb2_device_count() < 1:
        pytest.fail("no gfx950 device visible: the panel builder runs on the GPU only")


def _gram_ref(G):
    # float64 BLAS is exact here: |entries| <= 4 * M < 2^53
    Gf = G.astype(np.float64)
    return np.rint(Gf.T @ Gf).astype(np.int64)


def _random_geno(M, N, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(M, N), p=[0.05, 0.45, 0.3, 0.2])


@pytest.mark.parametrize("M", [1, 4999])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1001, 2504])
def test_gram_is_exact(M, N):
    G = _random_geno(M, N, seed=M * 7919 + N)
    r = vb.build_panel_from_genotypes(G, num_svd_pcs=1)
    assert np.array_equal(r["gram"].astype(np.int64), _gram_ref(G))
    assert np.array_equal(r["row_sum"], G.astype(np.int64).sum(axis=1))


@pytest.mark.parametrize("N", [65, 1001, 2504])
def test_gram_is_exact_over_many_chunks(N):
    M = 70001
    G = _random_geno(M, N, seed=N)
    want = _gram_ref(G)
    one = vb.build_panel_from_genotypes(G, num_svd_pcs=2, chunk_markers=1 << 17)     # a single chunk
    many = vb.build_panel_from_genotypes(G, num_svd_pcs=2, chunk_markers=4096)       # 18 chunks
    assert np.array_equal(one["gram"].astype(np.int64), want)
    assert np.array_equal(many["gram"].astype(np.int64), want)


def test_gram_special_matrices():
    M, N = 3000, 130
    G = _random_geno(M, N, seed=11)
    G[:500, :] = 2                 # an all-2 block: the largest entries
    G[500:700, :] = 0              # all-zero rows
    G[700:900, :] = -1             # all-missing rows (-1 stays in the matrix, as in the reference)
    G[:, 5] = -1
    for cm in (128, 0):
        r = vb.build_panel_from_genotypes(G, num_svd_pcs=3, chunk_markers=cm)
        assert np.array_equal(r["gram"].astype(np.int64), _gram_ref(G))
    # the -1 entries are in the mean too: mu = (float)sum / (float)N
    assert np.array_equal(r["mu"], (G.astype(np.float32).sum(axis=1, dtype=np.float32) / np.float32(N)).astype(np.float64))


def _restate(G, k):
    """ProcessRefVCF + ComputeSvdGram in numpy: float32 mu, FP64 centred Gram, eigh, our sign convention."""
    M, N = G.shape
    mu = (G.sum(axis=1).astype(np.float32) / np.float32(N)).astype(np.float64)
    Gf = G.astype(np.float64)
    S = Gf.T @ Gf
    c = Gf.T @ mu
    tau = mu @ mu
    C = ((S - c[:, None]) - c[None, :]) + tau
    w, U = np.linalg.eigh(C)
    sigma = np.sqrt(np.maximum(w[::-1], 0.0))
    V = U[:, ::-1][:, :k].copy()
    for q in range(k):
        j = int(np.argmax(np.abs(V[:, q])))
        if V[j, q] < 0:
            V[:, q] = -V[:, q]
    UD = (Gf - mu[:, None]) @ V
    return mu, sigma, V, UD


def _write_panel(prefix, d, mu, UD, V):
    """WriteSVD's format (ostream defaults: 6 significant digits, a tab after every .UD/.V value)."""
    with open(prefix + ".mu", "w") as f:
        for c, p, m in zip(d["chr"], d["pos"], mu):
            f.write("%s:%d\t%s\n" % (c, p, "%g" % m))
    with open(prefix + ".bed", "w") as f:
        for c, p, r, a in zip(d["chr"], d["pos"], d["ref"], d["alt"]):
            f.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(prefix + ".UD", "w") as f:
        for row in UD:
            f.write("".join("%g\t" % x for x in row) + "\n")
    with open(prefix + ".V", "w") as f:
        for s, row in zip(d["samples"], V):
            f.write(s + "\t" + "".join("%g\t" % x for x in row) + "\n")


@pytest.fixture(scope="module")
def structured(tmp_path_factory):
    t = tmp_path_factory.mktemp("panel")
    path = str(t / "ref.vcf.gz")
    info = vb.synth.write_structured_vcf(path, 6000, 1200, num_pop=3, fst=0.1, missing=0.02, seed=21, skipped_every=97)
    return t, path, info


def test_panel_against_the_restatement(structured):
    t, path, info = structured
    d = vb.read_vcf(path)
    G = d["genotypes"]
    assert G.shape == (6000, 1200) and (G < 0).any()
    k = 10
    pre_a, pre_b = str(t / "a"), str(t / "b")
    r = vb.build_panel(path, output_prefix=pre_a, num_svd_pcs=k, chunk_markers=1024)
    r2 = vb.build_panel(path, output_prefix=pre_b, num_svd_pcs=k, num_thread=7)
    mu, sigma, V, UD = _restate(G, k)
    assert np.array_equal(r["mu"], mu)
    # the full spectrum as eigenvalues (sigma of the null direction that centring leaves is the root of rounding noise),
    # the top k as singular values
    assert np.max(np.abs(r["sigma"] ** 2 - sigma ** 2)) <= 1e-10 * sigma[0] ** 2
    assert np.allclose(r["sigma"][:k], sigma[:k], rtol=1e-10, atol=0)
    for q in range(k):
        s = 1.0 if V[:, q] @ r["v"][:, q] >= 0 else -1.0
        assert np.max(np.abs(r["v"][:, q] - s * V[:, q])) <= 1e-8 * np.linalg.norm(V[:, q]), q
        assert np.max(np.abs(r["ud"][:, q] - s * UD[:, q])) <= 1e-8 * np.linalg.norm(UD[:, q]), q
        j = int(np.argmax(np.abs(r["v"][:, q])))
        assert r["v"][j, q] > 0                           # the sign convention
    # .bed and .mu byte for byte against the reference's format; two builds give the same bytes
    _write_panel(str(t / "re"), d, mu, UD, V)
    for ext in (".bed", ".mu"):
        assert open(pre_a + ext, "rb").read() == open(str(t / "re") + ext, "rb").read(), ext
    for ext in (".bed", ".mu", ".UD", ".V"):
        assert open(pre_a + ext, "rb").read() == open(pre_b + ext, "rb").read(), ext
    ud_lines = open(pre_a + ".UD").read().splitlines()
    assert len(ud_lines) == 6000 and ud_lines[0].count("\t") == k and ud_lines[0].endswith("\t")
    # .UD and .V line by line against the struct's numbers (a transposed or shifted column would pass the two-builds
    # comparison above both ways)
    for m, (line, row) in enumerate(zip(ud_lines, r["ud"])):
        assert line == "".join("%g\t" % x for x in row), (".UD", m)
    v_lines = open(pre_a + ".V").read().splitlines()
    assert len(v_lines) == 1200 == len(d["samples"])
    for j, (line, name, row) in enumerate(zip(v_lines, d["samples"], r["v"])):
        assert line == name + "\t" + "".join("%g\t" % x for x in row), (".V", j)
    # the populations separate on the first two PCs
    pop = info["pop"]
    cent = np.array([r["v"][pop == p, :2].mean(axis=0) for p in range(3)])
    assert np.min([np.linalg.norm(cent[a] - cent[b]) for a in range(3) for b in range(a + 1, 3)]) > 0.01


def test_num_svd_pcs():
    G = _random_geno(300, 80, seed=3)
    assert vb.build_panel_from_genotypes(G, num_svd_pcs=0)["ud"].shape == (300, 80)
    assert vb.build_panel_from_genotypes(G, num_svd_pcs=500)["v"].shape == (80, 80)
    r1 = vb.build_panel_from_genotypes(G, num_svd_pcs=1)
    assert r1["ud"].shape == (300, 1) and r1["v"].shape == (80, 1)
    Gs = _random_geno(50, 80, seed=4)                  # fewer markers than samples: min(M, N)
    assert vb.build_panel_from_genotypes(Gs, num_svd_pcs=0)["v"].shape == (80, 50)
    assert vb.build_panel_from_genotypes(Gs, num_svd_pcs=0)["sigma"].shape == (80,)


def test_genotype_entry_minimums():
    G = _random_geno(300, 80, seed=5)
    with pytest.raises(_abi.Vb2Error, match="Insufficient number of markers"):
        vb.build_panel_from_genotypes(G, check_minimums=True)


def test_end_to_end_contamination_on_the_built_panel(structured):
    t, path, info = structured
    d = vb.read_vcf(path)
    G = d["genotypes"]
    k = 4
    pre = str(t / "e2e")
    r = vb.build_panel(path, output_prefix=pre, num_svd_pcs=k)
    mu, sigma, V, UD = _restate(G, k)
    _write_panel(str(t / "e2e_re"), d, mu, UD, V)
    # held-out individuals: intended from population 0, contaminant from population 1, alpha 0.05
    rng = np.random.default_rng(77)
    assert np.array_equal(info["pos"], d["pos"])        # the rows the reader skips are extra rows of the writer
    g_int = rng.binomial(2, info["freqs"][0])
    g_con = rng.binomial(2, info["freqs"][1])
    ref_c = np.array([ord(x) for x in d["ref"]], dtype=np.uint8)
    alt_c = np.array([ord(x) for x in d["alt"]], dtype=np.uint8)
    off, bases, quals = vb.synth.reads_from_genotypes(g_int, g_con, ref_c, alt_c, mean_depth=30, alpha_true=0.05, seed=8)
    pile = str(t / "s.pileup")
    vb.synth.write_pileup_text(pile, d["chr"], d["pos"], ref_c, off, bases, quals)
    a = vb.run_files(pre, pile, num_pc=2, disable_sanity=True, device=0)
    b = vb.run_files(str(t / "e2e_re"), pile, num_pc=2, disable_sanity=True, device=0)
    assert abs(a["alpha"] - b["alpha"]) <= 1e-4, (a["alpha"], b["alpha"])
    assert abs(a["alpha"] - 0.05) <= 0.02, a["alpha"]
    assert r["ud"].shape == (6000, k)

    # the command line: build at <vcf>, then estimate with --SVDPrefix <vcf>
    vcf = str(t / "cli.vcf.gz")
    os.symlink(path, vcf)
    r1 = subprocess.run([EXE, "--RefVCF", vcf, "--NumSVDPCs", "4", "--NumThread", "8"], capture_output=True, text=True,
                        timeout=600)
    assert r1.returncode == 0, r1.stderr
    assert "variance_explained" in r1.stderr and "unknown option" not in r1.stderr
    for ext in (".UD", ".mu", ".bed", ".V"):
        assert os.path.exists(vcf + ext)
    assert open(vcf + ".bed", "rb").read() == open(pre + ".bed", "rb").read()
    out = str(t / "cli_out")
    r2 = subprocess.run([EXE, "--SVDPrefix", vcf, "--PileupFile", pile, "--Reference", str(t / "unused.fa"),
                         "--DisableSanityCheck", "--Output", out], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr
    assert os.path.exists(out + ".selfSM")
