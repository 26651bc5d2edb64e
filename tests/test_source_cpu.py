"""--FindSource without a GPU: the C entries exist, the command line refuses what it must before reading any file, and
the numpy restatement of the statistic (tests/source_ref.py) has the properties DESIGN.md section 11 derives."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_ref as sr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
NEW_SYMBOLS = ["vb2_ctx_marginals", "vb2_source_set_create", "vb2_source_set_add", "vb2_source_set_scores",
               "vb2_source_set_size", "vb2_source_set_destroy", "vb2_cohort_run_sources"]


def test_new_entries_exist_and_abi_version_stays():
    from verifybamid_amd import _abi
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _abi.SYMBOLS, name
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert lib.vb2_abi_version() == 7
    assert re.search(r"#define\s+VB2_ABI_VERSION\s+7\b", header)
    # the floor is part of the definition: one constant, the same in the header and the restatement
    assert float(re.search(r"#define\s+VB2_SOURCE_DOT_FLOOR\s+(\S+)", header).group(1)) == sr.DOT_FLOOR
    # no new struct crosses the boundary: the set is an opaque handle
    assert "typedef struct vb2_source_set vb2_source_set;" in header


def test_python_layer_exposes_the_feature():
    import inspect
    import verifybamid_amd as vb
    assert hasattr(vb, "SourceSet") and hasattr(vb.LikelihoodContext, "marginals")
    sig = inspect.signature(vb.run_cohort_files)
    assert sig.parameters["find_source"].default is False and sig.parameters["source_top"].default == 3


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_refuses_find_source_without_pileup_list(tmp_path):
    # (none of the named files exists: the refusal comes before any of them is opened)
    r = _cli(["--SVDPrefix", "nopanel", "--Reference", "noref.fa", "--PileupFile", "no.pileup", "--FindSource",
              "--Output", str(tmp_path / "out")], tmp_path)
    assert r.returncode != 0
    assert b"--FindSource needs --PileupList" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_cli_refuses_find_source_on_several_devices(tmp_path):
    r = _cli(["--SVDPrefix", "nopanel", "--Reference", "noref.fa", "--PileupList", "nolist.txt", "--FindSource",
              "--Devices", "0,1", "--Output", str(tmp_path / "out")], tmp_path)
    assert r.returncode != 0
    assert b"--FindSource cannot be combined with more than one --Devices" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_cli_refuses_a_source_top_below_one(tmp_path):
    r = _cli(["--SVDPrefix", "nopanel", "--Reference", "noref.fa", "--PileupList", "nolist.txt", "--FindSource",
              "--SourceTop", "0", "--Output", str(tmp_path / "out")], tmp_path)
    assert r.returncode != 0
    assert b"--SourceTop takes a positive number" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_kernels_floor_is_the_headers():
    """One constant: the device code takes the float32 rounding of the header's macro, not a literal of its own."""
    src = open(os.path.join(ROOT, "verifybamid_amd", "csrc", "source_kernels.h")).read()
    assert "kSourceDotFloor = (float)VB2_SOURCE_DOT_FLOOR" in src
    assert abs(float(np.float32(sr.DOT_FLOOR)) / sr.DOT_FLOOR - 1) < 1e-8


def test_entry_refuses_several_devices_before_reading():
    import ctypes as C
    from verifybamid_amd import _abi
    lib = _abi.lib()
    devs = (C.c_int32 * 2)(0, 1)
    ca = _abi.CohortArgs()
    ca.base.ud_path, ca.base.mean_path, ca.base.bed_path = b"nopanel.UD", b"nopanel.mu", b"nopanel.bed"
    ca.base.num_pc = 2
    ca.base.devices, ca.base.num_device = devs, 2
    piles = (C.c_char_p * 1)(b"no.pileup")
    ca.num_sample, ca.pileup_paths = 1, piles
    res, st = (_abi.RunResult * 1)(), (C.c_int32 * 1)()
    rc = lib.vb2_cohort_run_sources(C.byref(ca), 3, res, st, None, None)
    assert rc == _abi.VB2_ERR_INVALID
    assert b"one device" in lib.vb2_last_error()


# ---- the restatement's own properties ----

def _one_sample(M=3000, depth=25, alpha=0.04, seed=5, known_af=False, k=2):
    panel = sr.make_panel(M, k, seed=seed)
    G = sr.draw_individuals(panel, 2, seed=seed + 1)
    return sr.make_sample(panel, G[0], G[1], depth, alpha, seed + 2, known_af=known_af)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_marginals_normalise(dtype):
    d = _one_sample()
    rng = np.random.default_rng(0)
    pc1, pc2 = rng.normal(0, 0.01, 2), rng.normal(0, 0.01, 2)
    m = sr.marginals(Counts(d, dtype), pc1, pc2, 0.04)
    live = m["live"]
    assert live.sum() > 2900
    eps = np.finfo(dtype).eps
    assert np.max(np.abs((m["gf1"] * m["c"]).sum(axis=1)[live] - 1)) <= 16 * eps        # sum GF1 c = 1
    assert np.max(np.abs(m["q"].sum(axis=1)[live] - 1)) <= 16 * eps                       # sum q = 1
    assert np.all(m["c"][~live] == 0) and np.all(m["q"][~live] == 0)


def test_clean_sample_has_no_source():
    d = _one_sample(alpha=0.0)
    z = np.zeros(2)
    m = sr.marginals(Counts(d), z, z, 0.0)
    assert np.max(np.abs(m["c"][m["live"]] - 1)) <= 1e-12                                # c == 1 at alpha = 0
    cl, _ = sr.sample_rows(d, z, z, 0.0)
    other = _one_sample(seed=9, alpha=0.0)
    _, q = sr.sample_rows(other, z, z, 0.0)
    s, shared, _ = sr.score(cl, q)
    assert shared > 2900 and abs(s) <= 1e-9                                              # ... and S == 0


def test_mirroring_gives_the_mirrored_samples_scores():
    d = _one_sample(alpha=0.04)
    rng = np.random.default_rng(1)
    pc1, pc2 = rng.normal(0, 0.01, 2), rng.normal(0, 0.01, 2)
    c64 = Counts(d)
    # the identity the mirror rests on: L(pc1, pc2, a) = L(pc2, pc1, 1 - a), marker by marker
    a = sr.marginals(c64, pc1, pc2, 0.96)["log_l"]
    b = sr.marginals(c64, pc2, pc1, 1 - 0.96)["log_l"]
    assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b))
    # an estimate reported with alpha >= 0.5 (indices 0 and 1 of its PCs swapped, as the estimator reports them) ...
    rep1, rep2 = pc1.copy(), pc2.copy()
    rep1[:2], rep2[:2] = pc2[:2], pc1[:2]
    p1, p2, al = sr.search_point(rep1, rep2, 0.96, heter=True)
    assert np.array_equal(p1, pc2) and np.array_equal(p2, pc1) and abs(al - 0.04) < 1e-15
    # ... scores as its mirrored twin does, as target and as candidate
    twin = sr.sample_rows(d, pc2, pc1, al)
    mirrored = sr.sample_rows(d, rep1, rep2, 0.96)
    other = sr.sample_rows(_one_sample(seed=9), np.zeros(2), np.zeros(2), 0.02)
    assert sr.score(mirrored[0], other[1])[:2] == sr.score(twin[0], other[1])[:2]
    assert sr.score(other[0], mirrored[1])[:2] == sr.score(other[0], twin[1])[:2]
    # without the two-ancestry model there is no swap to undo
    p1, p2, al = sr.search_point(pc1, pc1, 0.7, heter=False)
    assert np.array_equal(p1, pc1) and np.array_equal(p2, pc1) and abs(al - 0.3) < 1e-15


def test_floor_bounds_one_markers_veto():
    c = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    q = np.array([[0.0, 0.0, 1.0], [0.2, 0.3, 0.5]])
    s, shared, bound = sr.score(c, q)
    assert shared == 2 and abs(s - np.log(1e-30)) <= 1e-12 and s > -70


# (markers, depth, alpha of target 0, contaminated by individual 1): the table of the feature's proposal, with the true
# allele frequencies as priors and alpha fixed at 1e-3 for the clean targets.  Measured with these seeds: true source
# +2449.9 / +127.2 / +80.1 nats, the six other individuals -5779 .. -5600 / -180 .. -130 / -210 .. -159, clean targets
# -18.6 .. +2.5 / -4.1 .. +2.0 / -7.9 .. +2.2; rounding the triples to float32 moves the first score by 2.7e-5.
@pytest.mark.parametrize("M,depth,alpha,true_lo,others_hi", [(20000, 30, 0.05, 2000.0, -5000.0),
                                                              (10000, 10, 0.02, 100.0, -100.0),
                                                              (5000, 30, 0.01, 60.0, -100.0)])
def test_true_source_separates(M, depth, alpha, true_lo, others_hi):
    panel = sr.make_panel(M, 2, seed=11)
    G = sr.draw_individuals(panel, 9, seed=12)               # 8 cohort members and one outsider
    z = np.zeros(2)
    rows = []
    for i in range(8):
        d = sr.make_sample(panel, G[i], G[1 if i == 0 else 8], depth, alpha if i == 0 else 0.0, 100 + i, known_af=True)
        rows.append(sr.sample_rows(d, z, z, alpha if i == 0 else 1e-3))
    S, shared, _ = sr.score_matrix(rows)
    print("true source %+.1f, others %+.1f .. %+.1f, clean targets %+.1f .. %+.1f" %
          (S[0, 1], np.nanmin(S[0, 2:]), np.nanmax(S[0, 2:]), np.nanmin(S[1:]), np.nanmax(S[1:])))
    assert np.all(np.isnan(np.diag(S)))
    assert S[0, 1] > true_lo
    assert np.nanmax(S[0, 2:]) < others_hi
    assert np.nanmax(np.abs(S[1:])) < 25.0 < S[0, 1]
    # float32 triples: nine orders of magnitude below the separation
    r32 = [(c.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64)) for c, q in rows]
    assert abs(sr.score(r32[0][0], r32[1][1])[0] - S[0, 1]) < 1e-3
