"""--FindRelated without a GPU: the C entries exist, the command line and the entry refuse what they must before reading
any file, the new kernels' code-object notes are what DESIGN.md section 15 records, and the numpy restatement of the
statistic (tests/related_ref.py) has the properties section 15 derives."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import related_ref as rr  # noqa: E402
import source_ref as sr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
LIB = os.path.join(ROOT, "verifybamid_amd", "libvb2.so")
NEW_SYMBOLS = ["vb2_source_set_create_ex", "vb2_source_set_relations", "vb2_ctx_marginals_related", "vb2_cohort_run_related"]
# DESIGN.md section 15, "Resources": VGPRs of the new kernels, from the code-object notes
VGPRS = {"related_pair_kernel": 52, "related_reduce_kernel": 26, "source_marginal_kernel<true, true>": 94,
         "source_marginal_kernel<false, true>": 121}


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
    for name, value in (("VB2_SET_SOURCE", 1), ("VB2_SET_RELATED", 2), ("VB2_NUM_RELATION", 4), ("VB2_REL_DUP", 0),
                        ("VB2_REL_PO", 1), ("VB2_REL_FS", 2), ("VB2_REL_D2", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(_abi, name) == value
    assert float(re.search(r"#define\s+VB2_SOURCE_DOT_FLOOR\s+(\S+)", header).group(1)) == rr.DOT_FLOOR


def test_the_kernels_floor_is_the_headers():
    """One constant: the pair kernel floors its mixtures at section 11's float32 rounding of the header's macro."""
    src = open(os.path.join(ROOT, "verifybamid_amd", "csrc", "related_kernels.h")).read()
    assert "kRelatedFloor = kSourceDotFloor" in src
    assert "kSourceDotFloor = (float)VB2_SOURCE_DOT_FLOOR" in open(os.path.join(ROOT, "verifybamid_amd", "csrc", "source_kernels.h")).read()
    # the twelve coefficients are exact in float32
    assert np.array_equal(rr.COEF.astype(np.float32).astype(np.float64), rr.COEF)


def test_python_layer_exposes_the_feature():
    import inspect
    import verifybamid_amd as vb
    assert hasattr(vb.SourceSet, "relations")
    assert inspect.signature(vb.SourceSet.__init__).parameters["planes"].default == vb.SourceSet.SOURCE == 1
    assert vb.SourceSet.RELATED == 2 and vb.SourceSet.RELATIONS == rr.RELATIONS
    assert inspect.signature(vb.LikelihoodContext.marginals).parameters["related"].default is False
    sig = inspect.signature(vb.run_cohort_files)
    assert sig.parameters["find_related"].default is False and sig.parameters["related_top"].default == 3


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


# (none of the named files exists: the refusal comes before any of them is opened)
@pytest.mark.parametrize("extra,message", [
    (["--PileupFile", "no.pileup"], b"--FindRelated needs --PileupList"),
    (["--PileupList", "nolist.txt", "--FindSource", "--RefitSource"], b"--FindRelated cannot be combined with --RefitSource"),
    (["--PileupList", "nolist.txt", "--CohortInterval"], b"--FindRelated cannot be combined with --CohortInterval"),
    (["--PileupList", "nolist.txt", "--Devices", "0,1"], b"--FindRelated cannot be combined with more than one --Devices"),
    (["--PileupList", "nolist.txt", "--RelatedTop", "0"], b"--RelatedTop takes a positive number"),
])
def test_cli_refuses_what_it_must_before_reading(tmp_path, extra, message):
    r = _cli(["--SVDPrefix", "nopanel", "--Reference", "noref.fa", "--FindRelated", "--Output", str(tmp_path / "out")] + extra,
             tmp_path)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr[-500:]
    assert os.listdir(str(tmp_path)) == []


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
    rc = lib.vb2_cohort_run_related(C.byref(ca), 3, 0, res, st, None, None)
    assert rc == _abi.VB2_ERR_INVALID
    assert b"one device" in lib.vb2_last_error()


def test_new_kernels_use_no_scratch_and_the_recorded_vgprs():
    """Notes only; no instruction is looked at."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_diff
    from test_kernel_resources_cpu import all_kernel_notes
    if not os.path.exists(LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = all_kernel_notes(LIB)
    seen = {}
    for (co, name), v in notes.items():
        m = re.search(r"\b(related_\w+_kernel|source_marginal_kernel<\w+, \w+>)\(", name)
        short = m.group(1) if m else None
        if short in VGPRS:
            print("%4d VGPRs %5d B scratch  %s" % (v["vgpr_count"], v["private_segment_fixed_size"], short))
            assert v["private_segment_fixed_size"] == 0, short
            assert v["vgpr_count"] == VGPRS[short], (short, v["vgpr_count"])
            seen[short] = seen.get(short, 0) + 1
    assert seen == {k: 1 for k in VGPRS}, seen


# ---- the restatement's own properties ----

def _one_sample(M=3000, depth=25, alpha=0.04, seed=5, known_af=False, k=2, missing=0):
    panel = sr.make_panel(M, k, seed=seed)
    G = sr.draw_individuals(panel, 2, seed=seed + 1)
    d = sr.make_sample(panel, G[0], G[1], depth, alpha, seed + 2, known_af=known_af)
    if missing:                                           # the last `missing` markers carry no read
        d.read_off = d.read_off.copy()
        d.read_off[M - missing:] = d.read_off[M - missing]
    return d


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_rows_normalise_and_vanish_off_the_counted_markers(dtype):
    d = _one_sample(missing=100)
    rng = np.random.default_rng(0)
    pc1, pc2 = rng.normal(0, 0.01, 2), rng.normal(0, 0.01, 2)
    cn = Counts(d, dtype)
    m = rr.marginals(cn, pc1, pc2, 0.04)
    live = m["live"]
    assert 2800 < live.sum() <= 2900
    eps = np.finfo(dtype).eps
    assert np.max(np.abs((m["gf2"] * m["h"]).sum(axis=1)[live] - 1)) <= 16 * eps          # sum GF2 h = 1
    assert np.max(np.abs(m["q"] - m["gf2"] * m["h"])[live]) <= 16 * eps                     # q = GF2 h
    assert np.max(np.abs(m["t"].sum(axis=1)[live] - 1)) <= 16 * eps                         # sum t = 1
    assert np.max(np.abs(m["q"] - sr.marginals(cn, pc1, pc2, 0.04)["q"])) <= 16 * eps        # section 11's q
    q, h, t = rr.panel_order(cn, d.num_marker, m)
    off = np.ones(d.num_marker, dtype=bool)
    off[cn.idx[live]] = False
    assert off.sum() >= 100 and not q[off].any() and not h[off].any() and not t[off].any()  # h = t = 0 off the counted markers


def test_floor_bounds_one_markers_veto():
    # marker 0: the target is surely one homozygote, the partner's reads allow only the other
    q = np.array([[1.0, 0.0, 0.0], [0.25, 0.5, 0.25]])
    t = np.einsum("ma,mab->mb", q, rr.transition(np.array([0.01, 0.5])))
    h = np.array([[0.0, 0.0, 3.0], [1.0, 1.0, 1.0]])
    K, shared, bound = rr.pair((q, h, t), (q, h, t))
    assert shared == 2
    assert abs(K[0] - np.log(1e-30)) <= 1e-12 and abs(K[1] - np.log(1e-30)) <= 1e-12       # DUP and PO: floored
    assert np.all(K > -70) and K[2] > np.log(0.25) - 1e-12 and K[3] > np.log(0.5) - 1e-12  # FS, D2: their k0 stands


def test_mirroring_gives_the_mirrored_samples_relations():
    d = _one_sample(alpha=0.04)
    rng = np.random.default_rng(1)
    pc1, pc2 = rng.normal(0, 0.01, 2), rng.normal(0, 0.01, 2)
    rep1, rep2 = pc1.copy(), pc2.copy()
    rep1[:2], rep2[:2] = pc2[:2], pc1[:2]                  # as the estimator reports an alpha >= 0.5
    twin = rr.rows(d, pc2, pc1, 1.0 - 0.96)
    mirrored = rr.rows(d, rep1, rep2, 0.96)
    other = rr.rows(_one_sample(seed=9), np.zeros(2), np.zeros(2), 0.02)
    for a, b in ((rr.pair(mirrored, other), rr.pair(twin, other)), (rr.pair(other, mirrored), rr.pair(other, twin))):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# The table of the feature's proposal: known allele frequencies, alpha = 1e-3 for the clean samples, the second library at
# its 0.03.  Measured with these seeds (LLR in nats, DUP / PO / FS / D2), 3 000 x 30 and 5 000 x 10:
#   A, A2          +2179 / +935 / +1188 / +551        +3395 / +1494 / +1888 / +879
#   smallest lead of the true relationship over the runner-up (all ten related pairs, both directions): 81.4 and 109.7
#   largest of the four over all eighteen unrelated pairs, both directions: -59.1 and -118.8
#   float32 rows move K_DUP(A, A2) by 5.0e-6 and 4.4e-6
@pytest.mark.parametrize("M,depth", [(3000, 30), (5000, 10)])
def test_true_relationships_separate(M, depth):
    panel = sr.make_panel(M, 2, seed=11)
    data, alphas = rr.make_family(panel, depth, 111, known_af=True)
    z = np.zeros(2)
    rows = [rr.rows(d, z, z, al if al > 0 else 1e-3) for d, al in zip(data, alphas)]
    K, shared, _ = rr.relations(rows)
    n = len(rows)
    assert np.all(np.isnan(K[np.eye(n, dtype=bool)]))
    lead, unrelated = [], []
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            k, order = K[i, j], np.argsort(K[i, j])
            true = rr.TRUE.get((min(i, j), max(i, j)))
            if true is None:
                unrelated.append(k.max())
                continue
            print("%-10s %-10s %-3s  %s" % (rr.FAMILY[i], rr.FAMILY[j], true, " ".join("%+9.1f" % x for x in k)))
            assert rr.RELATIONS[order[-1]] == true, (rr.FAMILY[i], rr.FAMILY[j], k)
            lead.append(k[order[-1]] - k[order[-2]])
    print("smallest lead %.1f, largest LLR of an unrelated pair %.1f" % (min(lead), max(unrelated)))
    assert min(lead) >= 50.0
    assert max(unrelated) <= -50.0
    r32 = [tuple(x.astype(np.float32).astype(np.float64) for x in r) for r in rows]
    shift = abs(rr.pair(r32[0], r32[1])[0][0] - K[0, 1, 0])
    print("float32 rows move K_DUP(A, A2) by %.3g" % shift)
    assert shift < 1e-3
