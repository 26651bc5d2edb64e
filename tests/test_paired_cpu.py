"""The likelihood given priors on both components without a GPU: the additions to the ABI, the six
identities of the model on the numpy restatement (tests/paired_ref.py) at np.longdouble against the pinned oracle and the
section 13 restatement, the lock-step driver over the host seam (vb2_paired_lockstep), the new kernels' resources from the
code-object notes, and the point of the feature: a tumour's allelic imbalance passes for contamination in the anonymous
fit and not in the fit given the matched normal."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioned_ref as cr  # noqa: E402
import paired_ref as pr  # noqa: E402
import replicate_ref as rr  # noqa: E402
import source_ref as sr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vb2_paired_create", "vb2_paired_create_from_set", "vb2_paired_destroy", "vb2_paired_eval",
               "vb2_paired_optimize_llk", "vb2_paired_info_get", "vb2_paired_lockstep", "vb2_cohort_run_paired",
               "vb2_matched_normal_read"]
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
RTOL = 1e-12                      # the project's evaluation tolerance


def test_new_symbols_and_the_abi_is_still_7():
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.vb2_abi_version() == 7
    assert re.search(r"#define VB2_ABI_VERSION 7\b", header)
    assert hasattr(vb, "Paired") and hasattr(vb, "paired_with_evaluator")


@pytest.fixture(scope="module")
def pair():
    """300 markers x 20, k = 2: a tumour contaminated at 5 % by individual 1, and its normal's posterior as the device
    would hold it."""
    panel = sr.make_panel(300, 2, seed=3)
    G = sr.draw_individuals(panel, 3, seed=4)
    tumour = sr.make_sample(panel, G[0], G[1], 20, 0.05, 50)
    normal = sr.make_sample(panel, G[0], G[2], 20, 0.0, 51)
    return tumour, pr.normal_q(normal)


def _points(seed, n=6):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02, 2), rng.normal(0, 0.02, 2), a) for a in (0.0, 1e-6, 0.03, 0.5, 1.0, 0.25)][:n]


def _close(got, want, rtol=RTOL):
    got, want = float(got), float(want)
    assert abs(got - want) <= rtol * abs(want), (got, want)


def test_identity_1_with_pi2_all_zero_it_is_the_conditioned_likelihood(pair):
    tumour, q = pair
    c80 = Counts(tumour, np.longdouble)
    third = q.copy()
    third[::3] = 0
    for prior in (q, third):
        for pc1, pc2, a in _points(1):
            got = pr.llk(c80, pr.hypothesis(300, pi1=prior), pc1, pc2, a)
            assert got.dtype == np.longdouble
            _close(got, cr.llk(c80, prior, pc1, pc2, a))


def test_identity_2_with_both_all_zero_it_is_the_plain_likelihood(pair):
    from oracle.bridge import oracle_data
    tumour, _ = pair
    ora = oracle_data(tumour)
    c80 = Counts(tumour, np.longdouble)
    for pc1, pc2, a in _points(2):
        for hyp in (pr.hypothesis(300), None):
            _close(pr.llk(c80, hyp, pc1, pc2, a), ora.llk(pc1, pc2, a))


def test_identity_3_leaving_markers_out_is_a_zero_one_weight(pair):
    tumour, _ = pair
    c80 = Counts(tumour, np.longdouble)
    w = (np.random.default_rng(5).random(300) < 0.6).astype(np.uint8)
    ora = rr.ExpandedOracle(tumour, w[None])
    hyp = pr.hypothesis(300)
    hyp[w == 0, 3:] = pr.LEFT_OUT
    assert 0 < pr.given_count(c80, hyp) < len(c80.idx)
    for pc1, pc2, a in _points(3):
        _close(pr.llk(c80, hyp, pc1, pc2, a), ora.llk(0, pc1, pc2, a))
    # nothing walked: 0.0
    hyp[:, 3:] = pr.LEFT_OUT
    assert pr.llk(c80, hyp, np.zeros(2), np.zeros(2), 0.1) == 0 and pr.given_count(c80, hyp) == 0


def test_identity_4_the_mirror(pair):
    """The only identity with a prior on both sides at once.  alpha with an exact complement."""
    tumour, q = pair
    c80 = Counts(tumour, np.longdouble)
    rng = np.random.default_rng(6)
    a = rng.dirichlet(np.ones(3), 300).astype(np.float32)
    b = q.copy()
    b[::4] = 0                                                # some markers fall back on the b side
    b[1::7] = pr.LEFT_OUT                                     # (left out where b is pi2 only: both orders leave them out below)
    out = b[:, 0] < 0
    b_as_pi1 = np.where(out[:, None], np.float32(0), b)
    ha, hb = pr.hypothesis(300, pi1=a, pi2=b), pr.hypothesis(300, pi1=b_as_pi1, pi2=a)
    hb[out, 3:] = pr.LEFT_OUT
    for (pc1, pc2, _), alpha in zip(_points(4), (0.25, 0.5, 0.75, 0.125, 0.0, 1.0)):
        left, right = pr.llk(c80, ha, pc1, pc2, alpha), pr.llk(c80, hb, pc2, pc1, 1.0 - alpha)
        assert left != 0
        _close(left, right)
    # ... and it is no symmetry of one hypothesis: swapping the sides' arguments alone changes the value
    assert abs(pr.llk(c80, ha, pc1, pc2, 0.25) - pr.llk(c80, ha, pc2, pc1, 0.75)) > 1.0


def test_identity_5_both_one_hot_on_one_genotype_reads_alpha_out(pair):
    tumour, _ = pair
    c80 = Counts(tumour, np.longdouble)
    eye = np.eye(3, dtype=np.float32)
    for g in range(3):
        hyp = pr.hypothesis(300, pi1=np.tile(eye[g], (300, 1)), pi2=np.tile(eye[g], (300, 1)))
        want = pr.diagonal_constants(c80, g)
        for pc1, pc2, a in _points(7):
            _close(pr.llk(c80, hyp, pc1, pc2, a), want)


def test_identity_6_alpha_is_the_other_components_share_and_is_not_folded(pair):
    """A sample that is 70 % one individual, given the genotypes of the 30 % individual as the INTENDED one: the fit
    reports alpha near 0.7 -- the share of the component that is not the intended one -- not 0.3."""
    panel = sr.make_panel(300, 2, seed=3)
    G = sr.draw_individuals(panel, 3, seed=4)
    mix = sr.make_sample(panel, G[0], G[1], 30, 0.7, 60)      # 30 % individual 0, 70 % individual 1
    q0 = pr.normal_q(sr.make_sample(panel, G[0], G[2], 30, 0.0, 61))
    est, given = pr.paired_fit(mix, q0, np.zeros(2), hom_min=0.0)
    print("alpha %.4f over %d markers" % (est["alpha"], given))
    assert est["status"] == 0 and abs(est["alpha"] - 0.7) < 0.1


# ---- the lock-step driver over the host seam ----

@pytest.mark.parametrize("model", [dict(), dict(fix_pc=[0.01, -0.02]), dict(known_af=True)])
def test_the_driver_fixes_pc2_at_every_call_and_an_empty_hypothesis_fails_alone(pair, model):
    tumour, q = pair
    c64 = Counts(tumour)
    fixed = np.array([[0.011, -0.007], [0.02, 0.03], [-0.01, 0.004]])
    nothing = pr.hypothesis(300)
    nothing[:, 3:] = pr.LEFT_OUT
    hyps = [pr.normal_rule(q, 0.99), nothing, pr.normal_rule(q, 0.0)]
    est, ev = pr.search([c64] * 3, hyps, fixed, **model)
    assert [e["status"] for e in est] == [0, _abi.VB2_ERR_INVALID, 0]
    # pc2 arrives overwritten at every call -- the first (the start) and the last (llk0 at alpha = 0) included
    for num_point, pc1, pc2, alpha in ev.calls:
        assert len(num_point) == 3 and max(num_point) <= _abi.VB2_BATCH_SLOTS
        assert np.array_equal(pc2, fixed[np.repeat(np.arange(3), num_point)])
    first, last = ev.calls[0], ev.calls[-1]
    assert first[0].tolist() == [1, 1, 1]
    assert all(c[0][1] == 0 for c in ev.calls[1:])                        # the empty hypothesis leaves after its first value
    assert np.all(last[3] == 0.0)
    for h in (0, 2):
        e = est[h]
        if "fix_pc" in model:
            assert np.array_equal(e["pc"], model["fix_pc"])
        # llk1 and llk0 are the restatement's values at the returned point and at alpha = 0 under the fixed pc2
        assert -e["llk1"] == float(pr.llk(c64, hyps[h], e["pc"], fixed[h], e["alpha"]))
        assert -e["llk0"] == float(pr.llk(c64, hyps[h], e["pc"], fixed[h], 0.0))
        assert e["llk1"] <= e["llk0"] and 0.0 < e["alpha"] < 1.0


def test_a_fixed_alpha_is_refused(pair):
    tumour, q = pair
    with pytest.raises(_abi.Vb2Error, match="fixed alpha"):
        vb.paired_with_evaluator(pr.Evaluator([Counts(tumour)], [pr.normal_rule(q, 0.99)]), 1, 2, np.zeros((1, 2)),
                                 fix_alpha=0.02)


def test_an_evaluator_error_ends_every_search(pair):
    tumour, q = pair
    c64 = Counts(tumour)
    ev = pr.Evaluator([c64, c64], [pr.normal_rule(q, 0.99), None])
    seen = []

    def evaluate(num_point, pc1, pc2, alpha):
        seen.append(1)
        if len(seen) == 3:
            raise RuntimeError("evaluator gave up")
        return ev(num_point, pc1, pc2, alpha)

    with pytest.raises(RuntimeError, match="evaluator gave up"):
        vb.paired_with_evaluator(evaluate, 2, 2, np.zeros((2, 2)))
    assert len(seen) == 3


def test_the_normal_rule():
    q = np.array([[0.995, 0.005, 0], [0.5, 0.5, 0], [0, 0, 0], [0, 0.01, 0.99], [0.98, 0.02, 0], [0, 0, 1]], dtype=np.float32)
    at = lambda tau: (pr.normal_rule(q, tau)[:, 3] >= 0).tolist()
    assert at(0.99) == [True, False, False, True, False, True]      # (float32 0.99 widened is >= 0.99)
    assert at(0.0) == [True, True, False, True, True, True]          # every marker the normal counts
    assert at(1.0) == [False, False, False, False, False, True]
    h = pr.normal_rule(q, 0.99)
    assert not h[:, :3].any() and np.array_equal(h[0, 3:], q[0]) and np.array_equal(h[1, 3:], pr.LEFT_OUT)


# ---- the point of the feature ----

def test_an_allelic_imbalance_passes_for_contamination_only_without_the_normal():
    """3 000 x 30, k = 2, a tumour contaminated at 0.03 by an outsider, half its markers at a reference fraction of 0.7 where
    it is heterozygous (paired_ref.pair_case, seed 42).  Measured on the restatements: anonymous fit 0.039783, paired fit
    (2 048 markers where the normal is homozygous at 0.99) 0.029349; without the shift 0.029348 and 0.029349.  The
    assertions are relative.  "Agree without the shift" is taken as: the two fits differ by less there than under the shift,
    and by less than either is from the planted value's neighbourhood -- no absolute alpha is asserted."""
    from oracle.bridge import oracle_data
    planted = 0.03
    panel, shifted, plain, normal, _ = pr.pair_case(alpha=planted)
    en = oracle_data(normal).optimize()
    pc2 = sr.search_point(en["pc"], en["pc2"], en["alpha"])[1]
    q = pr.normal_q(normal, en)
    out = {}
    for name, t in (("shifted", shifted), ("plain", plain)):
        anon = oracle_data(t).optimize()["alpha"]
        fit, given = pr.paired_fit(t, q, pc2)
        assert fit["status"] == 0 and 0 < given < 3000
        out[name] = (anon, fit["alpha"])
        print("%s: anonymous %.6f, paired %.6f over %d markers (planted %.3f)" % (name, anon, fit["alpha"], given, planted))
    anon, paired = out["shifted"]
    assert abs(paired - planted) < abs(anon - planted)
    gap_shifted, gap_plain = abs(anon - paired), abs(out["plain"][0] - out["plain"][1])
    assert gap_plain < gap_shifted


def test_the_seeded_cohort_gives_what_the_gpu_suite_asserts():
    """The cohort of the end-to-end test on the CPU, with the pinned oracle's free fits: the tumour with the imbalance
    (sample 0, planted 0.03) is closer to its planted value given its normal than anonymously; the tumour without
    (sample 2, planted 0.05) moves less."""
    from oracle.bridge import oracle_data
    panel, data = pr.pair_cohort()
    est = [oracle_data(d).optimize() for d in data[:4]]
    gaps = {}
    for t, n in pr.COHORT_PAIRS:
        want = pr.expected_pair(data, est, t, n)
        planted = pr.COHORT_PLANTED[t]
        print("tumour %d: FREEMIX %.6f, ALPHA_PAIRED %.6f over %d markers (planted %.3f); normal FREEMIX %.6f"
              % (t, want["freemix"], want["alpha_paired"], want["markers"], planted, min(est[n]["alpha"], 1 - est[n]["alpha"])))
        assert want["status"] == 0 and 1000 < want["markers"] < 3000
        gaps[t] = (abs(want["freemix"] - planted), abs(want["alpha_paired"] - planted), abs(want["freemix"] - want["alpha_paired"]))
    assert gaps[0][1] < gaps[0][0]
    assert gaps[2][2] < gaps[0][2]


# ---- the command line and the entry point, without a device ----

BASE = ["--SVDPrefix", "nopanel", "--Reference", "NA"]


@pytest.mark.parametrize("flags, message", [
    (["--MatchedNormal", "p.txt"], "--MatchedNormal needs --PileupList"),
    (["--PileupList", "l.txt", "--NormalHomMin", "0.9"], "--NormalHomMin needs --MatchedNormal"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--FixAlpha", "0.01"], "--MatchedNormal cannot be combined with --FixAlpha"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--CohortInterval"], "--MatchedNormal cannot be combined with --CohortInterval"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--FindSource"], "--MatchedNormal cannot be combined with --FindSource"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--FindSource", "--RefitSource"],
     "--MatchedNormal cannot be combined with --RefitSource"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--FindRelated"], "--MatchedNormal cannot be combined with --FindRelated"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--Devices", "0,1"],
     "--MatchedNormal cannot be combined with more than one --Devices"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--NormalHomMin", "1.5"], "--NormalHomMin takes a probability within [0, 1]"),
    (["--PileupList", "l.txt", "--MatchedNormal", "p.txt", "--NormalHomMin", "-0.1"], "--NormalHomMin takes a probability within [0, 1]"),
])
def test_command_line_refusals(flags, message, tmp_path):
    # (none of the named files exists: the refusal comes before any of them is opened, and no device is needed)
    p = subprocess.run([EXE] + BASE + ["--Output", str(tmp_path / "out")] + flags, capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode != 0
    assert message in p.stderr, p.stderr
    assert p.stdout == "" and os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("pairs, message", [
    ("t1.pileup\tn1.pileup\nt2.pileup\tnobody.pileup\n", "line 2: 'nobody.pileup' is not a pileup of the --PileupList"),
    ("t1.pileup\tn1.pileup\nt1.pileup\tn2.pileup\n", "line 2: the tumour 't1.pileup' is listed twice"),
    ("t1.pileup\tt1.pileup\n", "line 1: 't1.pileup' is paired with itself"),
    ("t1.pileup n1.pileup\n", "line 1: expected TUMOUR<TAB>NORMAL"),
    ("\n", "names no pair"),
])
def test_the_pairs_file_is_validated_before_any_device_work(pairs, message, tmp_path):
    """The list and the pairs exist, the panel and the pileups do not: the message comes before anything else is read."""
    with open(str(tmp_path / "l.txt"), "w") as f:
        for name in ("t1", "n1", "t2", "n2"):
            f.write("%s.pileup\t%s\n" % (name, name))
    with open(str(tmp_path / "p.txt"), "w") as f:
        f.write(pairs)
    p = subprocess.run([EXE] + BASE + ["--Output", "out", "--PileupList", "l.txt", "--MatchedNormal", "p.txt"], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert p.returncode != 0 and message in p.stderr, p.stderr
    assert "nopanel" not in p.stderr                               # (the panel was never asked for)
    assert p.stdout == "" and sorted(os.listdir(str(tmp_path))) == ["l.txt", "p.txt"]
    # a good file passes this stage: the run then fails on the panel it cannot open
    with open(str(tmp_path / "p.txt"), "w") as f:
        f.write("t1.pileup\tn1.pileup\nt2.pileup\tn1.pileup\n")   # (a normal may serve two tumours)
    p = subprocess.run([EXE] + BASE + ["--Output", "out", "--PileupList", "l.txt", "--MatchedNormal", "p.txt"], capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert p.returncode != 0 and "MatchedNormal" not in p.stderr.split("FATAL ERROR")[-1], p.stderr


def test_reading_the_pairs_file(tmp_path):
    lib = _abi.lib()
    names = (C.c_char_p * 4)(b"a/t1.pileup", b"a/n1.pileup", b"t2.pileup", b"n2.pileup")
    path = str(tmp_path / "p.txt")
    with open(path, "w") as f:
        f.write("t2.pileup\tn2.pileup\n\na/t1.pileup\ta/n1.pileup\r\n")
    n, t, m = C.c_int32(0), (C.c_int32 * 4)(), (C.c_int32 * 4)()
    assert lib.vb2_matched_normal_read(path.encode(), 4, names, C.byref(n), t, m) == 0
    assert n.value == 2 and list(t)[:2] == [2, 0] and list(m)[:2] == [3, 1]
    assert lib.vb2_matched_normal_read(b"/nonexistent/p.txt", 4, names, C.byref(n), t, m) == _abi.VB2_ERR_IO


def test_the_entry_refuses_before_reading():
    lib = _abi.lib()
    ca = _abi.CohortArgs()
    ca.base.ud_path, ca.base.mean_path, ca.base.bed_path = b"nopanel.UD", b"nopanel.mu", b"nopanel.bed"
    ca.base.num_pc = 2
    piles = (C.c_char_p * 3)(b"a.pileup", b"b.pileup", b"c.pileup")
    ca.num_sample, ca.pileup_paths = 3, piles
    res, st = (_abi.RunResult * 3)(), (C.c_int32 * 3)()
    run = lambda t, n, tau=0.99: lib.vb2_cohort_run_paired(C.byref(ca), len(t), (C.c_int32 * len(t))(*t), (C.c_int32 * len(n))(*n),
                                                           tau, res, st, None)
    for t, n, tau, word in [([0], [0], 0.99, b"paired with itself"), ([0, 0], [1, 2], 0.99, b"listed twice"),
                            ([3], [1], 0.99, b"outside the cohort"), ([0], [1], 1.01, b"--NormalHomMin"),
                            ([0], [1], float("nan"), b"--NormalHomMin")]:
        assert run(t, n, tau) == _abi.VB2_ERR_INVALID
        assert word in lib.vb2_last_error(), lib.vb2_last_error()
    ca.base.model.is_alpha_fixed, ca.base.model.fix_alpha = 1, 0.01
    assert run([0], [1]) == _abi.VB2_ERR_INVALID and b"--FixAlpha" in lib.vb2_last_error()
    ca.base.model.is_alpha_fixed = 0
    devs = (C.c_int32 * 2)(0, 1)
    ca.base.devices, ca.base.num_device = devs, 2
    assert run([0], [1]) == _abi.VB2_ERR_INVALID and b"one device" in lib.vb2_last_error()


# ---- the kernels' resources ----

def test_paired_kernels_resources():
    """Note-only, like tests/test_conditioned_cpu.py: the six pair-term instantiations of llk_sum_marker_kernel, the
    permutation and the builder live in the weight term's code object, use no scratch memory and at most the project's 128
    VGPRs."""
    import test_kernel_resources_cpu as res
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = res.all_kernel_notes(res.LIB)
    short = lambda name: re.search(r"(\w+_kernel(<[^>]*>)?)\(", name).group(1)
    mine = {short(k[1]): (k[0], v) for k, v in notes.items()
            if re.search(r"llk_sum_marker_kernel<[^>]*PairTerm|pair_permute_kernel|pair_build_kernel", k[1])}
    theirs = {k[0] for k, v in notes.items() if re.search(r"llk_sum_marker_kernel<[^>]*WeightTerm", k[1])}
    for name, (obj, v) in sorted(mine.items()):
        print("%4d VGPRs %5d B scratch  %s  [%s]" % (v["vgpr_count"], v["private_segment_fixed_size"], name, obj))
    marker = sorted(n for n in mine if n.startswith("llk_sum_marker_kernel<"))
    assert len(marker) == 6, marker                      # PD x KSEL 0, 2, 4
    assert len(mine) == 8 and {obj for obj, _ in mine.values()} == theirs and len(theirs) == 1, sorted(mine)
    for name, (_, v) in mine.items():
        assert v["private_segment_fixed_size"] == 0, name
        assert v["vgpr_count"] <= 128, (name, v["vgpr_count"])
