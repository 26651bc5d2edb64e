"""The likelihood given a hypothesised contaminant without a GPU: the additions to the ABI, the
identities of the model on the numpy restatement (tests/conditioned_ref.py) at np.longdouble against the pinned oracle and
the source statistic's restatement, the lock-step driver over the host seam (vb2_conditioned_lockstep), and the new
kernels' resources from the code-object notes."""
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
import source_ref as sr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vb2_conditioned_create", "vb2_conditioned_create_from_set", "vb2_conditioned_destroy", "vb2_conditioned_eval",
               "vb2_conditioned_optimize_llk", "vb2_conditioned_info_get", "vb2_conditioned_lockstep",
               "vb2_cohort_run_source_fits"]
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
    assert hasattr(vb, "Conditioned") and hasattr(vb, "conditioned_with_evaluator")


@pytest.fixture(scope="module")
def pair():
    """300 markers x 20, k = 2: a target contaminated at 5 % by individual 1, and individual 1's own sample."""
    panel = sr.make_panel(300, 2, seed=3)
    G = sr.draw_individuals(panel, 3, seed=4)
    target = sr.make_sample(panel, G[0], G[1], 20, 0.05, 50)
    source = sr.make_sample(panel, G[1], G[2], 20, 0.0, 51)
    z = np.zeros(2)
    q = sr.sample_rows(source, z, z, 1e-3)[1].astype(np.float32)          # what the device would hold
    return target, source, q


def _points(seed, n=6):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02, 2), rng.normal(0, 0.02, 2), a) for a in (0.0, 1e-6, 0.03, 0.5, 1.0, 0.2)][:n]


def test_an_all_zero_hypothesis_is_the_plain_likelihood(pair):
    from oracle.bridge import oracle_data
    target, _, _ = pair
    ora = oracle_data(target)
    c80 = Counts(target, np.longdouble)
    zero = np.zeros((target.num_marker, 3), dtype=np.float32)
    for pc1, pc2, a in _points(1):
        want = ora.llk(pc1, pc2, a)
        for prior in (zero, None):
            got = cr.llk(c80, prior, pc1, pc2, a)
            assert got.dtype == np.longdouble
            assert abs(float(got) - want) <= RTOL * abs(want), (a, float(got), want)


def test_at_alpha_zero_a_normalised_prior_drops_out(pair):
    from oracle.bridge import oracle_data
    target, _, q = pair
    ora = oracle_data(target)
    c80 = Counts(target, np.longdouble)
    M = target.num_marker
    onehot = [np.tile(np.eye(3, dtype=np.float32)[g], (M, 1)) for g in range(3)]
    # q as float32 sums to 1 within 2^-23 per marker; normalised in the wider format the identity is exact to rounding
    for pc1, pc2, _ in _points(2, 3):
        want = ora.llk(pc2, pc2, 0.0)
        for prior in onehot:
            got = float(cr.llk(c80, prior, pc1, pc2, 0.0))
            assert abs(got - want) <= RTOL * abs(want), (got, want)
    # ... and a prior that is not normalised shifts every marker it covers by the logarithm of its sum
    half = (0.5 * onehot[1]).astype(np.float32)
    got = float(cr.llk(c80, half, np.zeros(2), np.zeros(2), 0.0))
    want = ora.llk(np.zeros(2), np.zeros(2), 0.0) + len(c80.idx) * np.log(0.5)
    assert abs(got - want) <= RTOL * abs(want)


def test_the_difference_to_the_free_likelihood_is_the_unfloored_source_score(pair):
    target, _, q = pair
    c80 = Counts(target, np.longdouble)
    covered = 0
    for pc1, pc2, a in _points(3):
        if a in (0.0, 1.0):
            a = 0.07                      # (c is 1 at alpha = 0: covered by the identity above)
        m = sr.marginals(c80, pc1, pc2, a)
        q80 = q[c80.idx].astype(np.longdouble)
        shared = m["live"] & (q80.sum(axis=1) > 0)
        dots = (m["c"][shared] * q80[shared]).sum(axis=1)
        assert np.all(dots > 0)
        want = np.log(dots).sum()
        given, free = cr.llk(c80, q, pc1, pc2, a), cr.llk(c80, None, pc1, pc2, a)
        assert abs((given - free) - want) <= RTOL * (abs(given) + abs(free)), (a, float(given - free), float(want))
        covered += int(shared.sum())
    assert covered > 1000
    # every third marker without information: those markers take the anonymous term, the identity holds over the rest
    q3 = q.copy()
    q3[::3] = 0
    pc1, pc2, a = _points(4)[2]
    m = sr.marginals(c80, pc1, pc2, a)
    q80 = q3[c80.idx].astype(np.longdouble)
    shared = m["live"] & (q80.sum(axis=1) > 0)
    want = np.log((m["c"][shared] * q80[shared]).sum(axis=1)).sum()
    given, free = cr.llk(c80, q3, pc1, pc2, a), cr.llk(c80, None, pc1, pc2, a)
    assert 0 < shared.sum() < m["live"].sum()
    assert abs((given - free) - want) <= RTOL * (abs(given) + abs(free))


def test_there_is_no_mirror_symmetry(pair):
    target, _, q = pair
    c64 = Counts(target)
    pc1, pc2, _ = _points(5)[0]
    free = [cr.llk(c64, None, pc1, pc2, 0.3), cr.llk(c64, None, pc2, pc1, 0.7)]
    assert abs(free[0] - free[1]) <= 1e-9 * abs(free[0])
    given = [cr.llk(c64, q, pc1, pc2, 0.3), cr.llk(c64, q, pc2, pc1, 0.7)]
    assert abs(given[0] - given[1]) > 1.0


def test_a_one_hot_triple_on_one_marker_costs_the_logarithm_of_its_c(pair):
    """No floor: the veto of a single marker is log c[g] whatever its size (section 11 stops at -69 nats)."""
    target, _, q = pair
    c64 = Counts(target)
    z = np.zeros(2)
    m = sr.marginals(c64, z, z, 0.05)
    worst = int(np.argmin(m["c"].min(axis=1) + (~m["live"]) * 1e9))
    g = int(np.argmin(m["c"][worst]))
    prior = np.zeros((target.num_marker, 3), dtype=np.float32)
    prior[c64.idx[worst], g] = 1.0
    given, free = cr.llk(c64, prior, z, z, 0.05), cr.llk(c64, None, z, z, 0.05)
    want = np.log(m["c"][worst, g])
    assert want < -1.0 and abs((given - free) - want) <= 1e-11 * (abs(given) + abs(free))


# ---- the lock-step driver over the host seam ----

@pytest.fixture(scope="module")
def seam_case(pair):
    target, source, q = pair
    c64 = Counts(target)
    empty = None                          # (conditioned_ref.Evaluator: a sample that counts no marker)
    fixed = np.array([[0.011, -0.007], [0.02, 0.03], [-0.01, 0.004]])
    return c64, empty, q, fixed


@pytest.mark.parametrize("model", [dict(), dict(fix_pc=[0.01, -0.02]), dict(known_af=True)])
def test_the_driver_fixes_pc1_at_every_call_and_an_empty_hypothesis_fails_alone(seam_case, model):
    c64, empty, q, fixed = seam_case
    est, ev = cr.search([c64, empty, c64], [q, None, None], fixed, **model)
    assert [e["status"] for e in est] == [0, _abi.VB2_ERR_INVALID, 0]
    # pc1 arrives overwritten at every call -- the first (the start) and the last (llk0 at alpha = 0) included
    for num_point, pc1, pc2, alpha in ev.calls:
        assert len(num_point) == 3 and max(num_point) <= _abi.VB2_BATCH_SLOTS
        rows = np.repeat(np.arange(3), num_point)
        assert np.array_equal(pc1, fixed[rows])
    first, last = ev.calls[0], ev.calls[-1]
    assert first[0].tolist() == [1, 1, 1]
    assert all(c[0][1] == 0 for c in ev.calls[1:])                        # the empty hypothesis leaves after its first value
    assert np.all(last[3] == 0.0) and np.array_equal(last[1], fixed[np.repeat(np.arange(3), last[0])])
    for h in (0, 2):
        e = est[h]
        prior = q if h == 0 else None
        assert np.array_equal(e["pc"], e["pc2"])
        if "fix_pc" in model:
            assert np.array_equal(e["pc2"], model["fix_pc"])
        # llk1 and llk0 are the restatement's values at the returned point and at alpha = 0 under the fixed pc1
        assert -e["llk1"] == float(cr.llk(c64, prior, fixed[h], e["pc2"], e["alpha"]))
        assert -e["llk0"] == float(cr.llk(c64, prior, fixed[h], e["pc2"], 0.0))
        assert e["llk1"] <= e["llk0"] and 0.0 < e["alpha"] < 1.0
    # given the true source the fit finds the contamination
    assert abs(est[0]["alpha"] - 0.05) < 0.03


def test_an_evaluator_error_ends_every_search(seam_case):
    c64, empty, q, fixed = seam_case
    ev = cr.Evaluator([c64, c64], [q, None])
    seen = []

    def evaluate(num_point, pc1, pc2, alpha):
        seen.append(1)
        if len(seen) == 3:
            raise RuntimeError("evaluator gave up")
        return ev(num_point, pc1, pc2, alpha)

    with pytest.raises(RuntimeError, match="evaluator gave up"):
        vb.conditioned_with_evaluator(evaluate, 2, 2, fixed[:2])
    assert len(seen) == 3


def test_a_fixed_alpha_is_refused(seam_case):
    c64, empty, q, fixed = seam_case
    with pytest.raises(_abi.Vb2Error, match="fixed alpha"):
        vb.conditioned_with_evaluator(cr.Evaluator([c64], [q]), 1, 2, fixed[:1], fix_alpha=0.02)


@pytest.mark.parametrize("flags, message", [
    (["--RefitSource"], "--RefitSource needs --FindSource"),
    (["--FindSource", "--RefitSource", "--FixAlpha", "0.01"], "--RefitSource cannot be combined with --FixAlpha"),
    (["--FindSource", "--RefitSource", "--CohortInterval"], "--RefitSource cannot be combined with --CohortInterval"),
    (["--FindSource", "--RefitSource", "--Devices", "0,1"], "--RefitSource cannot be combined with more than one --Devices"),
])
def test_command_line_refusals(flags, message, tmp_path):
    # (none of the named files exists: the refusal comes before any of them is opened, and no device is needed)
    p = subprocess.run([EXE, "--SVDPrefix", "nopanel", "--Reference", "NA", "--PileupList", "nolist.txt", "--Output",
                        str(tmp_path / "out")] + flags, capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode != 0
    assert message in p.stderr, p.stderr
    assert p.stdout == "" and os.listdir(str(tmp_path)) == []


def test_the_entry_refuses_before_reading():
    import ctypes as C
    lib = _abi.lib()
    ca = _abi.CohortArgs()
    ca.base.ud_path, ca.base.mean_path, ca.base.bed_path = b"nopanel.UD", b"nopanel.mu", b"nopanel.bed"
    ca.base.num_pc = 2
    piles = (C.c_char_p * 1)(b"no.pileup")
    ca.num_sample, ca.pileup_paths = 1, piles
    res, st = (_abi.RunResult * 1)(), (C.c_int32 * 1)()
    ca.base.model.is_alpha_fixed, ca.base.model.fix_alpha = 1, 0.01
    assert lib.vb2_cohort_run_source_fits(C.byref(ca), 3, res, st, None, None, None) == _abi.VB2_ERR_INVALID
    assert b"--FixAlpha" in lib.vb2_last_error()
    ca.base.model.is_alpha_fixed = 0
    devs = (C.c_int32 * 2)(0, 1)
    ca.base.devices, ca.base.num_device = devs, 2
    assert lib.vb2_cohort_run_source_fits(C.byref(ca), 3, res, st, None, None, None) == _abi.VB2_ERR_INVALID
    assert b"one device" in lib.vb2_last_error()


def test_the_seeded_cohort_gives_what_the_gpu_suite_asserts():
    """The cohort of the end-to-end test on the CPU: with the pinned oracle's free fits, the restatements rank sample 1
    first for sample 0 and the refit given it beats the anonymous maximum; sample 2's contaminant is nobody of the cohort
    (every score negative: no refit).  Measured with FIT_SEED = 42: LLR +398.40, ALPHA_GIVEN 0.053203, DELTA_LK +398.41;
    sample 2's best candidate -772.1."""
    from oracle.bridge import oracle_data
    panel, data = cr.fit_cohort()
    est = [oracle_data(d).optimize() for d in data]
    zero, two = cr.expected_refit(data, est, 0), cr.expected_refit(data, est, 2)
    print("sample 0: %r\nsample 2: %r" % (zero, two))
    assert zero["candidate"] == 1 and zero["llr"] > 0 and zero["delta_lk"] > 0
    assert abs(zero["alpha_given"] - 0.05) < 0.01
    assert two["llr"] < 0 and two["delta_lk"] is None


def test_conditioned_kernels_fit_the_weighted_kernels_budget():
    """Note-only, like tests/test_replicates_cpu.py: the six prior-term instantiations of llk_sum_marker_kernel
    (marker_sum_kernels.hip), the reduction and the permutation live in one code object -- the weight term's --, use no
    scratch memory, the weight term's LDS, and each marker kernel at most 8 VGPRs more than the weight-term kernel of the
    same layout and --NumPC selection."""
    import test_kernel_resources_cpu as res
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = res.all_kernel_notes(res.LIB)
    short = lambda name: re.search(r"(\w+_kernel(<[^>]*>)?)\(", name).group(1)
    mine = {short(k[1]): (k[0], v) for k, v in notes.items()
            if re.search(r"llk_sum_marker_kernel<[^>]*PriorTerm|llk_sum_reduce_kernel|prior_permute_kernel", k[1])}
    theirs = {short(k[1]): (k[0], v) for k, v in notes.items() if re.search(r"llk_sum_marker_kernel<[^>]*WeightTerm", k[1])}
    twin_of = lambda name: theirs.get(name.replace("PriorTerm", "WeightTerm"), (None, None))
    for name, (obj, v) in sorted(mine.items()):
        twin = (twin_of(name)[1] or {}).get("vgpr_count", -1)
        print("%4d VGPRs (weighted: %4d) %5d B scratch  %s  [%s]" % (v["vgpr_count"], twin, v["private_segment_fixed_size"], name, obj))
    marker = sorted(n for n in mine if n.startswith("llk_sum_marker_kernel<"))
    assert len(marker) == 6, marker                      # PD x KSEL 0, 2, 4
    assert len(mine) == 8 and len({obj for obj, _ in mine.values()} | {obj for obj, _ in theirs.values()}) == 1, sorted(mine)
    for name, (_, v) in mine.items():
        assert v["private_segment_fixed_size"] == 0, name
        twin = twin_of(name)[1]
        if twin is None:
            continue
        assert v["vgpr_count"] <= twin["vgpr_count"] + 8, (name, v["vgpr_count"], twin["vgpr_count"])
    assert sum(1 for n in marker if twin_of(n)[1] is not None) == 6
    # LDS: the table and the tree are dynamic, sized by the one launcher of both terms (at most 189 rows x 48 B + 2 KB =
    # 11 KB); the marker kernel declares no other shared memory, and nothing in the unit or the walk it includes is atomic
    csrc = os.path.join(ROOT, "verifybamid_amd", "csrc")
    src, walk = (open(os.path.join(csrc, n)).read() for n in ("marker_sum_kernels.hip", "marker_walk.h"))
    size = "const size_t shmem = ((size_t)nrow * kRowDoubles + kThreads) * sizeof(double);"
    assert src.count(size) == 1 and src.count("constexpr int kRowDoubles = 6;") == 1
    assert walk.count("constexpr int kThreads = 256;") == 1 and "kThreads =" not in src
    assert src.count("__shared__") == 2 and "__shared__" not in walk            # the marker kernel's table, the reduction's tree
    assert "atomic" not in src.lower() and "atomic" not in walk.lower()
