"""The reference bias without a GPU: the additions to the ABI, the identities
of the model on the numpy restatement (tests/refbias_ref.py), the estimate of beta over the host seam (vb2_refbias_lockstep)
on the seeded samples of refbias_ref -- which this file confirms --, the argument errors and the command line's refusals.

The seeds (3 000 x 30, k = 2, q30 reads, alpha = 0.03), on the float64 restatement:

    FIT_SEED  = 11, beta planted at 0.58:  beta 0.57998, SE 0.00303, LRT 684.3, FREEMIX 0.02886 fitted / 0.03028 at 0.5
    NULL_SEED = 12, beta planted at 0.5:   beta 0.49828, SE 0.00310, LRT 0.31
"""
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
import refbias_ref as rr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
NEW_SYMBOLS = ["vb2_refbias_create", "vb2_refbias_destroy", "vb2_refbias_eval", "vb2_refbias_optimize_llk", "vb2_refbias_info_get",
               "vb2_refbias_fit_ctx", "vb2_refbias_lockstep", "vb2_run_refbias"]
ALPHAS = (0.0, 1e-6, 0.03, 0.5, 1.0, 0.2)


def test_new_symbols_and_the_abi_is_still_7():
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.vb2_abi_version() == 7
    assert re.search(r"#define VB2_ABI_VERSION 7\b", header)
    assert hasattr(vb, "RefBias") and hasattr(vb, "refbias_with_evaluator")
    # the struct as the header lays it out: 4 + 2 x 64 + 3 + 2 x 28 doubles, one int64, six int32
    import ctypes
    assert ctypes.sizeof(_abi.RefBiasFit) == 8 * (4 + 128 + 3 + 56) + 8 + 24


def _points(seed, k):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02, k), rng.normal(0, 0.02, k), a) for a in ALPHAS]


@pytest.fixture(scope="module")
def samples():
    """300 x 20 with the wide range of qualities, k = 2 and k = 4 with known allele frequencies."""
    a = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=5, q_lo=2, q_hi=60, missing_frac=0.1)
    b = vb.synth.make_pileup(300, mean_depth=20, num_pc=4, alpha_true=0.05, seed=6)
    b.known_af = np.clip(b.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, 300), 0.0, 1.0)
    return a, b


def test_at_one_half_the_restatement_is_the_plain_likelihoods(samples):
    for d in samples:
        for T in (np.float64, np.longdouble):
            c = Counts(d, T)
            for pc1, pc2, a in _points(1, d.num_pc):
                got, want = rr.llk(c, 0.5, pc1, pc2, a), cr.llk(c, None, pc1, pc2, a)
                assert got.dtype == np.dtype(T) and got == want, (a, got, want)
    c = Counts(samples[0])
    z = np.zeros(2)
    assert rr.llk(c, 0.5, z, z, 1.5) == 0 and rr.llk(c, 0.58, z, z, -0.1) == 0
    assert rr.llk(c, 0.58, z, z, 0.03) != rr.llk(c, 0.5, z, z, 0.03)


def test_reflection_identity(samples):
    """REF and ALT exchanged: llk(beta) of the exchanged sample is llk(1 - beta) of the original.  Every term of the 80-bit
    restatement is the same number on both sides up to the rounding of 1 - beta, 2 - mu and the order of the nine terms."""
    for d in samples:
        c = Counts(d, np.longdouble)
        x = rr.exchanged(c)
        for beta in (0.25, 0.4375, 0.58, 0.75):
            for pc1, pc2, a in _points(2, d.num_pc):
                got, want = rr.llk(x, beta, pc1, pc2, a), rr.llk(c, 1.0 - beta, pc1, pc2, a)
                assert abs(got - want) <= 1e-15 * abs(want), (beta, a, got, want)
        # ... and it is no identity of the sample itself
        z = np.zeros(d.num_pc)
        assert abs(rr.llk(c, 0.58, z, z, 0.03) - rr.llk(c, 0.42, z, z, 0.03)) > 1e-6 * abs(rr.llk(c, 0.5, z, z, 0.03))


def test_only_entries_with_a_heterozygote_depend_on_beta():
    quals = np.array([2, 20, 37])
    t0 = rr._table(0.03, 0.5, quals, np.float64).reshape(2, 3, 3, 3)
    t1 = rr._table(0.03, 0.625, quals, np.float64).reshape(2, 3, 3, 3)
    het = np.zeros((3, 3), dtype=bool)
    het[1, :] = het[:, 1] = True
    assert np.all((t0 != t1) == het[None, None])
    # class alt is class ref at 1 - beta, read mirrored
    m = rr._table(0.03, 0.375, quals, np.float64).reshape(2, 3, 3, 3)
    assert np.array_equal(t1[1], m[0][:, ::-1, ::-1])


@pytest.fixture(scope="module")
def planted():
    d = rr.fit_sample()
    ev = rr.Evaluator(Counts(d))
    return d, ev, vb.refbias_with_evaluator(ev, 2)


def test_the_planted_bias_is_found(planted):
    d, ev, f = planted
    print("planted 0.58: beta %.5f, SE %.5f, LRT %.2f, FREEMIX %.5f with the bias fitted, %.5f at 0.5; %d steps"
          % (f["beta"], f["beta_se"], f["lrt"], f["freemix_bias"], min(f["alpha_at_half"], 1 - f["alpha_at_half"]), f["num_step"]))
    assert f["status"] == 0 and not f["at_bound"]
    assert abs(f["beta"] - 0.58) <= 3 * f["beta_se"] and 0 < f["beta_se"] < 0.01
    assert f["lrt"] > 3.84
    assert f["lrt"] == 2 * (f["llk1_bias"] - f["llk1_at_half"])
    assert abs(f["freemix_bias"] - 0.03) < 0.01


def test_the_procedure_is_28_searches_in_five_calls(planted):
    d, ev, f = planted
    pairs = f["pairs"]
    assert len(pairs) == 28 and f["num_refit"] == 28 and f["num_round"] == 4
    calls = ev.lockstep_calls()
    assert [len(b) for b in calls] == [9, 6, 6, 6, 1]                    # four rounds and the final search
    assert f["num_step"] == len(ev.calls)
    beta = np.array([b for b, _ in pairs])
    assert np.array_equal(beta[:9], 0.25 + np.arange(9) / 16.0) and beta[4] == 0.5
    assert np.array_equal(np.concatenate(calls), beta)
    assert pairs[4][1] == f["llk1_at_half"] and pairs[27] == (f["beta"], f["llk1_bias"])
    # every round's six new values: between the neighbours of the best value so far, the ends and the centre kept
    gs, ls = [b for b, _ in pairs[:9]], [v for _, v in pairs[:9]]
    for r, h in enumerate((2.0 ** -6, 2.0 ** -8, 2.0 ** -10)):
        new = pairs[9 + 6 * r: 15 + 6 * r]
        c = min(max(int(np.argmax(ls)), 1), 7)                           # (argmax: the lowest index on ties)
        lo, keep = gs[c - 1], (ls[c - 1], ls[c], ls[c + 1])
        assert [b for b, _ in new] == [lo + i * h for i in (1, 2, 3, 5, 6, 7)], (r, new)
        gs = [lo + i * h for i in range(9)]
        ls = [keep[0]] + [v for _, v in new[:3]] + [keep[1]] + [v for _, v in new[3:]] + [keep[2]]
    # the estimate: the vertex through the last round's best value and its neighbours; the SE from its ends and centre
    ls = np.array(ls)
    b = int(np.argmax(ls))
    assert 0 < b < 8
    vertex = gs[b] + 0.5 * 2.0 ** -10 * (ls[b - 1] - ls[b + 1]) / (ls[b - 1] - 2 * ls[b] + ls[b + 1])
    assert abs(f["beta"] - vertex) <= 1e-15
    curv = (ls[0] - 2 * ls[4] + ls[8]) / (2.0 ** -8) ** 2
    assert abs(f["beta_se"] - np.sqrt(-1 / curv)) <= 1e-12
    # a search of the procedure is the row's own refit
    again = rr.search(Counts(d), [0.5])[0]
    assert -again["llk1"] == f["llk1_at_half"] and again["alpha"] == f["alpha_at_half"]


def test_without_a_bias_the_test_does_not_reject():
    d = rr.fit_sample(rr.NULL_SEED, 0.5)
    f = vb.refbias_with_evaluator(rr.Evaluator(Counts(d)), 2)
    print("planted 0.5: beta %.5f, SE %.5f, LRT %.2f" % (f["beta"], f["beta_se"], f["lrt"]))
    assert f["status"] == 0 and 0 <= f["lrt"] < 3.84
    assert abs(f["beta"] - 0.5) <= 3 * f["beta_se"]
    assert len(f["pairs"]) == 28


def test_argument_errors():
    L = _abi.lib()
    import ctypes as C
    m, _ = vb.api._model()
    fit = _abi.RefBiasFit()
    fn = _abi.REFBIAS_EVAL_FN(lambda *a: 0)
    # null pointers
    assert L.vb2_refbias_lockstep(C.cast(None, _abi.REFBIAS_EVAL_FN), None, 2, C.byref(m), 0, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_lockstep(fn, None, 2, None, 0, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_lockstep(fn, None, 2, C.byref(m), 0, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_lockstep(fn, None, 0, C.byref(m), 0, C.byref(fit)) == _abi.VB2_ERR_INVALID
    h = C.c_void_p()
    b = np.array([0.5])
    assert L.vb2_refbias_create(None, 1, b.ctypes.data, C.byref(h)) == _abi.VB2_ERR_INVALID and not h
    assert L.vb2_refbias_create(None, 1, b.ctypes.data, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_eval(None, None, None, None, None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_optimize_llk(None, C.byref(m), None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_info_get(None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_refbias_fit_ctx(None, C.byref(m), C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_run_refbias(None, None, None) == _abi.VB2_ERR_INVALID
    L.vb2_refbias_destroy(None)
    # a fixed alpha leaves nothing to estimate: refused before the evaluator is called
    ev = rr.Evaluator(None)
    with pytest.raises(_abi.Vb2Error, match="fixed alpha") as ei:
        vb.refbias_with_evaluator(ev, 2, fix_alpha=0.01)
    assert ei.value.code == _abi.VB2_ERR_INVALID and not ev.calls
    # an evaluator's failure ends the fit and comes back
    ev = rr.Evaluator(Counts(vb.synth.make_pileup(50, mean_depth=10, num_pc=2, seed=3)), fail_at=3)
    with pytest.raises(RuntimeError, match="on purpose"):
        vb.refbias_with_evaluator(ev, 2)
    assert len(ev.calls) == 3
    seen = []

    def failing(user, rows, npt, beta, p1, p2, a, out):
        seen.append(rows)
        return -77
    assert L.vb2_refbias_lockstep(_abi.REFBIAS_EVAL_FN(failing), None, 2, C.byref(m), 0, C.byref(fit)) == -77
    assert seen == [9]
    # a sample that counts no marker: the search's status goes into the fit
    rc = L.vb2_refbias_lockstep(_abi.REFBIAS_EVAL_FN(lambda u, rows, npt, beta, p1, p2, a, out: 0), None, 2, C.byref(m), 0,
                                C.byref(fit))
    assert rc == _abi.VB2_ERR_INVALID and fit.status == _abi.VB2_ERR_INVALID and fit.num_pair == 0


def test_beta_outside_the_domain_is_refused_by_the_set():
    """vb2_refbias_create checks its rows before it looks at the context's device."""
    if _abi.lib().vb2_device_count() > 0:
        d = vb.synth.make_pileup(50, mean_depth=10, num_pc=2, seed=3)
        with vb.LikelihoodContext(d) as ctx:
            for bad in (0.2499, 0.7501, float("nan")):
                with pytest.raises(_abi.Vb2Error, match="outside"):
                    vb.RefBias(ctx, [0.5, bad])
    import ctypes as C

    class Ctx(C.Structure):                        # a handle whose context is never reached: the rows are checked first
        _fields_ = [("impl", C.c_void_p)]
    fake = Ctx(1)
    h = C.c_void_p()
    for bad in (0.2499, 0.7501, float("nan")):
        b = np.array([0.5, bad])
        rc = _abi.lib().vb2_refbias_create(C.byref(fake), 2, b.ctypes.data, C.byref(h))
        assert rc == _abi.VB2_ERR_INVALID and b"outside [0.25, 0.75]" in _abi.lib().vb2_last_error() and not h
    assert rr.BETA_MIN == _abi.VB2_REFBIAS_MIN and rr.BETA_MAX == _abi.VB2_REFBIAS_MAX


REFUSALS = {
    "pileup_list": (["--PileupList", "absent.list"], "--PileupList"),
    "per_read_group": (["--BamFile", "absent.bam", "--PerReadGroup"], "--PerReadGroup"),
    "fix_alpha": (["--PileupFile", "absent.pileup", "--FixAlpha", "0.01"], "--FixAlpha"),
    "confidence_interval": (["--PileupFile", "absent.pileup", "--ConfidenceInterval"], "--ConfidenceInterval"),
    "per_chromosome": (["--PileupFile", "absent.pileup", "--PerChromosome"], "--PerChromosome"),
    "bootstrap": (["--PileupFile", "absent.pileup", "--Bootstrap", "5"], "--Bootstrap"),
    "two_devices": (["--PileupFile", "absent.pileup", "--Devices", "0,1"], "more than one --Devices"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_command_line_refuses_before_any_file_is_read(case, tmp_path):
    extra, reason = REFUSALS[case]
    p = subprocess.run([EXE, "--SVDPrefix", str(tmp_path / "absent_panel"), "--Reference", "unread.fa", "--RefBias",
                        "--Output", str(tmp_path / "o")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "FATAL ERROR" in p.stderr
    assert "--RefBias cannot be combined with" in p.stderr and reason in p.stderr, p.stderr
    assert "absent_panel" not in p.stderr and "absent.pileup" not in p.stderr and "absent.bam" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.RefBias"))


def test_the_library_refuses_the_same_before_any_file_is_read(tmp_path):
    for kw, reason in ((dict(devices=[0, 1]), "one device"), (dict(fix_alpha=0.01), "--FixAlpha")):
        with pytest.raises(_abi.Vb2Error) as ei:
            vb.run_files(str(tmp_path / "absent_panel"), str(tmp_path / "absent.pileup"), None, ref_bias=True, **kw)
        msg = _abi.lib().vb2_last_error().decode()
        assert ei.value.code == _abi.VB2_ERR_INVALID and "--RefBias" in msg and reason in msg and "absent" not in msg
    with pytest.raises(ValueError):
        vb.run_files(str(tmp_path / "absent_panel"), str(tmp_path / "absent.pileup"), None, ref_bias=True, confidence_interval=True)
