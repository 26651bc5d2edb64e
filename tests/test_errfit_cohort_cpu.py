"""The cohort form of the error-rate fit without a GPU: the additions to the
ABI, the argument errors, the numpy restatement of the pooled procedure (tests/errfit_cohort_ref.py) on its own, and the
library's statement of the procedure (vb2_errfit_cohort_lockstep) driven by the restatement's callbacks.

The samples are errfit_ref.sample's at 600 markers x 30 reads (k = 2, known allele frequencies, alpha = 0.03, qualities
20 / 30 / 37), one of the three calibrated, the others with the rates of q - 5 planted.

The pooled log-posterior -- the samples' log-likelihoods at their searched estimates plus the Beta prior's logarithm of the
table -- may not decrease from one iteration to the next beyond the searches' own stopping noise: tests/test_errfit_cpu.py's
monotone allowance, 1e-7 of its magnitude.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errfit_cohort_ref as ecr  # noqa: E402
import errfit_ref as er  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vb2_errstat_batch_create", "vb2_errstat_batch_destroy", "vb2_errstat_batch_eval", "vb2_errstat_batch_info_get",
               "vb2_errfit_cohort_inputs", "vb2_errfit_cohort_lockstep", "vb2_cohort_run_errfit",
               "vb2_err_table_read", "vb2_run_under_table", "vb2_cohort_run_under_table"]
SEEDS_SHIFTS = [(21, 5), (22, 0), (23, 5)]
MONOTONE = 1e-7                    # tests/test_errfit_cpu.py: "monotone within the searches' own stopping noise"
RECORD = ("iter_llk", "iter_change", "iter_alpha", "iter_err", "err", "n", "s")


def test_new_symbols_and_the_abi_is_still_7():
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.vb2_abi_version() == 7
    assert re.search(r"#define VB2_ABI_VERSION 7\b", header)
    for name in ("ErrStatBatch", "errfit_cohort", "errfit_cohort_with_evaluator"):
        assert hasattr(vb, name), name
    assert _abi.get_tunable("errstat_multi_groups") == 0
    # the structs as the header lays them out; vb2_errfit is untouched
    est = C.sizeof(_abi.Estimate)
    assert C.sizeof(_abi.ErrFit) == 3 * 8 * 94 + est + 4 * 8 + 3 * 8 * 24 + 4 * 24 * 94 + 8 + 4 * 4
    assert C.sizeof(_abi.ErrStatBatchInfo) == 4 * 4 + 5 * 8
    assert C.sizeof(_abi.ErrFitPool) == 3 * 8 * 94 + 8 * 24 + 4 * 24 * 94 + 4 * 8 + 2 * 8 + 8 * 4


def test_argument_errors():
    L = _abi.lib()
    d = vb.synth.make_pileup(50, mean_depth=10, num_pc=2, seed=3)
    inp = d.as_input()
    ptrs = (C.POINTER(_abi.Input) * 1)(C.pointer(inp))
    h = C.c_void_p()
    assert L.vb2_errstat_batch_create(ptrs, 1, None, None) == _abi.VB2_ERR_INVALID
    for bad in (0, 65, -1):
        assert L.vb2_errstat_batch_create(ptrs, bad, None, C.byref(h)) == _abi.VB2_ERR_INVALID and not h
        assert b"1..64 samples" in L.vb2_last_error()
    assert L.vb2_errstat_batch_create(None, 1, None, C.byref(h)) == _abi.VB2_ERR_INVALID and not h
    broken = d.as_input()
    broken.num_pc = 0
    assert L.vb2_errstat_batch_create((C.POINTER(_abi.Input) * 1)(C.pointer(broken)), 1, None, C.byref(h)) == _abi.VB2_ERR_INVALID
    assert b"vb2_errstat_batch_create: invalid input" in L.vb2_last_error()
    assert L.vb2_errstat_batch_eval(None, None, None, None, None, None, None, None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_errstat_batch_info_get(None, None) == _abi.VB2_ERR_INVALID
    L.vb2_errstat_batch_destroy(None)
    m, keep = vb.api._model()
    ests, fits, pool = (_abi.Estimate * 1)(), (_abi.ErrFit * 1)(), _abi.ErrFitPool()
    e, f = C.addressof(ests), C.addressof(fits)
    ok = (ptrs, 1, None, C.byref(m), e, None, None, 0, f, C.byref(pool))
    for i, bad in ((0, None), (1, 0), (1, 65), (3, None), (4, None), (8, None), (9, None)):
        args = list(ok)
        args[i] = bad
        assert L.vb2_errfit_cohort_inputs(*args) == _abi.VB2_ERR_INVALID, i
    fixed, keep2 = vb.api._model(fix_alpha=0.01)
    assert L.vb2_errfit_cohort_inputs(ptrs, 1, None, C.byref(fixed), e, None, None, 0, f, C.byref(pool)) == _abi.VB2_ERR_INVALID
    assert b"fixed alpha" in L.vb2_last_error()
    fns = _abi.ErrFitCohortFns(_abi.ERRFIT_COHORT_EVAL_FN(lambda *a: 0), _abi.ERRFIT_COHORT_STATS_FN(lambda *a: 0))
    ok = (C.byref(fns), None, 1, 2, C.byref(m), 0, e, None, None, 0, f, C.byref(pool))
    for i, bad in ((0, None), (0, C.byref(_abi.ErrFitCohortFns())), (2, 0), (2, 65), (3, 0), (4, None), (6, None), (10, None),
                   (11, None)):
        args = list(ok)
        args[i] = bad
        assert L.vb2_errfit_cohort_lockstep(*args) == _abi.VB2_ERR_INVALID, i
    assert L.vb2_errfit_cohort_lockstep(C.byref(fns), None, 1, 2, C.byref(fixed), 0, e, None, None, 1, f,
                                        C.byref(pool)) == _abi.VB2_ERR_INVALID
    assert b"fixed alpha" in L.vb2_last_error()
    # options as vb2_errfit_lockstep checks them, before any callback is called
    calls = []
    nom = dict(alpha=0.03, pc=[0, 0], pc2=[0, 0])
    for kw in (dict(prior_reads=-1.0), dict(tol=-1.0), dict(max_iter=25), dict(prior_reads=float("nan"))):
        with pytest.raises(_abi.Vb2Error, match="prior_reads and tol are positive"):
            vb.errfit_cohort_with_evaluator(lambda *a: calls.append(1), lambda *a: calls.append(2), 2, [nom], **kw)
    assert not calls
    # a statistics callback that fails ends the fit with its code
    bad_fns = _abi.ErrFitCohortFns(_abi.ERRFIT_COHORT_EVAL_FN(lambda *a: 0), _abi.ERRFIT_COHORT_STATS_FN(lambda *a: -77))
    assert L.vb2_errfit_cohort_lockstep(C.byref(bad_fns), None, 1, 2, C.byref(m), 0, e, None, None, 1, f, C.byref(pool)) == -77
    del keep, keep2


# ---- the pooled restatement, and the library's statement over its callbacks ----
@pytest.fixture(scope="module")
def cohort():
    datas = [er.sample(600, seed, shift=shift)[0] for seed, shift in SEEDS_SHIFTS]
    co = ecr.Cohort(datas)
    noms = co.nominal_estimates()
    return datas, co, noms, co.pooled_fit(noms)


def _same_record(got, want):
    assert got["status"] == want["status"] == 0 and got["num_iter"] == want["num_iter"] and got["converged"] == want["converged"]
    for key in RECORD:
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    for key in ("llk_fit", "llk_nominal", "alpha_nominal", "lrt", "alpha_fit", "num_bin", "num_step"):
        assert got[key] == want[key], key
    assert got["estimate"]["num_eval"] == want["estimate"]["num_eval"]


def test_pooling_one_sample_is_the_single_sample_fit():
    d = er.sample(600, 21)[0]
    ev = er.Evaluator(d)
    single, nom = ev.fit(2, True)
    fits, pool = ecr.Cohort([d]).pooled_fit([nom])
    _same_record(fits[0], single)
    assert np.array_equal(pool["n"], single["n"]) and np.array_equal(pool["s"], single["s"]) and pool["lrt_sum"] == single["lrt"]
    assert np.array_equal(pool["err"], single["err"]) and pool["iter_err"].tobytes() == single["iter_err"].tobytes()
    # ... and so is the library's statement, pooled or not
    co = ecr.Cohort([d])
    for pooled in (True, False):
        got, gpool = vb.errfit_cohort_with_evaluator(co.eval, co.stats, 2, [nom], pooled=pooled, known_af=True)
        _same_record(got[0], single)
        assert gpool["num_fitted"] == 1 and gpool["lrt_sum"] == single["lrt"] and np.array_equal(gpool["n"], single["n"])
        assert gpool["converged"] and gpool["num_estep"] == single["num_iter"] + 1


def test_the_pooled_log_posterior_does_not_decrease(cohort):
    datas, co, noms, (fits, pool) = cohort
    lp = pool["iter_logpost"]
    # the library's own record says the same: its samples' iter_llk summed, plus the prior of its iteration's table
    got, gpool = vb.errfit_cohort_with_evaluator(co.eval, co.stats, 2, noms, pooled=True, known_af=True)
    lib_lp = np.array([sum(f["iter_llk"][t] for f in got) + ecr.log_prior(gpool["iter_err"][t].astype(np.float64), 100.0)
                       for t in range(gpool["num_iter"])])
    assert np.all(np.diff(lib_lp) >= -MONOTONE * np.abs(lib_lp[1:])), np.diff(lib_lp)
    assert np.allclose(lib_lp, lp, rtol=1e-12, atol=0)
    print("pooled log-posterior per iteration:", lp, "changes", pool["iter_change"])
    assert pool["converged"] and 2 <= pool["num_iter"] <= 24
    assert np.all(np.diff(lp) >= -MONOTONE * np.abs(lp[1:])), np.diff(lp)
    # the rules: every table a float32 where the pool has reads, nominal elsewhere; the stop at the first change within tol
    has = pool["n"] > 0
    e0 = vb.nominal_err_table()
    assert sorted(np.nonzero(has)[0]) == list(er.SAMPLE_QUALS)
    assert np.array_equal(pool["err"][~has], e0[~has]) and np.array_equal(pool["n"], sum(f["n"] for f in fits))
    assert [c <= 1e-4 for c in pool["iter_change"]] == [False] * (pool["num_iter"] - 1) + [True]
    # the calibrated sample is pulled along by the two shifted ones: one table for all
    assert all(np.array_equal(f["err"], pool["err"]) for f in fits)


def test_the_lockstep_entry_returns_the_restatements_record(cohort):
    datas, co, noms, (want, wpool) = cohort
    got, gpool = vb.errfit_cohort_with_evaluator(co.eval, co.stats, 2, noms, pooled=True, known_af=True)
    for g, w in zip(got, want):
        _same_record(g, w)
    for key in ("n", "s", "err", "iter_change", "iter_err"):
        assert np.asarray(gpool[key]).tobytes() == np.asarray(wpool[key]).tobytes(), key
    for key in ("lrt_sum", "num_bin", "num_iter", "converged", "pooled", "num_sample", "num_entered", "num_fitted", "num_estep",
                "num_step"):
        assert gpool[key] == wpool[key], key


def test_per_sample_in_lockstep_is_every_sample_alone(cohort):
    datas, co, noms, _ = cohort
    got, gpool = vb.errfit_cohort_with_evaluator(co.eval, co.stats, 2, noms, pooled=False, known_af=True)
    alone = [co.ev[i].fit(2, True, nominal_est=noms[i])[0] for i in range(len(datas))]
    for g, w in zip(got, alone):
        _same_record(g, w)
    # the calibrated sample converges before the shifted ones: the lock-step thins out
    iters = [f["num_iter"] for f in got]
    assert gpool["num_iter"] == max(iters) and gpool["num_estep"] == max(iters) + 1 and not gpool["pooled"]
    assert gpool["lrt_sum"] == sum(f["lrt"] for f in got) and np.array_equal(gpool["err"], vb.nominal_err_table())


def test_a_sample_that_never_enters_and_one_that_fails_mid_fit(cohort):
    datas, co, noms, _ = cohort
    # sample 1 failed its own run: absent from the pool, the others are a pool without it
    sub = ecr.Cohort([datas[0], datas[2]])
    want, wpool = sub.pooled_fit([noms[0], noms[2]])
    got, gpool = vb.errfit_cohort_with_evaluator(co.eval, co.stats, 2, [noms[0], None, noms[2]], pooled=True, known_af=True,
                                                 enter_status=[0, _abi.VB2_ERR_INVALID, 0])
    _same_record(got[0], want[0])
    _same_record(got[2], want[1])
    assert got[1]["status"] == _abi.VB2_ERR_INVALID and got[1]["num_iter"] == 0 and not got[1]["n"].any()
    assert np.isnan(got[1]["lrt"]) and np.isnan(got[1]["llk_fit"])
    assert gpool["num_entered"] == gpool["num_fitted"] == 2 and np.array_equal(gpool["n"], wpool["n"])
    assert gpool["iter_err"].tobytes() == wpool["iter_err"].tobytes() and gpool["lrt_sum"] == wpool["lrt_sum"]
    # sample 2's search fails under the second table: it leaves with the code and is in no later sum; the others go on
    first = []

    def failing_eval(sample, err, pc1, pc2, alpha):
        if sample == 2:
            if not first:
                first.append(err.tobytes())
            if err.tobytes() != first[0]:
                raise vb.SearchFailed(_abi.VB2_ERR_SANITY)
        return co.eval(sample, err, pc1, pc2, alpha)

    class Failing(ecr.Cohort):
        def search(self, i, table, **kw):
            return vb.optimize_with_evaluator(lambda a, b, al: failing_eval(i, table, a, b, al), self.num_pc, known_af=True)
    want, wpool = Failing(datas).pooled_fit(noms)
    first.clear()
    got, gpool = vb.errfit_cohort_with_evaluator(failing_eval, co.stats, 2, noms, pooled=True, known_af=True)
    assert got[2]["status"] == want[2]["status"] == _abi.VB2_ERR_SANITY and got[2]["num_iter"] == want[2]["num_iter"] == 1
    assert not got[2]["n"].any() and np.isnan(got[2]["lrt"])
    _same_record(got[0], want[0])
    _same_record(got[1], want[1])
    assert gpool["num_entered"] == 3 and gpool["num_fitted"] == 2 and np.array_equal(gpool["n"], got[0]["n"] + got[1]["n"])
    assert gpool["iter_err"].tobytes() == wpool["iter_err"].tobytes() and gpool["lrt_sum"] == got[0]["lrt"] + got[1]["lrt"]
    # the second table still held sample 2's statistics; a pool that never had it goes another way from the start
    never, _ = ecr.Cohort(datas[:2]).pooled_fit(noms[:2])
    assert never[0]["iter_err"][0].tobytes() != got[0]["iter_err"][0].tobytes()


# ---- the command line's and the library's refusals, before any file is read ----
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
REFUSALS = {
    "fix_alpha": (["--FixAlpha", "0.01"], "--FixAlpha"),
    "num_start": (["--NumStart", "4"], "--NumStart"),
    "line_search": (["--KnownAF", "absent.af", "--LineSearch"], "--LineSearch"),
    "two_devices": (["--Devices", "0,1"], "more than one --Devices"),
    "find_source": (["--FindSource"], "--FindSource"),
    "find_related": (["--FindRelated"], "--FindRelated"),
    "matched_normal": (["--MatchedNormal", "absent.pairs"], "--MatchedNormal"),
    "cohort_interval": (["--CohortInterval"], "--CohortInterval"),
}


def _exe(tmp_path, extra):
    return subprocess.run([EXE, "--SVDPrefix", str(tmp_path / "absent_panel"), "--Reference", "unread.fa", "--Output",
                           str(tmp_path / "o")] + extra, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_command_line_refuses_before_any_file_is_read(case, tmp_path):
    extra, reason = REFUSALS[case]
    p = _exe(tmp_path, ["--PileupList", "absent.list", "--CohortFitError"] + extra)
    assert p.returncode != 0 and "FATAL ERROR" in p.stderr
    assert "--CohortFitError cannot be combined with " + reason in p.stderr, p.stderr
    line = [ln for ln in p.stderr.splitlines() if "--CohortFitError cannot be combined" in ln][0]
    others = {r for _, r in REFUSALS.values()} - {reason}
    assert not any(o in line for o in others), line              # each refusal has its own message
    assert "absent" not in p.stderr
    assert not os.path.exists(str(tmp_path / "o.PooledFit")) and not os.path.exists(str(tmp_path / "o.ErrorRates"))


def test_the_flags_need_each_other(tmp_path):
    p = _exe(tmp_path, ["--PileupFile", "absent.pileup", "--CohortFitError"])
    assert p.returncode != 0 and "--CohortFitError needs --PileupList" in p.stderr and "absent" not in p.stderr
    p = _exe(tmp_path, ["--PileupList", "absent.list", "--PooledError"])
    assert p.returncode != 0 and "--PooledError needs --CohortFitError" in p.stderr and "absent" not in p.stderr
    p = _exe(tmp_path, ["--PileupList", "absent.list", "--ErrorPrior", "50"])
    assert p.returncode != 0 and "--ErrorPrior needs --FitError" in p.stderr and "absent" not in p.stderr
    p = _exe(tmp_path, ["--PileupList", "absent.list", "--CohortFitError", "--ErrorPrior", "0"])
    assert p.returncode != 0 and "--ErrorPrior takes a positive number" in p.stderr and "absent" not in p.stderr
    # --FitError with a list stays refused with its own message
    p = _exe(tmp_path, ["--PileupList", "absent.list", "--FitError", "--CohortFitError"])
    assert p.returncode != 0 and "--FitError cannot be combined with --PileupList" in p.stderr


def test_the_library_refuses_the_same_before_any_file_is_read(tmp_path):
    absent = [str(tmp_path / "absent0.pileup"), str(tmp_path / "absent1.pileup")]
    for kw, reason in ((dict(devices=[0, 1]), "one device"), (dict(fix_alpha=0.01), "--FixAlpha"), (dict(num_start=4), "--NumStart"),
                       (dict(line_search=True), "--LineSearch"), (dict(error_prior=-1.0), "prior_reads")):
        with pytest.raises(_abi.Vb2Error) as ei:
            vb.run_cohort_files(str(tmp_path / "absent_panel"), absent, cohort_fit_error=True, **kw)
        msg = _abi.lib().vb2_last_error().decode()
        assert ei.value.code == _abi.VB2_ERR_INVALID and reason in msg and "absent" not in msg, msg
    with pytest.raises(_abi.Vb2Error, match="at most 64 samples"):
        vb.run_cohort_files(str(tmp_path / "absent_panel"), absent * 33, cohort_fit_error=True, pooled_error=True)
    assert "absent" not in _abi.lib().vb2_last_error().decode()
    for other in (dict(find_source=True), dict(find_related=True), dict(confidence_interval=True), dict(matched_normal=[(0, 1)])):
        with pytest.raises(ValueError):
            vb.run_cohort_files(str(tmp_path / "absent_panel"), absent, cohort_fit_error=True, **other)
    with pytest.raises(ValueError):
        vb.run_cohort_files(str(tmp_path / "absent_panel"), absent, pooled_error=True)
    L = _abi.lib()
    assert L.vb2_cohort_run_errfit(None, None, 0, None, None, None, None) == _abi.VB2_ERR_INVALID


# ---- --ErrorTable: the reader, and the refusals ----
RATES_HEAD = "#Q_REPORTED\tREADS\tEXPECTED_ERRORS\tERROR_RATE\tQ_EMPIRICAL\tSE_BINOM\n"
GOOD_ROWS = "20\t100\t3.1\t0.031\t15.1\t0.01\n30\t200\t0.7\t0.0035\t24.6\t0.004\n37\t50\t0\t0\tinf\t0\n"
# name -> (text, what the message says, the line it names)
MALFORMED = {
    "empty": ("", "the file is empty", 1),
    "no_quality_column": ("READS\tERROR_RATE\n20\t0.03\n", "no column #Q_REPORTED", 1),
    "no_rate_column": ("#Q_REPORTED\tREADS\n20\t100\n", "no column ERROR_RATE", 1),
    "short_row": (RATES_HEAD + "20\t100\t3.1\t0.031\t15.1\t0.01\n30\t200\n", "2 fields", 3),
    "rate_above_one": (RATES_HEAD + "20\t100\t3.1\t1.0000001\t0\t0\n", "outside [0, 1]", 2),
    "rate_negative": (RATES_HEAD + GOOD_ROWS + "40\t1\t0\t-1e-9\t0\t0\n", "outside [0, 1]", 5),
    "rate_nan": (RATES_HEAD + "20\t100\t3.1\tnan\t0\t0\n", "NaN", 2),
    "rate_text": (RATES_HEAD + "20\t100\t3.1\t0.03x\t0\t0\n", "is no number", 2),
    "rate_missing": (RATES_HEAD + "20\t100\t3.1\t\t0\t0\n", "is no number", 2),
    "quality_94": (RATES_HEAD + "94\t100\t3.1\t0.03\t0\t0\n", "outside 0..93", 2),
    "quality_negative": (RATES_HEAD + "-1\t100\t3.1\t0.03\t0\t0\n", "outside 0..93", 2),
    "quality_fraction": (RATES_HEAD + "20.5\t100\t3.1\t0.03\t0\t0\n", "no whole number", 2),
    "quality_twice": (RATES_HEAD + GOOD_ROWS + "30\t1\t0\t0.5\t0\t0\n", "the quality 30 is listed twice", 5),
}


def _table_files(tmp_path):
    good = str(tmp_path / "good.ErrorRates")
    open(good, "w").write(RATES_HEAD + GOOD_ROWS)
    narrow = str(tmp_path / "narrow.txt")                # the two columns alone, in the other order, CRLF, a blank line
    open(narrow, "w").write("ERROR_RATE\t#Q_REPORTED\r\n1\t0\r\n\r\n0.25\t93\r\n")
    bad = {}
    for name, (text, _, _) in MALFORMED.items():
        bad[name] = str(tmp_path / (name + ".txt"))
        open(bad[name], "w").write(text)
    return good, narrow, bad


def test_the_table_reader(tmp_path):
    good, narrow, bad = _table_files(tmp_path)
    e0 = vb.nominal_err_table()
    t, taken = vb.read_err_table(good)
    assert taken == 3 and t[20] == 0.031 and t[30] == 0.0035 and t[37] == 0.0
    rest = np.ones(94, dtype=bool)
    rest[[20, 30, 37]] = False
    assert np.array_equal(t[rest], e0[rest])
    t, taken = vb.read_err_table(narrow)
    assert taken == 2 and t[0] == 1.0 and t[93] == 0.25 and np.array_equal(t[1:93], e0[1:93])
    for name, (_, what, line) in MALFORMED.items():
        with pytest.raises(_abi.Vb2Error) as ei:
            vb.read_err_table(bad[name])
        msg = str(ei.value)
        assert ei.value.code == _abi.VB2_ERR_INVALID and what in msg and "line %d:" % line in msg and bad[name] in msg, (name, msg)
    with pytest.raises(_abi.Vb2Error, match="cannot be opened"):
        vb.read_err_table(str(tmp_path / "absent.ErrorRates"))
    L = _abi.lib()
    assert L.vb2_err_table_read(None, None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_err_table_read(good.encode(), None, None) == _abi.VB2_ERR_INVALID
    # what vb2_run_errfit writes is what the reader takes: default ostream formatting, "inf" in the other columns
    e = np.array([0.0316228, 0.00316228, 1.0])
    rows = "".join("%d\t%d\t%g\t%g\t%g\t%g\n" % (q, 1000, 1000 * r, r, -10 * np.log10(r), np.sqrt(r * (1 - r) / 1000))
                   for q, r in zip((20, 30, 37), e))
    written = str(tmp_path / "written.ErrorRates")
    open(written, "w").write(RATES_HEAD + rows)
    t, taken = vb.read_err_table(written)
    assert taken == 3 and np.array_equal(t[[20, 30, 37]], e)


def test_the_table_reader_under_the_sanitizers(tmp_path):
    """tests/err_table_check_main.cpp + err_table.cpp built with -fsanitize=address,undefined and run directly, on the CPU,
    over the good files and every malformed one: a sanitizer report (they abort) fails the test."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "err_table_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "verifybamid_amd", "csrc"), os.path.join(ROOT, "tests", "err_table_check_main.cpp"),
           os.path.join(ROOT, "verifybamid_amd", "csrc", "err_table.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    good, narrow, bad = _table_files(tmp_path)
    long_line = str(tmp_path / "long.txt")               # a header of 10 000 columns and a row as wide
    open(long_line, "w").write("\t".join(["X"] * 9998 + ["#Q_REPORTED", "ERROR_RATE"]) + "\n" + "\t".join(["0"] * 9998 + ["5", "0.5"]) + "\n")
    args = [exe, "ok", good, "ok", narrow, "ok", long_line, "fail", str(tmp_path / "absent.txt")]
    for name in sorted(bad):
        args += ["fail", bad[name]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[0] == "ok 3 20:0.031 30:0.0035000000000000001 37:0" and lines[1] == "ok 2 93:0.25"       # (quality 0 at rate 1 is the nominal rate)
    assert lines[2] == "ok 1 5:0.5" and len(lines) == 4 + len(bad) and all(ln.startswith("error ") for ln in lines[3:])


TABLE_REFUSALS = {
    "fit_error": (["--PileupFile", "absent.pileup", "--FitError"], "--FitError"),
    "cohort_fit_error": (["--PileupList", "absent.list", "--CohortFitError"], "--CohortFitError"),
    "confidence_interval": (["--PileupFile", "absent.pileup", "--ConfidenceInterval"], "--ConfidenceInterval"),
    "cohort_interval": (["--PileupList", "absent.list", "--CohortInterval"], "--CohortInterval"),
    "find_source": (["--PileupList", "absent.list", "--FindSource"], "--FindSource"),
    "find_related": (["--PileupList", "absent.list", "--FindRelated"], "--FindRelated"),
    "matched_normal": (["--PileupList", "absent.list", "--MatchedNormal", "absent.pairs"], "--MatchedNormal"),
    "per_read_group": (["--BamFile", "absent.bam", "--PerReadGroup"], "--PerReadGroup"),
    "per_chromosome": (["--PileupFile", "absent.pileup", "--PerChromosome"], "--PerChromosome"),
    "bootstrap": (["--PileupFile", "absent.pileup", "--Bootstrap", "5"], "--Bootstrap"),
    "ref_bias": (["--PileupFile", "absent.pileup", "--RefBias"], "--RefBias"),
    "two_devices": (["--PileupFile", "absent.pileup", "--Devices", "0,1"], "more than one --Devices"),
}


@pytest.mark.parametrize("case", sorted(TABLE_REFUSALS))
def test_the_command_line_refuses_a_table_with_every_stage_before_any_file_is_read(case, tmp_path):
    extra, reason = TABLE_REFUSALS[case]
    p = _exe(tmp_path, ["--ErrorTable", "absent.ErrorRates"] + extra)
    assert p.returncode != 0 and "FATAL ERROR" in p.stderr
    assert "--ErrorTable cannot be combined with " + reason in p.stderr, p.stderr
    line = [ln for ln in p.stderr.splitlines() if "--ErrorTable cannot be combined" in ln][0]
    others = {r for _, r in TABLE_REFUSALS.values()} - {reason}
    assert not any(o in line for o in others), line              # each refusal has its own message
    assert "absent" not in p.stderr


def test_a_malformed_table_ends_the_run_before_the_panel_is_read(tmp_path):
    _, _, bad = _table_files(tmp_path)
    for extra in (["--PileupFile", "absent.pileup"], ["--PileupList", "absent.list"]):
        p = _exe(tmp_path, extra + ["--ErrorTable", bad["quality_twice"]])
        assert p.returncode != 0 and "line 5: the quality 30 is listed twice" in p.stderr and "absent" not in p.stderr
    p = _exe(tmp_path, ["--PileupFile", "absent.pileup", "--ErrorTable", str(tmp_path / "none.ErrorRates")])
    assert p.returncode != 0 and "cannot be opened" in p.stderr and "absent" not in p.stderr


def test_the_library_refuses_a_bad_table_before_any_file_is_read(tmp_path):
    panel, pile = str(tmp_path / "absent_panel"), str(tmp_path / "absent.pileup")
    t = vb.nominal_err_table()
    t[30] = 1.5
    for call in (lambda: vb.run_files(panel, pile, None, error_table=t), lambda: vb.run_cohort_files(panel, [pile, pile], error_table=t)):
        with pytest.raises(_abi.Vb2Error, match="quality 30") as ei:
            call()
        assert ei.value.code == _abi.VB2_ERR_INVALID and "absent" not in str(ei.value)
    with pytest.raises(_abi.Vb2Error, match="--ErrorTable takes one device") as ei:
        vb.run_files(panel, pile, None, error_table=vb.nominal_err_table(), devices=[0, 1])
    assert "absent" not in str(ei.value)
    for other in ("fit_error", "confidence_interval", "per_chromosome", "per_read_group", "ref_bias"):
        with pytest.raises(ValueError):
            vb.run_files(panel, pile, None, error_table=vb.nominal_err_table(), **{other: True})
    for other in (dict(cohort_fit_error=True), dict(find_source=True), dict(find_related=True), dict(confidence_interval=True),
                  dict(matched_normal=[(0, 1)])):
        with pytest.raises(ValueError):
            vb.run_cohort_files(panel, [pile, pile], error_table=vb.nominal_err_table(), **other)
    L = _abi.lib()
    assert L.vb2_run_under_table(None, None, None) == _abi.VB2_ERR_INVALID
    assert L.vb2_cohort_run_under_table(None, None, None, None) == _abi.VB2_ERR_INVALID


def test_pooling_brings_the_rates_nearer_at_low_depth():
    """8 samples of 3 000 x depth 10 with the rates of q - 5 planted (tools/errfit_cohort_time.py --stat, seed set 400 -- of
    the four sets of profiles/errfit_cohort/pooling_stat.txt the one where pooling gains least: the worst relative error of a
    rate 0.550 per sample, 0.151 pooled; the other sets 0.57 - 1.22 against 0.05 - 0.12).  Asserted is what every set shows:
    the pooled table's worst rate lies nearer the planted one than the worst per-sample rate does.  FREEMIX improves alike
    either way, so nothing is asserted between the two there, only that both beat the nominal estimate on average."""
    qs = list(er.SAMPLE_QUALS)
    made = [er.sample(3000, 400 + i, depth=10, shift=5) for i in range(8)]
    datas, planted = [m[0] for m in made], made[0][1]
    co = ecr.Cohort(datas)
    noms = co.nominal_estimates()
    pfits, pool = co.pooled_fit(noms)
    own = [co.ev[i].fit(2, True, nominal_est=noms[i])[0] for i in range(8)]
    rel_own = max(float(np.max(np.abs(f["err"][qs] - planted[qs]) / planted[qs])) for f in own)
    rel_pool = float(np.max(np.abs(pool["err"][qs] - planted[qs]) / planted[qs]))
    dist = lambda alphas: float(np.mean([abs(min(a, 1 - a) - 0.03) for a in alphas]))
    d_nom, d_own, d_pool = dist([n["alpha"] for n in noms]), dist([f["alpha_fit"] for f in own]), dist([f["alpha_fit"] for f in pfits])
    print("worst relative error of a rate: per sample %.3f, pooled %.3f; mean |FREEMIX - 0.03| nominal %.5f, per sample %.5f, "
          "pooled %.5f" % (rel_own, rel_pool, d_nom, d_own, d_pool))
    assert pool["converged"] and rel_pool < rel_own
    assert d_own < d_nom and d_pool < d_nom
