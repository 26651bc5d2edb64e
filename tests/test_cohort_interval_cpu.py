"""--CohortInterval without a GPU: the lock-step interval driver (vb2_intervals_lockstep) over the numpy restatement of the
derivatives (tests/deriv_ref.py, float64) -- a gang of three against three gangs of one, the numbers against
tests/interval_ref.py, and how the evaluator is called --, the command line's refusals before any file is read, and the
additions to the ABI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402
import interval_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
C_HALF = 1.9207294103470620
NEW_SYMBOLS = ["vb2_batch_derivs", "vb2_batch_interval", "vb2_intervals_lockstep", "vb2_cohort_run_intervals"]


def _same(a, b):
    """Two interval dicts hold the same bits (NaN = NaN)."""
    assert a.keys() == b.keys()
    for key in a:
        if key == "rows":
            assert len(a["rows"]) == len(b["rows"])
            for ra, rb in zip(a["rows"], b["rows"]):
                assert ra["param"] == rb["param"] and ra["method"] == rb["method"]
                for f in ("estimate", "stderr", "lo", "hi"):
                    assert np.float64(ra[f]).tobytes() == np.float64(rb[f]).tobytes(), (ra, rb)
        elif isinstance(a[key], float):
            assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), (key, a[key], b[key])
        else:
            assert a[key] == b[key], (key, a[key], b[key])


@pytest.fixture(scope="module")
def gang():
    """Three samples of 300 markers x 10 reads, their estimates from the restatement's own optimum, and the evaluator."""
    k = 2
    samples = []
    for alpha_true, seed in ((0.05, 3), (0.1, 4), (0.2, 5)):
        d = vb.synth.make_pileup(300, mean_depth=10, num_pc=k, alpha_true=alpha_true, seed=seed)
        c = deriv_ref.Counts(d)
        est = interval_ref.optimum_ref(d, np.zeros(k), np.zeros(k), alpha_true, counts=c)
        samples.append((d, c, est))
    calls = []

    def make_eval(which):
        """The evaluator of a gang made of samples `which`; every call is recorded as (which, num_point)."""
        def evaluate(num_point, pc1, pc2, alpha):
            calls.append((tuple(which), tuple(int(x) for x in num_point)))
            n = 2 * k + 1
            P = int(num_point.sum())
            llk, grad, hess = np.zeros(P), np.zeros((P, n)), np.zeros((P, n, n))
            o = 0
            for slot, s in enumerate(which):
                for _ in range(int(num_point[slot])):
                    f, g, h = deriv_ref.derivs(samples[s][1], pc1[o], pc2[o], alpha[o])
                    llk[o], grad[o], hess[o] = float(f), np.asarray(g, dtype=np.float64), np.asarray(h, dtype=np.float64)
                    o += 1
            return llk, grad, hess
        return evaluate
    return k, samples, calls, make_eval


def test_a_gang_of_three_is_three_gangs_of_one(gang):
    k, samples, calls, make_eval = gang
    ests = [s[2] for s in samples]
    del calls[:]
    together, steps = vb.intervals_with_evaluator(make_eval([0, 1, 2]), k, ests)
    shared = list(calls)
    assert all(ci["status"] == 0 for ci in together)
    # the evaluator is called max(num_launch) times, and each call carries every live sample's request: sample s asks
    # for one point in each of its first num_launch[s] steps and for none afterwards
    launches = [ci["num_launch"] for ci in together]
    assert steps == len(shared) == max(launches) and sum(launches) > max(launches)
    for step, (_, num_point) in enumerate(shared):
        assert num_point == tuple(1 if step < n else 0 for n in launches), (step, num_point, launches)
    for s in range(3):
        alone, steps1 = vb.intervals_with_evaluator(make_eval([s]), k, [ests[s]])
        assert steps1 == alone[0]["num_launch"]
        _same(together[s], alone[0])


def test_the_numbers_against_the_restatement(gang):
    k, samples, calls, make_eval = gang
    ests = [s[2] for s in samples]
    cis, _ = vb.intervals_with_evaluator(make_eval([0, 1, 2]), k, ests)
    for (d, c, est), ci in zip(samples, cis):
        ref = interval_ref.se_ref(d, est, counts=c)
        assert ci["pos_def"] == ref["pos_def"] and ci["num_free"] == ref["num_free"]
        assert [r["param"] for r in ci["rows"]] == [name for name, _, _ in ref["rows"]]
        rel = 1e-4 * ref["cond"]                      # (tests/test_interval_cpu.py: the restatement's SEs)
        for row, (name, value, se) in zip(ci["rows"], ref["rows"]):
            assert row["estimate"] == value
            if np.isnan(se):
                assert np.isnan(row["stderr"])
            else:
                assert abs(row["stderr"] / se - 1) <= rel, (name, row["stderr"], se)
        llk = abs(est["llk1"])
        assert 0.0 <= ci["lo"] <= ci["freemix"] <= ci["hi"] <= 0.5
        for b, v, edge in ((ci["lo"], ci["llk_lo"], 0.0), (ci["hi"], ci["llk_hi"], 0.5)):
            # the profile value at the bound against the restatement's Newton profile there (the tolerances of
            # test_profile_ref_against_the_oracles_fixed_alpha_search: neither climb beats the other by more)
            want = interval_ref.profile_ref(d, est, b, counts=c)
            assert want <= v + 1e-6 * llk and want >= v - 1e-6 * llk, (b, v, want)
            if b != edge:
                assert abs(v - (ci["llk_max"] - C_HALF)) <= 1e-7 * llk, (b, v, ci["llk_max"])
            else:
                assert v >= ci["llk_max"] - C_HALF


def test_an_evaluator_that_fails_ends_every_interval(gang):
    k, samples, calls, make_eval = gang
    inner = make_eval([0, 1])
    count = [0]

    def evaluate(num_point, pc1, pc2, alpha):
        count[0] += 1
        if count[0] == 3:
            raise RuntimeError("third step")
        return inner(num_point, pc1, pc2, alpha)
    with pytest.raises(RuntimeError, match="third step"):
        vb.intervals_with_evaluator(evaluate, k, [samples[0][2], samples[1][2]])
    assert count[0] == 3


def _refused(tmp_path, extra):
    # no panel, pileup or list file exists: a refusal that came after reading one would name the missing file
    cmd = [EXE, "--CohortInterval", "--SVDPrefix", str(tmp_path / "nopanel"), "--Reference", "x.fa",
           "--Output", str(tmp_path / "o")] + extra
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode != 0
    assert "FATAL ERROR" in p.stderr
    return p.stderr


def test_cli_refuses_cohort_interval_without_a_pileup_list(tmp_path):
    err = _refused(tmp_path, ["--PileupFile", str(tmp_path / "s.pileup")])
    assert "--CohortInterval needs --PileupList" in err
    assert "NOTICE - Starting phase" not in err


def test_cli_refuses_cohort_interval_on_several_devices(tmp_path):
    err = _refused(tmp_path, ["--PileupList", str(tmp_path / "list.txt"), "--Devices", "0,1"])
    assert "--CohortInterval cannot be combined with more than one --Devices" in err
    assert "cannot open --PileupList" not in err


def test_library_refuses_several_devices_before_any_file_is_read(tmp_path):
    devs = (C.c_int32 * 2)(0, 1)
    args, keep = vb.api._run_args(str(tmp_path / "nopanel"), str(tmp_path / "s.pileup"), 2, True, None, None, devices=[0, 1])
    ca = _abi.CohortArgs()
    ca.base = args
    ca.num_sample = 1
    piles = (C.c_char_p * 1)(str(tmp_path / "s.pileup").encode())
    ca.pileup_paths = piles
    res, status, ci = (_abi.RunResult * 1)(), (C.c_int32 * 1)(), (_abi.Interval * 1)()
    rc = _abi.lib().vb2_cohort_run_intervals(C.byref(ca), 0, res, status, ci)
    assert rc == _abi.VB2_ERR_INVALID
    assert b"one device" in _abi.lib().vb2_last_error()
    del devs, keep


def test_abi_additions(tmp_path):
    lib = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    assert lib.vb2_abi_version() == 7
    # the header still compiles as C99 with the additions, and the structs the new entry points take have the binding's sizes
    names = ["vb2_interval", "vb2_estimate", "vb2_model", "vb2_cohort_args", "vb2_run_result"]
    src = tmp_path / "abi_check.c"
    src.write_text('#include <stdio.h>\n#include "vb2_abi.h"\n'
                   "static int ev(void *u, int32_t s, const int32_t *n, const double *a, const double *b, const double *c,\n"
                   "              double *l, double *g, double *h)\n"
                   "{ (void)u; (void)s; (void)n; (void)a; (void)b; (void)c; (void)l; (void)g; (void)h; return 0; }\n"
                   "int main(void) {\n  vb2_batch_derivs_fn fn = ev;\n  (void)fn;\n" +
                   "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   "  return 0;\n}\n")
    exe = tmp_path / "abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for cname, ctype in zip(names, (_abi.Interval, _abi.Estimate, _abi.Model, _abi.CohortArgs, _abi.RunResult)):
        assert int(got[cname]) == C.sizeof(ctype), cname
