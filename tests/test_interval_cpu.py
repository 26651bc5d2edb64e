"""--ConfidenceInterval without a GPU: the new struct's layout against its ctypes mirror, and the command line's refusals
of what the interval does not serve (cohorts, marker shards) before any file is read or any device call is made."""
import ctypes as C
import os
import subprocess

from verifybamid_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")


def test_interval_struct_layout_matches_the_binding(tmp_path):
    fields = [f for f, _ in _abi.Interval._fields_]
    src = tmp_path / "ci_check.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vb2_abi.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vb2_interval));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(vb2_interval, %s));\n' % (f, f) for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "ci_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_abi.Interval)
    for f in fields:
        assert int(got[f]) == getattr(_abi.Interval, f).offset, f
    for name in ("vb2_ctx_interval", "vb2_run_interval"):
        assert name in _abi.SYMBOLS and hasattr(_abi.lib(), name)


def _refused(tmp_path, extra):
    # no panel, pileup or list file exists: a refusal that came after reading one would name the missing file
    cmd = [EXE, "--ConfidenceInterval", "--SVDPrefix", str(tmp_path / "nopanel"), "--Reference", "x.fa",
           "--Output", str(tmp_path / "o")] + extra
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode != 0
    assert "FATAL ERROR" in p.stderr
    assert not (tmp_path / "o.CI").exists()
    return p.stderr


def test_cli_refuses_a_pileup_list(tmp_path):
    err = _refused(tmp_path, ["--PileupList", str(tmp_path / "list.txt")])
    assert "--ConfidenceInterval cannot be combined with --PileupList" in err
    assert "cannot open --PileupList" not in err


def test_cli_refuses_several_devices(tmp_path):
    err = _refused(tmp_path, ["--PileupFile", str(tmp_path / "s.pileup"), "--Devices", "0,1"])
    assert "--ConfidenceInterval cannot be combined with more than one --Devices" in err
    assert "NOTICE - Starting phase" not in err


# ---- the numpy restatement of the interval (tests/interval_ref.py) against the oracle ----

def _ref_modules():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import deriv_ref
    import interval_ref
    return deriv_ref, interval_ref


def test_se_ref_against_finite_differences_of_the_oracles_llk():
    """se_ref's A = -J' H J with alpha as logit (within ancestry: the shared PC is the sum of both blocks) against central
    second differences of the oracle's LLK in those very coordinates (u, x = logit alpha), Richardson-extrapolated.
    Steps of 0.05 standard deviations of each coordinate: the LLK (3e4) rounds to 4e-12, so a second difference carries
    4 x 4e-12 / 0.05^2 = 6e-9 of sqrt(A_ii A_jj), and the extrapolated truncation error is of order 0.05^4; 1e-4 of
    sqrt(A_ii A_jj) per entry is asked."""
    import numpy as np
    import verifybamid_amd as vb
    from oracle.bridge import oracle_data
    deriv_ref, interval_ref = _ref_modules()
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.2, seed=21)
    od = oracle_data(d)
    est = od.optimize(within_ancestry=True)
    ref = interval_ref.se_ref(d, est, within_ancestry=True)
    assert ref["pos_def"] and ref["num_free"] == 3 and not ref["swapped"]
    x0 = np.array([est["pc"][0], est["pc"][1], np.log(est["alpha"] / (1 - est["alpha"]))])

    def f(x):
        return od.llk(x[:2], x[:2], 1.0 / (1.0 + np.exp(-x[2])))
    h = 0.05 * ref["se"]

    def second(i, j, s):
        ei, ej = np.zeros(3), np.zeros(3)
        ei[i], ej[j] = s * h[i], s * h[j]
        return (f(x0 + ei + ej) - f(x0 + ei - ej) - f(x0 - ei + ej) + f(x0 - ei - ej)) / (4 * s * s * h[i] * h[j])
    A = np.array([[-(4 * second(i, j, 1.0) - second(i, j, 2.0)) / 3 for j in range(3)] for i in range(3)])
    se_fd = np.sqrt(np.diag(np.linalg.inv(A)))
    # entry by entry, in units of sqrt(A_ii A_jj) (1 / (se_i se_j) up to the correlations)
    scale = 1.0 / np.outer(ref["se"], ref["se"])
    assert np.max(np.abs(A - ref["A"]) / scale) <= 1e-4, (A, ref["A"])
    assert np.max(np.abs(se_fd / ref["se"] - 1)) <= 1e-4 * ref["cond"], (se_fd, ref["se"])
    s = est["alpha"] * (1 - est["alpha"])
    assert ref["freemix_se"] == s * ref["se"][2]
    assert [r[0] for r in ref["rows"]] == ["FREEMIX", "PC1", "PC2"]


def test_profile_ref_against_the_oracles_fixed_alpha_search():
    import verifybamid_amd as vb
    from oracle.bridge import oracle_data
    deriv_ref, interval_ref = _ref_modules()
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.2, seed=21)
    od = oracle_data(d)
    c = deriv_ref.Counts(d)
    for kw in ({}, dict(within_ancestry=True)):
        est = od.optimize(**kw)
        llk = abs(est["llk1"])
        # Newton from the search's end point does not lose likelihood
        assert interval_ref.profile_ref(d, est, est["alpha"], counts=c, **kw) >= -est["llk1"] - 1e-9 * llk
        for f in (0.8 * est["alpha"], 1.2 * est["alpha"]):
            v = interval_ref.profile_ref(d, est, f, counts=c, **kw)
            o = -od.optimize(fix_alpha=f, **kw)["llk1"]
            assert o <= v + 1e-9 * llk and o >= v - 1e-6 * llk, (kw, f, v, o)
    # no free PC: the profile is the LLK itself
    est = od.optimize(within_ancestry=True, fix_pc=[0.01, 0.02])
    v = interval_ref.profile_ref(d, est, 0.1, counts=c, within_ancestry=True, fix_pc=[0.01, 0.02])
    want = od.llk([0.01, 0.02], [0.01, 0.02], 0.1)
    assert abs(v - want) <= 1e-11 * abs(want)


def test_se_ref_undoes_the_swap_of_indices_0_and_1():
    """alpha >= 0.5 in a heterogeneous model: the likelihood is taken at the PCs with indices 0 and 1 swapped back, and
    each SE is reported at the row that holds its coordinate's value -- the twin of an estimate has the SEs of the
    estimate itself, row for row by value."""
    import numpy as np
    import verifybamid_amd as vb
    from oracle.bridge import oracle_data
    deriv_ref, interval_ref = _ref_modules()
    k = 4
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=k, alpha_true=0.2, seed=33)
    est = oracle_data(d).optimize()
    assert est["alpha"] < 0.5
    twin = dict(est, alpha=1 - est["alpha"],
                pc=np.concatenate([est["pc"][:2], est["pc2"][2:k]]), pc2=np.concatenate([est["pc2"][:2], est["pc"][2:k]]))
    p1, p2, swapped = interval_ref.search_point(d, twin)
    assert swapped and np.array_equal(p1, est["pc2"][:k]) and np.array_equal(p2, est["pc"][:k])
    a, b = interval_ref.se_ref(d, est), interval_ref.se_ref(d, twin)
    assert a["pos_def"] and b["pos_def"]
    by_value = {v: se for _, v, se in a["rows"][1:]}
    assert [n for n, _, _ in b["rows"]] == [n for n, _, _ in a["rows"]]
    for name, v, se in b["rows"][1:]:
        assert abs(se - by_value[v]) <= 1e-9 * se, (name, se, by_value[v])
    assert abs(a["freemix_se"] - b["freemix_se"]) <= 1e-9 * a["freemix_se"]
    # --FixPC: the fixed values show as ContaminatingSample.PC1/2 without an SE, the free ones as IntendedSample.PC1/2
    fx = dict(est, alpha=0.8, pc=np.array([0.01, 0.02, est["pc"][2], est["pc"][3]]),
              pc2=np.array([est["pc"][0], est["pc"][1], 0.0, 0.0]))
    r = interval_ref.se_ref(d, fx, fix_pc=[0.01, 0.02, 0.0, 0.0])
    assert [n for n, _, _ in r["rows"]] == ["FREEMIX"] + ["ContaminatingSample.PC%d" % j for j in (1, 2, 3, 4)] + \
        ["IntendedSample.PC1", "IntendedSample.PC2"]
    assert np.isnan(r["rows"][1][2]) and np.isnan(r["rows"][2][2]) and r["rows"][1][1] == 0.01
    assert r["rows"][5][1] == est["pc"][0] and r["num_free"] == k + 1
