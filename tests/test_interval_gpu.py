"""The FREEMIX confidence interval (vb2_ctx_interval, vb2_run_interval, --ConfidenceInterval) on the MI355X: the
profile's defining properties, the oracle's own FixAlpha search at the bounds, calibration over seeds, and the command
line end to end (stdout, .selfSM and .Ancestry untouched; .CI rows of the model's free parameters).

The interval's numbers against a numpy restatement that shares no code with csrc/interval.cpp (tests/interval_ref.py):
every standard error and Wald bound in every model, the estimate's mirror image at alpha >= 0.5 (the reference's swap of
PC indices 0 and 1 undone and redone), the profile bounds against a plain Newton profile, the NA path of a Hessian that
is not negative definite, and every number of the .CI file against the struct."""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402
import interval_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
C_HALF = 1.9207294103470620


@pytest.mark.parametrize("alpha_true", [0.03, 0.8])
def test_profile_interval_properties(alpha_true):
    """(alpha_true 0.8 does NOT reach the alpha >= 0.5 branch: the search starts on the low side and ends at the mirror
    optimum, alpha = 0.1975.  test_mirrored_estimate does.)"""
    _profile_properties(vb.synth.make_pileup(10000, mean_depth=30, num_pc=4, alpha_true=alpha_true, seed=21), {}, 1 + 2 * 4)


@pytest.mark.parametrize("alpha_true", [0.03, 0.2])
def test_profile_interval_properties_within_ancestry(alpha_true):
    _profile_properties(vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=alpha_true, seed=21),
                        dict(within_ancestry=True), 1 + 2)


def _profile_properties(d, kw, num_row):
    od = oracle_data(d)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize(**kw)
        ci = ctx.interval(est, **kw)
    llk = abs(est["llk1"])
    f = ci["freemix"]
    assert f == (est["alpha"] if est["alpha"] < 0.5 else 1 - est["alpha"])
    assert ci["lo"] <= f <= ci["hi"]
    assert ci["llk_max"] >= -est["llk1"]
    side = est["alpha"] >= 0.5
    interior = [(b, v) for b, v, edge in ((ci["lo"], ci["llk_lo"], 0.0), (ci["hi"], ci["llk_hi"], 0.5)) if b != edge]
    assert interior
    for b, v in interior:
        assert abs(v - (ci["llk_max"] - C_HALF)) <= 1e-7 * llk, (b, v, ci["llk_max"])
        # the oracle's own search over the PCs at the bound's alpha cannot beat the profile, and comes close to it
        ref = od.optimize(fix_alpha=(1 - b) if side else b, **kw)
        assert -ref["llk1"] <= v + 1e-9 * llk, (b, -ref["llk1"], v)
        assert -ref["llk1"] >= v - 1e-6 * llk, (b, -ref["llk1"], v)
    assert ci["num_launch"] > 0 and ci["num_profile"] >= 3
    assert ci["rows"][0]["param"] == "FREEMIX" and len(ci["rows"]) == num_row


def test_calibration_over_seeds():
    """alpha_true 0.02: the interval covers it in >= 33 of 40 samples (nominal 38).  alpha_true 0: lo == 0 where the profile
    at 0 is within the cut.  At that boundary the likelihood ratio is not the half-and-half chi2 mixture that would give lo > 0
    in 1 of 40: the contaminant's PCs are not identified at alpha = 0 and the ratio maximises over them, which makes it
    heavier.  Measured on these seeds: lo == 0 in 35 of 40, the bound below."""
    covered = zero_lo = 0
    for s in range(1, 41):
        for alpha_true in (0.02, 0.0):
            d = vb.synth.make_pileup(10000, mean_depth=20, num_pc=2, alpha_true=alpha_true, seed=s)
            with vb.LikelihoodContext(d) as ctx:
                ci = ctx.interval(ctx.optimize())
            if alpha_true > 0:
                covered += ci["lo"] <= alpha_true <= ci["hi"]
            else:
                zero_lo += ci["lo"] == 0.0
    assert covered >= 33, covered
    assert zero_lo >= 35, zero_lo


def _run(args, out, ci):
    cmd = [EXE] + args + ["--Output", out] + (["--ConfidenceInterval"] if ci else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


MODELS = [("default", [], ["ContaminatingSample.PC1", "ContaminatingSample.PC2", "IntendedSample.PC1", "IntendedSample.PC2"]),
          ("within", ["--WithinAncestry"], ["PC1", "PC2"]),
          ("fixpc", ["--FixPC", "0.01:0.02"], ["ContaminatingSample.PC1", "ContaminatingSample.PC2"]),
          ("fixalpha", ["--FixAlpha", "0.05"], ["ContaminatingSample.PC1", "ContaminatingSample.PC2",
                                                  "IntendedSample.PC1", "IntendedSample.PC2"]),
          ("knownaf", None, [])]


def _cases(golden_dir, tmp_path):
    hap = os.path.join(golden_dir, "hapmap", "hapmap_3.3.b37.dat")
    yield "golden", ["--DisableSanityCheck", "--PileupFile", os.path.join(golden_dir, "expected", "result.Pileup"),
                     "--SVDPrefix", hap, "--Reference", "x.fa", "--NumPC", "2"]
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.04, seed=31)
    pre = str(tmp_path / "syn")
    vb.synth.write_files(d, pre)
    yield "synthetic", ["--DisableSanityCheck", "--PileupFile", pre + ".pileup", "--SVDPrefix", pre, "--Reference",
                        "x.fa", "--NumPC", "2"]


@pytest.mark.parametrize("name,extra,pc_rows", MODELS, ids=[m[0] for m in MODELS])
def test_cli_end_to_end(golden_dir, tmp_path, name, extra, pc_rows):
    for case, base in _cases(golden_dir, tmp_path):
        args = list(base)
        if extra is None:                                  # --KnownAF: the allele frequencies from the panel's means
            kaf = str(tmp_path / (case + ".kaf"))
            vb.synth.write_known_af(args[args.index("--SVDPrefix") + 1], kaf, seed=3)
            args += ["--KnownAF", kaf]
        else:
            args += extra
        a = _run(args, str(tmp_path / (case + name + ".a")), False)
        b = _run(args, str(tmp_path / (case + name + ".b")), True)
        assert a.stdout == b.stdout
        for ext in (".selfSM", ".Ancestry"):
            assert open(str(tmp_path / (case + name + ".a")) + ext).read() == \
                open(str(tmp_path / (case + name + ".b")) + ext).read()
        assert not os.path.exists(str(tmp_path / (case + name + ".a")) + ".CI")
        assert "NOTICE - FREEMIX 95% CI (profile likelihood): [" in b.stderr
        lines = open(str(tmp_path / (case + name + ".b")) + ".CI").read().splitlines()
        assert lines[0] == "#PARAM\tESTIMATE\tSTDERR\tCI_LOW\tCI_HIGH\tMETHOD"
        rows = [ln.split("\t") for ln in lines[1:]]
        assert [r[0] for r in rows] == ["FREEMIX"] + pc_rows
        assert rows[0][5] == ("fixed" if name == "fixalpha" else "profile")
        assert all(r[5] == "wald" for r in rows[1:])
        sm = open(str(tmp_path / (case + name + ".b")) + ".selfSM").read().splitlines()
        assert rows[0][1] == sm[1].split("\t")[6]           # FREEMIX as .selfSM prints it


# ---- the interval's numbers against tests/interval_ref.py ----

Z = 1.959963984540054
API_MODELS = [("default", {}, False), ("within", dict(within_ancestry=True), False),
              ("fixpc", dict(fix_pc=[0.01, 0.02]), False), ("fixalpha", dict(fix_alpha=0.05), False),
              ("within_fixpc", dict(within_ancestry=True, fix_pc=[0.01, 0.02]), False), ("knownaf", {}, True)]


def _sample(alpha_true, known_af=False, k=2, seed=31, M=3000):
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=k, alpha_true=alpha_true, seed=seed)
    if known_af:
        d.known_af = np.clip(d.means / 2.0, 0.01, 0.99)
    return d


def _largest_block_tolerance(d, est, kw):
    """The largest tol(block) of the derivative kernels' check (tests/test_derivs_gpu.py) at the estimate: what the
    kernels' Hessian may differ from the restatement's by, in units no smaller than the entries themselves."""
    pc1, pc2, _ = interval_ref.search_point(d, est, **kw)
    ref = deriv_ref.reference(deriv_ref.Counts(d), deriv_ref.Counts(d, np.longdouble), pc1, pc2, est["alpha"])
    return max(t for _, _, t in deriv_ref.block_devs(ref, ref["g64"], ref["h64"]).values())


def _close(x, want, rel):
    if np.isnan(want):
        return bool(np.isnan(x))
    return bool(abs(x - want) <= rel * abs(want))


def _check_rows(ci, ref, rel):
    """Row names, order and estimates exactly; every SE, FREEMIX's SE and the Wald bounds to `rel`."""
    assert [r["param"] for r in ci["rows"]] == [name for name, _, _ in ref["rows"]]
    assert ci["pos_def"] == ref["pos_def"] and ci["num_free"] == ref["num_free"]
    assert _close(ci["freemix_se"], ref["freemix_se"], rel), (ci["freemix_se"], ref["freemix_se"], rel)
    for row, (name, value, se) in zip(ci["rows"], ref["rows"]):
        assert row["estimate"] == value, (name, row, value)
        assert _close(row["stderr"], se, rel), (name, row["stderr"], se, rel)
        if name == "FREEMIX":
            assert row["stderr"] == ci["freemix_se"] or (np.isnan(row["stderr"]) and np.isnan(ci["freemix_se"]))
            for got, want in ((row["lo"], ci["lo"]), (row["hi"], ci["hi"])):
                assert got == want or (np.isnan(got) and np.isnan(want))
        elif np.isnan(se):
            assert np.isnan(row["lo"]) and np.isnan(row["hi"]), row
        else:
            assert abs(row["lo"] - (value - Z * se)) <= rel * Z * se, (name, row, se)
            assert abs(row["hi"] - (value + Z * se)) <= rel * Z * se, (name, row, se)


@pytest.mark.parametrize("alpha_true", [0.03, 0.2])
@pytest.mark.parametrize("name,kw,kaf", API_MODELS, ids=[m[0] for m in API_MODELS])
def test_standard_errors_in_every_model(name, kw, kaf, alpha_true):
    """Every row's SE, FREEMIX's SE and the Wald bounds against se_ref.  The kernels' Hessian agrees with the
    restatement's to the per-block tolerance of the derivative tests and the inversion amplifies that by cond(A):
    relative error cond(A) x (the largest tol(block) at the estimate) x 10 is accepted."""
    d = _sample(alpha_true, kaf)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize(**kw)
        ci = ctx.interval(est, **kw)
    ref = interval_ref.se_ref(d, est, **kw)
    assert ref["pos_def"], ref["eig"]
    rel = ref["cond"] * _largest_block_tolerance(d, est, kw) * 10
    print("%s alpha_true %g: cond(A) %.3g, accepted relative error %.3g" % (name, alpha_true, ref["cond"], rel))
    assert rel < 1e-4                                        # the bound itself has not gone soft
    _check_rows(ci, ref, rel)
    expect_rows = {"default": 5, "within": 3, "fixpc": 3, "fixalpha": 5, "within_fixpc": 1, "knownaf": 1}[name]
    assert len(ci["rows"]) == expect_rows
    assert ci["alpha_free"] == (name != "fixalpha")


def _twin(est, k, heter):
    """The same point seen from the other side: alpha' = 1 - alpha with the two samples' PCs exchanged, reported as the
    reference reports an alpha >= 0.5 (indices 0 and 1 swapped back).  Within ancestry there is one PC and no swap."""
    t = dict(est, alpha=1 - est["alpha"])
    if heter:
        pc, pc2 = np.array(est["pc2"], dtype=np.float64), np.array(est["pc"], dtype=np.float64)   # the search's point
        for j in range(min(k, 2)):
            pc[j], pc2[j] = pc2[j], pc[j]
        t["pc"], t["pc2"] = pc, pc2
    return t


@pytest.mark.parametrize("name,k,kw", [("default", 2, {}), ("default", 4, {}), ("within", 2, dict(within_ancestry=True))],
                         ids=["default-k2", "default-k4", "within"])
def test_mirrored_estimate(name, k, kw):
    """The alpha >= 0.5 branch (no search of these samples ends there: it starts on the low side and finds the mirror
    optimum).  L(pc1, pc2, alpha) = L(pc2, pc1, 1 - alpha): the twin of an estimate must give the same interval, and
    each PC row's SE must sit at the row that holds that value.  1 - (1 - alpha) is not alpha in the last bit, so:
    1e-9 relative on the log-likelihoods and the SEs, 4 x the root solver's stopping width on the bounds."""
    d = _sample(0.2, k=k, seed=33)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize(**kw)
        assert est["alpha"] < 0.5
        twin = _twin(est, k, name == "default")
        assert twin["alpha"] >= 0.5
        if name == "default":
            if k <= 2:
                assert np.array_equal(twin["pc"], est["pc"]) and np.array_equal(twin["pc2"], est["pc2"])
            else:
                assert np.array_equal(twin["pc"], np.concatenate([est["pc"][:2], est["pc2"][2:]]))
                assert np.array_equal(twin["pc2"], np.concatenate([est["pc2"][:2], est["pc"][2:]]))
        a = ctx.interval(est, **kw)
        b = ctx.interval(twin, **kw)
    assert abs(a["freemix"] - b["freemix"]) <= 1e-15
    for key in ("llk_max", "llk_lo", "llk_hi", "freemix_se"):
        assert abs(a[key] - b[key]) <= 1e-9 * abs(a[key]), (key, a[key], b[key])
    for key in ("lo", "hi"):
        assert abs(a[key] - b[key]) <= 4 * max(1e-6 * a[key], 1e-9), (key, a[key], b[key])
    assert a["pos_def"] and b["pos_def"] and len(a["rows"]) == len(b["rows"])
    se_of_value = {r["estimate"]: r["stderr"] for r in a["rows"][1:]}
    assert len(se_of_value) == len(a["rows"]) - 1
    for r, value in zip(b["rows"][1:], list(twin["pc"]) + ([] if name == "within" else list(twin["pc2"]))):
        assert r["estimate"] == value                        # rows in the order .Ancestry prints the PCs
        assert abs(r["stderr"] - se_of_value[value]) <= 1e-9 * se_of_value[value], (r, se_of_value[value])
    # and against the restatement, which un-swaps by its own rule
    ref = interval_ref.se_ref(d, twin, **kw)
    assert ref["swapped"] == (name == "default")
    _check_rows(b, ref, ref["cond"] * _largest_block_tolerance(d, twin, kw) * 10)


def test_fixed_pc_estimate_at_alpha_above_one_half():
    """--FixPC with alpha >= 0.5.  (The mirror image of a --FixPC estimate is no --FixPC estimate -- it would have the
    contaminant's PCs fixed -- so this one is the model's own maximum near alpha = 0.8 on a sample of that mixture,
    found on the CPU by Newton steps on the restatement; the search itself ends at alpha = 0.2022 on this sample.)
    The search's free PCs are the contaminant's; the reference prints indices 0 and 1 of the two samples swapped, so
    .Ancestry shows the fixed values as ContaminatingSample.PC1/2 and the free ones as IntendedSample.PC1/2.  The rows
    follow the values: NA beside the fixed numbers, and an IntendedSample row with its SE for each free coordinate that
    is printed there -- no free parameter's SE is dropped."""
    F = [0.01, 0.02]
    kw = dict(fix_pc=F)
    for k in (2, 4):
        fix = F + [0.0] * (k - 2)
        kw = dict(fix_pc=fix)
        d = _sample(0.8, k=k, seed=21)
        est = interval_ref.optimum_ref(d, np.zeros(k), np.array(fix), 0.8, **kw)
        assert est["alpha"] >= 0.5
        ref = interval_ref.se_ref(d, est, **kw)
        assert ref["pos_def"] and ref["swapped"]
        with vb.LikelihoodContext(d) as ctx:
            ci = ctx.interval(est, **kw)
        names = [r["param"] for r in ci["rows"]]
        assert names == (["FREEMIX"] + ["ContaminatingSample.PC%d" % (j + 1) for j in range(k)] +
                         ["IntendedSample.PC1", "IntendedSample.PC2"])
        assert all(np.isnan(r["stderr"]) for r in ci["rows"][1:3]) and [r["estimate"] for r in ci["rows"][1:3]] == F
        assert all(np.isfinite(r["stderr"]) for r in ci["rows"][3:])
        _check_rows(ci, ref, ref["cond"] * _largest_block_tolerance(d, est, kw) * 10)
        _check_profile_bounds(d, est, ci, kw)


def _check_profile_bounds(d, est, ci, kw):
    """profile_ref on either side of each interior bound straddles the cut; at a reported edge it is above the cut; and
    the interval's maximum is not below the restatement's profile at the estimate."""
    c = deriv_ref.Counts(d)
    llk = abs(est["llk1"])
    cut = ci["llk_max"] - C_HALF
    assert ci["llk_max"] >= interval_ref.profile_ref(d, est, ci["freemix"], counts=c, **kw) - 1e-9 * llk
    for b, edge, inside in ((ci["lo"], 0.0, +1), (ci["hi"], 0.5, -1)):
        if b == edge:
            assert interval_ref.profile_ref(d, est, edge, counts=c, **kw) >= cut, (b, edge)
            continue
        delta = 4 * max(1e-6 * b, 1e-9)
        v_in = interval_ref.profile_ref(d, est, b + inside * delta, counts=c, **kw)
        v_out = interval_ref.profile_ref(d, est, b - inside * delta, counts=c, **kw)
        assert v_out < cut < v_in, (b, v_out, cut, v_in)


FREE_ALPHA = [m for m in API_MODELS if m[0] != "fixalpha"]


@pytest.mark.parametrize("alpha_true", [0.03, 0.2])
@pytest.mark.parametrize("name,kw,kaf", FREE_ALPHA, ids=[m[0] for m in FREE_ALPHA])
def test_profile_bounds_in_every_model(name, kw, kaf, alpha_true):
    d = _sample(alpha_true, kaf, seed=35)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize(**kw)
        ci = ctx.interval(est, **kw)
    assert 0.0 <= ci["lo"] <= ci["freemix"] <= ci["hi"] <= 0.5
    _check_profile_bounds(d, est, ci, kw)


def _ci_file(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "#PARAM\tESTIMATE\tSTDERR\tCI_LOW\tCI_HIGH\tMETHOD"
    return [ln.split("\t") for ln in lines[1:]]


def _ostream(v):
    """A double in the default ostream format (6 significant digits), NA for none."""
    return "NA" if np.isnan(v) else "%g" % v


def test_hessian_not_negative_definite_gives_na(tmp_path):
    """A sample without contamination whose -H at the estimate is CLEARLY not positive definite -- its smallest
    eigenvalue negative by more than 1e-6 of the largest (chosen on the CPU with the oracle and se_ref; asserted again
    here), so that the kernels' rounding cannot flip it: pos_def = 0, every SE NaN, the profile bounds still there with
    lo = 0, the NOTICE on the command line's stderr and NA in the .CI columns."""
    d = vb.synth.make_pileup(300, mean_depth=10, num_pc=2, alpha_true=0.0, seed=11)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize()
        ci = ctx.interval(est)
    ref = interval_ref.se_ref(d, est)
    assert ref["eig"].min() < -1e-6 * ref["eig"].max(), ref["eig"]
    assert not ci["pos_def"] and np.isnan(ci["freemix_se"])
    assert all(np.isnan(r["stderr"]) for r in ci["rows"]) and len(ci["rows"]) == 5
    assert all(np.isnan(r["lo"]) and np.isnan(r["hi"]) for r in ci["rows"][1:])
    assert ci["lo"] == 0.0 and np.isfinite(ci["hi"]) and ci["freemix"] <= ci["hi"] <= 0.5
    assert np.isfinite(ci["llk_lo"]) and np.isfinite(ci["llk_hi"]) and np.isfinite(ci["llk_max"])
    # (hi is not held against profile_ref here: with the contaminant's PCs at (-0.21, 0.32) many allele frequencies sit on
    # their clamps and local climbs end on different maxima -- at f = 0.0072 the interval's climb ends at -864.74, Newton
    # steps on the restatement at -864.68, the oracle's simplex at -864.58.  test_profile_bounds_in_every_model does that
    # on samples where the profile has one maximum.)
    assert ci["llk_hi"] >= float(deriv_ref.derivs(d, *interval_ref.search_point(d, est)[:2], ci["hi"])[0]) - 1e-9 * abs(est["llk1"])
    pre = str(tmp_path / "clean")
    vb.synth.write_files(d, pre)
    out = str(tmp_path / "clean.out")
    p = _run(["--DisableSanityCheck", "--PileupFile", pre + ".pileup", "--SVDPrefix", pre, "--Reference", "x.fa",
              "--NumPC", "2"], out, True)
    assert "NOTICE - the Hessian of the log-likelihood at the estimate is not negative definite" in p.stderr
    assert "standard errors are NA" in p.stderr
    rows = _ci_file(out + ".CI")
    assert [r[0] for r in rows] == [r["param"] for r in ci["rows"]]
    assert rows[0][2] == "NA" and rows[0][3] == "0" and rows[0][4] == _ostream(ci["hi"]) and rows[0][5] == "profile"
    for r in rows[1:]:
        assert r[2:] == ["NA", "NA", "NA", "wald"], r


@pytest.mark.parametrize("name,kw", [("default", {}), ("within", dict(within_ancestry=True))])
def test_ci_file_holds_the_structs_numbers(tmp_path, name, kw):
    d = _sample(0.04, seed=31)
    pre = str(tmp_path / "syn")
    vb.synth.write_files(d, pre)
    out = str(tmp_path / ("syn." + name))
    res = vb.run_files(pre, pre + ".pileup", output_prefix=out, num_pc=2, disable_sanity=True, confidence_interval=True,
                       **kw)
    ci = res["interval"]
    assert ci["pos_def"] and ci["freemix"] == res["alpha"]
    rows = _ci_file(out + ".CI")
    assert len(rows) == len(ci["rows"]) == (5 if name == "default" else 3)
    for got, r in zip(rows, ci["rows"]):
        assert got == [r["param"], _ostream(r["estimate"]), _ostream(r["stderr"]), _ostream(r["lo"]), _ostream(r["hi"]),
                       r["method"]], (got, r)
    # and the struct is the context's: the same sample through the arrays
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize(**kw)
        direct = ctx.interval(est, **kw)
    ref = interval_ref.se_ref(d, est, **kw)
    _check_rows(direct, ref, ref["cond"] * _largest_block_tolerance(d, est, kw) * 10)
    assert [r["param"] for r in direct["rows"]] == [r["param"] for r in ci["rows"]]
    for a, b in zip(direct["rows"], ci["rows"]):
        assert _ostream(a["estimate"]) == _ostream(b["estimate"]) and _ostream(a["stderr"]) == _ostream(b["stderr"])
