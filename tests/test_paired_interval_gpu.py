"""The interval of a paired refit on the MI355X (vb2_paired_interval, vb2_cohort_run_paired_intervals, --PairInterval; DESIGN.md
section 17): every standard error and Wald bound and the profile bounds against the numpy restatement
(tests/paired_deriv_ref.py) under the default model, --FixPC and known allele frequencies; the branches (lo = 0, a hypothesis
that walks nothing, a Hessian that is not negative definite); two sets on two contexts in one gang; the calibration over 40
seeds against the restatement's own (profiles/paired_interval/calibration_restatement.json); the command line end to end.

Measured on an MI355X (pair_case's tumour with the allelic shift): alpha 0.029349, SE 0.00165, interval [0.02624, 0.03272];
cond(A) 366 and an accepted relative error of 3.7e-10 under the default model, 1e-12 with --FixPC and known AF.  End to end
(seed 42): tumour 0 ALPHA_PAIRED 0.030109, SE 0.00168, [0.02695, 0.03355] for a planted 0.03 (FREEMIX 0.054223); tumour 2
ALPHA_PAIRED 0.046854, SE 0.00212, [0.04286, 0.05117] for a planted 0.05.
"""
import json
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import deriv_ref  # noqa: E402
import paired_deriv_ref as pdr  # noqa: E402
import paired_interval_calibration as calib  # noqa: E402
import paired_ref as pr  # noqa: E402
from deriv_ref import Counts  # noqa: E402
from test_paired_gpu import _run_cli, _write_cohort  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_HALF = 1.9207294103470620
Z = 1.959963984540054


@pytest.fixture(scope="module")
def case():
    """pair_case at its own seed: the tumour with the shift (and the same with known AF), the rule's hypothesis from its
    normal, one from a stranger, and the held PCs."""
    import copy
    panel, shifted_t, plain_t, normal, stranger = pr.pair_case()
    known = copy.deepcopy(shifted_t)
    known.known_af = np.clip(known.means / 2.0, 0.01, 0.99)
    rows = np.stack([pr.normal_rule(pr.normal_q(n), 0.99) for n in (normal, stranger)])
    return dict(tumour=shifted_t, tumour_af=known, plain=plain_t, rows=rows, fixed=np.zeros(2))


MODELS = {"default": ("tumour", dict(), False), "fix_pc": ("tumour", dict(fix_pc=[0.01, -0.02]), True),
          "known_af": ("tumour_af", dict(), False)}


def _close(x, want, rel):
    return bool(np.isnan(x)) if np.isnan(want) else bool(abs(x - want) <= rel * abs(want))


def _check_profile_bounds(c, hyp, est, pc2, ci, fix_pc):
    """tests/test_interval_gpu.py's check, unfolded: the restatement's profile straddles the cut on either side of each
    interior bound and is above it at a reported edge."""
    llk = abs(est["llk1"])
    cut = ci["llk_max"] - C_HALF
    assert ci["llk_max"] >= pdr.profile_ref(c, hyp, est, pc2, ci["freemix"], fix_pc) - 1e-9 * llk
    for b, edge, inside in ((ci["lo"], 0.0, +1), (ci["hi"], 1.0, -1)):
        if b == edge:
            assert pdr.profile_ref(c, hyp, est, pc2, edge, fix_pc) >= cut, (b, edge)
            continue
        delta = 4 * max(1e-6 * b, 1e-9)
        v_in = pdr.profile_ref(c, hyp, est, pc2, b + inside * delta, fix_pc)
        v_out = pdr.profile_ref(c, hyp, est, pc2, b - inside * delta, fix_pc)
        assert v_out < cut < v_in, (b, v_out, cut, v_in)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_interval_matches_the_restatement(case, name):
    """Every SE and Wald bound within cond(A) x (the largest block tolerance of the derivative check at the estimate) x 10,
    tests/test_interval_gpu.py's rule; the profile bounds straddled by the restatement's plain Newton profile."""
    which, model, fix_pc = MODELS[name]
    d, hyp, pc2 = case[which], case["rows"][0], case["fixed"]
    c64, c80 = Counts(d), Counts(d, np.longdouble)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, hyp[None]) as pair:
        (est,) = pair.optimize(pc2, **model)
        assert est["status"] == 0
        (ci,) = pair.interval([est], pc2, **model)
        assert pair.info()["given"][0] == pr.given_count(c64, hyp)
    ref = pdr.se_ref(c64, hyp, est, pc2, fix_pc=fix_pc)
    assert ref["pos_def"] and ci["status"] == 0
    at = pdr.reference(c64, c80, hyp, est["pc"][:2], pc2, est["alpha"])
    tol = max(t for _, _, t in deriv_ref.block_devs(at, at["g64"], at["h64"]).values())
    rel = ref["cond"] * tol * 10
    print("%s: alpha %.6g SE %.3g interval [%.5g, %.5g]; cond(A) %.3g, accepted relative error %.3g"
          % (name, ci["freemix"], ci["freemix_se"], ci["lo"], ci["hi"], ref["cond"], rel))
    assert rel < 1e-4                                        # the bound itself has not gone soft
    assert ci["freemix"] == est["alpha"] and ci["alpha_free"] and ci["pos_def"] and ci["num_free"] == ref["num_free"]
    assert [r["param"] for r in ci["rows"]] == ["FREEMIX"] + [n for n, _, _ in ref["rows"][1:]]
    assert len(ci["rows"]) == (3 if name == "default" else 1)
    assert _close(ci["freemix_se"], ref["alpha_se"], rel), (ci["freemix_se"], ref["alpha_se"], rel)
    for row, (n, value, se) in zip(ci["rows"], ref["rows"]):
        assert row["estimate"] == value and _close(row["stderr"], se, rel), (n, row, se, rel)
        if n != "ALPHA":
            assert abs(row["lo"] - (value - Z * se)) <= rel * Z * se and abs(row["hi"] - (value + Z * se)) <= rel * Z * se
    assert ci["rows"][0]["lo"] == ci["lo"] and ci["rows"][0]["hi"] == ci["hi"]
    assert 0.0 < ci["lo"] < est["alpha"] < ci["hi"] < 1.0
    _check_profile_bounds(c64, hyp, est, pc2, ci, fix_pc)


def test_a_strangers_normal_keeps_the_interval_on_its_own_side(case):
    d, hyp, pc2 = case["plain"], case["rows"][1], case["fixed"]
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, hyp[None]) as pair:
        (est,) = pair.optimize(pc2)
        (ci,) = pair.interval([est], pc2)
    assert est["alpha"] > 0.9 and ci["status"] == 0 and ci["freemix"] == est["alpha"]
    assert 0.5 < ci["lo"] <= est["alpha"] <= ci["hi"] <= 1.0
    _check_profile_bounds(Counts(d), hyp, est, pc2, ci, False)


def test_a_clean_tumour_has_lo_zero_and_an_empty_hypothesis_fails_alone():
    import source_ref as sr
    panel = sr.make_panel(3000, 2, seed=5)
    G = sr.draw_individuals(panel, 3, seed=6)
    tumour = sr.make_sample(panel, G[0], G[1], 30, 0.0, 70)
    normal = sr.make_sample(panel, G[0], G[2], 30, 1e-3, 71)
    hyp = pr.normal_rule(pr.normal_q(normal), 0.99)
    nothing = np.zeros_like(hyp)
    nothing[:, 3:] = pr.LEFT_OUT
    pc2 = np.zeros(2)
    c = Counts(tumour)
    with vb.LikelihoodContext(tumour) as ctx, vb.Paired(ctx, np.stack([nothing, hyp])) as pair:
        est = pair.optimize(pc2)
        assert est[0]["status"] == _abi.VB2_ERR_INVALID and est[1]["status"] == 0
        ci = pair.interval(est, pc2)
        assert ci[0]["status"] == _abi.VB2_ERR_INVALID and ci[0]["num_launch"] == 0
        with vb.Paired(ctx, hyp[None]) as alone:
            (want,) = alone.interval(est[1:], pc2)
    got = ci[1]
    assert got["status"] == 0 and got["lo"] == 0.0 and got["freemix"] == est[1]["alpha"] <= got["hi"] < 0.5
    assert pdr.profile_ref(c, hyp, est[1], pc2, 0.0) >= got["llk_max"] - C_HALF
    for key in want:
        if key != "rows":
            assert got[key] == want[key] or (np.isnan(got[key]) and np.isnan(want[key])), key


def test_hessian_not_negative_definite_gives_na():
    """A small clean sample whose -H in the free coordinates is CLEARLY not positive definite at the estimate -- chosen on the
    restatement (eigenvalues -0.79, 0.08, 1.75 at alpha = 0.0012) and asserted again here, so that the kernels' rounding
    cannot flip it: pos_def = 0, every SE NaN, the profile bounds still there."""
    import source_ref as sr
    panel = sr.make_panel(300, 2, seed=11)
    G = sr.draw_individuals(panel, 3, seed=12)
    tumour = sr.make_sample(panel, G[0], G[1], 10, 0.0, 80)
    normal = sr.make_sample(panel, G[0], G[2], 30, 1e-3, 81)
    hyp = pr.normal_rule(pr.normal_q(normal), 0.99)
    pc2 = np.zeros(2)
    with vb.LikelihoodContext(tumour) as ctx, vb.Paired(ctx, hyp[None]) as pair:
        (est,) = pair.optimize(pc2)
        (ci,) = pair.interval([est], pc2)
    ref = pdr.se_ref(Counts(tumour), hyp, est, pc2)
    eig = np.linalg.eigvalsh(ref["A"])
    assert not ref["pos_def"] and eig.min() < -1e-6 * eig.max(), eig
    assert ci["status"] == 0 and not ci["pos_def"] and np.isnan(ci["freemix_se"])
    assert all(np.isnan(r["stderr"]) for r in ci["rows"]) and all(np.isnan(r["lo"]) for r in ci["rows"][1:])
    assert 0.0 <= ci["lo"] <= est["alpha"] <= ci["hi"] <= 1.0 and ci["num_profile"] >= 3


def test_two_sets_on_two_contexts_in_one_gang(case):
    """out[i] is bit for bit what the hypothesis gives alone, and num_step is the largest num_launch."""
    a, b, rows, fixed = case["tumour"], case["plain"], case["rows"], case["fixed"]
    other = np.array([0.002, -0.001])
    with vb.LikelihoodContext(a) as ca, vb.LikelihoodContext(b) as cb, vb.Paired(ca, rows) as sa, vb.Paired(cb, rows[:1]) as sb:
        est = vb.Paired.optimize_sets([sa, sb], [fixed, other])
        both, steps = vb.Paired.interval_sets([sa, sb], est, [fixed, other])
        alone = [vb.Paired.interval_sets([sa], est[:1], [fixed]), vb.Paired.interval_sets([sb], est[1:], [other])]
        launches = []
        for s in range(2):
            assert alone[s][1] == max(c["num_launch"] for c in alone[s][0][0])
            for got, want in zip(both[s], alone[s][0][0]):
                assert got["status"] == 0
                launches.append(got["num_launch"])
                for key in want:
                    if key == "rows":
                        assert got["rows"] == want["rows"] or all(
                            x[f] == y[f] or (np.isnan(x[f]) and np.isnan(y[f])) for x, y in zip(got["rows"], want["rows"]) for f in y)
                    else:
                        assert got[key] == want[key] or (np.isnan(got[key]) and np.isnan(want[key])), (s, key)
        assert steps == max(launches) and len(launches) == 3 and steps < sum(launches)


@pytest.mark.parametrize("shifted", [True, False], ids=["shifted", "plain"])
def test_calibration_over_40_seeds(shifted):
    """The same seeds are covered as by the restatement, and at least 33 of 40: the existing interval test's cap, which an
    exact 95 % interval misses with probability below 0.2 % (P(Bin(40, 0.05) >= 8))."""
    want = json.load(open(os.path.join(ROOT, "profiles", "paired_interval", "calibration_restatement.json")))
    assert want["seeds"] == calib.SEEDS and want["planted"] == calib.PLANTED and want["hom_min"] == calib.HOM_MIN
    ref = {r["seed"]: r for r in want["rows"] if r["shifted"] == shifted}
    covered = []
    for seed in calib.SEEDS:
        tumour, hyp, pc2 = calib.case(seed, shifted)
        with vb.LikelihoodContext(tumour) as ctx, vb.Paired(ctx, hyp[None]) as pair:
            (est,) = pair.optimize(pc2)
            (ci,) = pair.interval([est], pc2)
        assert est["status"] == 0 and ci["status"] == 0
        covered.append(bool(ci["lo"] <= calib.PLANTED <= ci["hi"]))
        r = ref[seed]
        assert covered[-1] == r["covered"], (seed, ci["lo"], ci["hi"], r)
        assert abs(ci["lo"] - r["lo"]) <= 1e-4 * max(r["lo"], 1e-3) and abs(ci["hi"] - r["hi"]) <= 1e-4 * r["hi"], (seed, ci, r)
    print("covered %d of %d (%s)" % (sum(covered), len(covered), "shifted" if shifted else "plain"))
    assert sum(covered) == want["covered_of_40"]["shifted" if shifted else "plain"]
    assert sum(covered) >= 33, sum(covered)


# ---- end to end: --PileupList --MatchedNormal --PairInterval ----

HEADER = ["#TUMOUR", "NORMAL", "MARKERS", "ALPHA_PAIRED", "SE", "LO95", "HI95", "LLK_MAX", "LLK_LO", "LLK_HI", "POS_DEF",
          "PROFILE_POINTS"]


def _read_ci(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == HEADER
    return [ln.split("\t") for ln in lines[1:]]


def _ci_row(f, piles):
    g = lambda x: "NA" if np.isnan(x) else "%g" % x
    row = [piles[f["tumour"]], piles[f["normal"]]]
    if "interval" not in f:
        return row + ["NA"] * 10
    c = f["interval"]
    return row + [str(f["markers"]), g(c["freemix"]), g(c["freemix_se"]), g(c["lo"]), g(c["hi"]), g(c["llk_max"]), g(c["llk_lo"]),
                  g(c["llk_hi"]), str(int(c["pos_def"])), str(c["num_profile"])]


@pytest.mark.parametrize("stream", [True, False])
def test_end_to_end_pair_interval(tmp_path, stream, tunable):
    tunable("cohort_stream", 1 if stream else 0)
    data, prefix, piles, outs, lst = _write_cohort(tmp_path)
    pairs_file = str(tmp_path / "pairs.txt")
    with open(pairs_file, "w") as f:
        for t, n in pr.COHORT_PAIRS:
            f.write("%s\t%s\n" % (piles[t], piles[n]))
    plain = _run_cli(prefix, lst, str(tmp_path / "run"), pairs_file, stream)
    assert plain.returncode == 0, plain.stderr[-2000:]
    others = [o + ext for o in outs for ext in (".selfSM", ".Ancestry")] + [str(tmp_path / "run.PairFit")]
    before = [open(p, "rb").read() for p in others]
    assert not os.path.exists(str(tmp_path / "run.PairCI"))
    with_ci = _run_cli(prefix, lst, str(tmp_path / "run"), pairs_file, stream, extra=["--PairInterval"])
    assert with_ci.returncode == 0, with_ci.stderr[-2000:]
    # stdout, .selfSM, .Ancestry and .PairFit: byte for byte what the run without the flag wrote
    assert with_ci.stdout == plain.stdout
    assert [open(p, "rb").read() for p in others] == before
    rows = _read_ci(str(tmp_path / "run.PairCI"))
    res, fits = vb.run_cohort_files(prefix, piles, num_pc=2, matched_normal=pr.COHORT_PAIRS, pair_interval=True)
    assert rows == [_ci_row(f, piles) for f in fits]
    for f, (t, n) in zip(fits, pr.COHORT_PAIRS):
        c = f["interval"]
        assert f["status"] == 0 and c["freemix"] == f["alpha_paired"] and c["pos_def"]
        assert 0.0 <= c["lo"] <= f["alpha_paired"] <= c["hi"] <= 1.0
        print("tumour %d: ALPHA_PAIRED %.6f SE %.3g [%.5f, %.5f], planted %.3f, FREEMIX %.6f"
              % (t, f["alpha_paired"], c["freemix_se"], c["lo"], c["hi"], pr.COHORT_PLANTED[t], f["freemix"]))
    # --PairInterval without --MatchedNormal is refused with a message
    import subprocess
    from test_paired_gpu import CLI
    p = subprocess.run([CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupList", lst, "--Output",
                        str(tmp_path / "bad"), "--PairInterval"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--PairInterval needs --MatchedNormal" in p.stderr


def test_a_normal_that_fails_its_sanity_check_gives_an_na_row_and_disturbs_nobody(tmp_path):
    data, prefix, piles, outs, lst = _write_cohort(tmp_path, extra_failing=True)
    bad = len(piles) - 1
    res, fits = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, matched_normal=[(0, 1), (2, bad)],
                                    sources_prefix=str(tmp_path / "run"), pair_interval=True)
    assert res[bad]["status"] == _abi.VB2_ERR_SANITY
    assert fits[1]["status"] == _abi.VB2_PAIR_FIT_NONE and "interval" not in fits[1] and "interval" in fits[0]
    rows = _read_ci(str(tmp_path / "run.PairCI"))
    assert rows[1] == [piles[2], piles[bad]] + ["NA"] * 10
    res6, fits6 = vb.run_cohort_files(prefix, piles[:bad], num_pc=2, matched_normal=[(0, 1), (2, 3)], pair_interval=True)
    assert rows[0] == _ci_row(fits6[0], piles)
    a, b = fits6[0]["interval"], fits[0]["interval"]
    assert all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a if k != "rows")
