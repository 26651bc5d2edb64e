"""The likelihood given a hypothesised contaminant on the MI355X (marker_sum_kernels.hip, conditioned.cpp; DESIGN.md section
13): vb2_conditioned_eval against the np.longdouble restatement (tests/conditioned_ref.py) in both layouts, the KSEL-compiled
and the general --NumPC, a known-AF column, every kind of hypothesis row and of step; the bits of a point whatever the step
holds; create_from_set against create; the lock-step refits against the same searches on the float64 restatement through
the host seam under three models; two sets on two contexts in one call.

The largest |kernel - restatement| / |restatement| over every evaluation case of this module, per layout, is printed at the
module's end (pytest -s); the checks fail above LLK_RTOL = 1e-12.  Measured on an MI355X:

    layout 0 (run words)           3.9e-16  (300 x 30, k = 4, one-hot on the heterozygote, alpha = 0.03)
    layout 1 (probability domain)  3.9e-16  (3 000 x 30, k = 2, one-hot on the heterozygote, alpha = 1e-6)

Refits (3 000 x 30, k = 2): alpha, llk1 and the evaluation counts are the float64 restatement's under all three models.  End
to end (seed 42): sample 0 ALPHA_GIVEN 0.053203 (restatement 0.053203), DELTA_LK +398.41; sample 2: no refit.
"""
import os
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")

LLK_RTOL = 1e-12                  # the project's evaluation tolerance (tests/test_gpu_parity.py)
ALPHAS = [0.0, 1e-6, 0.03, 0.5, 1.0]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for layout in sorted(_WORST):
        print("\nlayout %d: worst |kernel - restatement| / |restatement| = %.3g (%s)" % ((layout,) + _WORST[layout]))


def _close(got, want, layout, label):
    want = float(want)
    rel = abs(got - want) / abs(want) if want != 0 else abs(got)
    if rel > _WORST.get(layout, (-1.0, ""))[0]:
        _WORST[layout] = (rel, label)
    assert rel <= LLK_RTOL, (label, got, want, rel)


def _other_q(d, seed):
    """Another sample's genotype posterior as the device would hold it: float32 [M, 3], zeros where it counts nothing."""
    o = vb.synth.make_pileup(d.num_marker, mean_depth=15, num_pc=d.num_pc, alpha_true=0.01, seed=seed, missing_frac=0.1)
    z = np.zeros(d.num_pc)
    return sr.sample_rows(o, z, z, 1e-3)[1].astype(np.float32)


def _hyp_rows(d, seed):
    """all zero; one-hot on each genotype; another sample's q; that row with every third marker zeroed; that row with exact
    zeros for two genotypes on a marker whose reads contradict the third."""
    M = d.num_marker
    q = _other_q(d, seed)
    third = q.copy()
    third[::3] = 0
    contra = q.copy()
    c64 = Counts(d)
    z = np.zeros(d.num_pc)
    m = sr.marginals(c64, z, z, 0.05)
    depth = np.diff(d.read_off)[c64.idx]
    ok = m["live"] & (depth <= 100)
    assert ok.any()
    worst = int(np.argmin(np.where(ok, m["c"].min(axis=1), np.inf)))
    contra[c64.idx[worst]] = np.eye(3, dtype=np.float32)[int(np.argmin(m["c"][worst]))]
    eye = np.eye(3, dtype=np.float32)
    rows = [np.zeros((M, 3), dtype=np.float32)] + [np.tile(eye[g], (M, 1)) for g in range(3)] + [q, third, contra]
    return np.stack(rows)


def _points(k, n, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, (n, k)), rng.normal(0, scale, (n, k)), np.array([ALPHAS[i % len(ALPHAS)] for i in range(n)])


def _check_eval(d, ctx, cond, rows, steps, seed, label):
    """Every point of `steps` (lists of points per hypothesis) against the 80-bit restatement."""
    layout = ctx.info()["layout"]
    c80 = Counts(d, np.longdouble)
    for s, num_point in enumerate(steps):
        P = int(np.sum(num_point))
        pc1, pc2, alpha = _points(d.num_pc, P, seed + s)
        got = cond.eval(num_point, pc1, pc2, alpha)
        assert got.shape == (P,)
        p = 0
        for h, n in enumerate(num_point):
            for _ in range(n):
                where = "%s hypothesis %d alpha=%g" % (label, h, alpha[p])
                _close(got[p], cr.llk(c80, rows[h], pc1[p], pc2[p], alpha[p]), layout, where)
                if h == 0:                                   # all zero: the anonymous model
                    _close(got[p], ctx.llk(pc1[p], pc2[p], alpha[p])[0], layout, where + " vs ctx.llk")
                if 1 <= h <= 3 and alpha[p] == 0.0:          # a normalised prior drops out at alpha = 0
                    _close(got[p], ctx.llk(pc2[p], pc2[p], 0.0)[0], layout, where + " vs ctx.llk(pc2, pc2, 0)")
                p += 1


# points per hypothesis: 0 (the hypothesis sits the step out), 1, 4 and 8; every row is evaluated at every alpha in some step
STEPS = [[8, 1, 4, 8, 4, 1, 0], [5, 5, 5, 0, 5, 8, 5], [1, 0, 0, 1, 0, 0, 1]]


@pytest.mark.parametrize("M, k, pd", [(1, 2, 1), (17, 1, 0), (17, 4, 1), (300, 4, 0), (300, 1, 1), (3000, 2, 0), (3000, 2, 1)])
def test_eval_matches_the_restatement(M, k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=k, alpha_true=0.05, seed=100 + M + k)
    rows = _hyp_rows(d, M + 1)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        with vb.Conditioned(ctx, rows) as cond:
            info = cond.info()
            assert info["num_hyp"] == 7 and info["num_marker"] == M and info["device_bytes"] > 0
            _check_eval(d, ctx, cond, rows, STEPS, seed=M, label="%dx%d k=%d" % (M, 30, k))


@pytest.mark.parametrize("pd", [0, 1])
def test_eval_with_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(300, mean_depth=25, num_pc=2, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, 300), 0.0, 1.0)
    rows = _hyp_rows(d, 3)
    with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, rows) as cond:
        assert ctx.info()["layout"] == pd
        _check_eval(d, ctx, cond, rows, STEPS[:2], seed=5, label="known AF")


def test_eval_of_a_sample_that_takes_run_words_whatever_the_switch(tunable):
    """Three markers deeper than the probability-domain bound (about 900 reads) among 300 ordinary ones, and quality-0 reads."""
    tunable("pd", 1)
    a = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=31, q_lo=0, q_hi=40)
    b = vb.synth.make_pileup(3, mean_depth=1000, num_pc=2, alpha_true=0.05, seed=32)
    d = vb.PileupData(2, np.concatenate([a.ud, b.ud]), np.concatenate([a.means, b.means]),
                      np.concatenate([a.read_off, a.read_off[-1] + b.read_off[1:]]), np.concatenate([a.bases, b.bases]),
                      np.concatenate([a.quals, b.quals]), np.concatenate([a.alt_base, b.alt_base]), None, a.avg_depth, 0.0, True)
    rows = _hyp_rows(d, 9)
    with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, rows) as cond:
        assert ctx.info()["layout"] == 0
        _check_eval(d, ctx, cond, rows, STEPS[:2], seed=6, label="deep + q0")


def test_eval_with_missing_and_depth_filtered_markers():
    d = vb.synth.make_pileup(3000, mean_depth=20, num_pc=2, alpha_true=0.05, seed=21, missing_frac=0.15)
    d = vb.synth.with_sanity_stats(d)
    depth = np.diff(d.read_off)
    gone = (depth == 0) | (depth < d.avg_depth - 3 * d.sd_depth) | (depth > d.avg_depth + 3 * d.sd_depth)
    assert (depth == 0).sum() > 300 and gone.sum() > (depth == 0).sum() and not d.sanity_disabled
    rows = _hyp_rows(d, 4)
    with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, rows) as cond:
        _check_eval(d, ctx, cond, rows, STEPS[:2], seed=7, label="missing + filtered")


@pytest.fixture(scope="module")
def sample_3000():
    return vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=77)


@pytest.mark.parametrize("pd", [0, 1])
def test_a_step_of_49_points_and_the_bits_of_a_point(sample_3000, pd, tunable):
    """7 hypotheses x 7 points cross the launch boundary (48 points); one hypothesis's point gives the same bits alone, as
    the last of the 49, beside three other hypotheses and on a second call."""
    tunable("pd", pd)
    d = sample_3000
    rows = _hyp_rows(d, 12)
    with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, rows) as cond:
        assert ctx.info()["layout"] == pd
        before = cond.info()
        _check_eval(d, ctx, cond, rows, [[7] * 7], seed=49, label="49 points")
        after = cond.info()
        assert after["num_step"] == before["num_step"] + 1 and after["num_launch"] == before["num_launch"] + 2
        pc1, pc2, alpha = _points(2, 49, 49)
        alpha[-1] = 0.03
        full = cond.eval([7] * 7, pc1, pc2, alpha)
        again = cond.eval([7] * 7, pc1, pc2, alpha)
        assert full.tobytes() == again.tobytes()
        alone = cond.eval([0, 0, 0, 0, 0, 0, 1], pc1[-1:], pc2[-1:], alpha[-1:])
        assert alone.tobytes() == full[-1:].tobytes()
        # the same point behind three other hypotheses' points, and twice in one step
        mixed = cond.eval([3, 0, 8, 0, 1, 0, 2], np.concatenate([pc1[:12], pc1[-1:], pc1[-1:]]),
                          np.concatenate([pc2[:12], pc2[-1:], pc2[-1:]]), np.concatenate([alpha[:12], alpha[-1:], alpha[-1:]]))
        assert mixed[-1:].tobytes() == alone.tobytes() and mixed[-2:-1].tobytes() == alone.tobytes()
        # an alpha outside [0, 1] leaves every marker out, as in vb2_llk_eval_batch
        out = cond.eval([1, 0, 0, 0, 1, 0, 0], pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        want = ctx.llk(pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        assert out.tobytes() == want.tobytes() or np.array_equal(out, want)


def test_argument_errors(sample_3000):
    d = sample_3000
    with vb.LikelihoodContext(d) as ctx:
        with pytest.raises(ValueError):
            vb.Conditioned(ctx, np.ones((2, d.num_marker - 1, 3)))
        with pytest.raises(_abi.Vb2Error):
            vb.Conditioned(ctx, np.ones((0, d.num_marker, 3)))
        with vb.Conditioned(ctx, np.ones((2, d.num_marker, 3))) as cond:
            with pytest.raises(_abi.Vb2Error):
                cond.eval([9, 0], np.zeros((9, 2)), np.zeros((9, 2)), np.full(9, 0.1))
            assert cond.eval([0, 0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)).shape == (0,)
            with pytest.raises(_abi.Vb2Error, match="fixed alpha"):
                cond.optimize(np.zeros(2), fix_alpha=0.01)


# ---- a cohort in which the source is known ----

@pytest.fixture(scope="module")
def cohort():
    """3 000 x 30, k = 2: target 0 contaminated at 5 % by member 1; members 1 and 2 clean; the same target with known AF."""
    panel = sr.make_panel(3000, 2, seed=21)
    G = sr.draw_individuals(panel, 4, seed=22)
    target = sr.make_sample(panel, G[0], G[1], 30, 0.05, 200)
    target_af = sr.make_sample(panel, G[0], G[1], 30, 0.05, 200, known_af=True)
    members = [sr.make_sample(panel, G[i], G[3], 30, 0.0, 200 + i) for i in (1, 2)]
    z = np.zeros(2)
    qs = [sr.sample_rows(m, z, z, 1e-3)[1].astype(np.float32) for m in members]
    rows = np.stack([qs[0], qs[1], np.zeros_like(qs[0])])            # the true source, a non-source, all zero
    return dict(target=target, target_af=target_af, members=members, rows=rows, fixed=np.array([0.004, -0.003]))


def test_create_from_set_gives_the_bits_of_create(cohort):
    target, members = cohort["target"], cohort["members"]
    est = dict(pc=np.array([0.002, -0.001]), pc2=np.array([0.001, 0.003]), alpha=0.002)
    with vb.LikelihoodContext(target) as ctx, vb.SourceSet(target.num_marker, 2) as ss:
        host = []
        for m in members:
            with vb.LikelihoodContext(m) as c:
                assert ss.add(c, est) == len(host)
                host.append(c.marginals(est["pc"], est["pc2"], est["alpha"])[1].astype(np.float32))
        assert all(h.any() for h in host)
        pc1, pc2, alpha = _points(2, 10, 3)
        with vb.Conditioned(ctx, source_set=ss, candidates=[1, 0]) as a, vb.Conditioned(ctx, np.stack([host[1], host[0]])) as b:
            assert a.num_hyp == 2
            got, want = a.eval([5, 5], pc1, pc2, alpha), b.eval([5, 5], pc1, pc2, alpha)
            assert got.tobytes() == want.tobytes() and got[0] != got[5]
        with pytest.raises(_abi.Vb2Error):
            vb.Conditioned(ctx, source_set=ss, candidates=[2])


MODELS = {"default": ("target", dict()), "fix_pc": ("target", dict(fix_pc=[0.01, -0.02])), "known_af": ("target_af", dict())}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_refits_match_the_restatements_searches(cohort, name):
    which, model = MODELS[name]
    d, rows, fixed = cohort[which], cohort["rows"], cohort["fixed"]
    c64 = Counts(d)
    want, _ = cr.search([c64] * 3, list(rows), np.tile(fixed, (3, 1)), known_af=d.known_af is not None, **model)
    with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, rows) as cond:
        got = cond.optimize(fixed, **model)
        for h in range(3):
            g, w = got[h], want[h]
            print("%s hypothesis %d: alpha %.9g (restatement %.9g), -llk1 %.12g (restatement %.12g), -llk0 %.12g, %d evaluations (%d)"
                  % (name, h, g["alpha"], w["alpha"], -g["llk1"], -w["llk1"], -g["llk0"], g["num_eval"], w["num_eval"]))
            assert g["status"] == 0 and w["status"] == 0 and g["converged"]
            assert abs(g["alpha"] - w["alpha"]) <= 1e-4, (name, h, g["alpha"], w["alpha"])
            assert abs(g["llk1"] - w["llk1"]) <= 1e-6 * abs(w["llk1"]), (name, h, g["llk1"], w["llk1"])
            assert np.array_equal(g["pc"], g["pc2"])
            npt = [0] * 3
            npt[h] = 1
            at = cond.eval(npt, fixed[None], g["pc2"][None], [g["alpha"]])[0]
            assert abs(-at - g["llk1"]) <= LLK_RTOL * abs(g["llk1"]), (name, h, at, g["llk1"])
        # the true source explains the reads better than a random contaminant, a stranger worse; alpha is the source's share
        assert got[0]["llk1"] < got[2]["llk1"] < got[1]["llk1"]
        assert abs(got[0]["alpha"] - 0.05) < 0.01
        if name == "known_af":
            # pc1 is irrelevant with known allele frequencies: the all-zero hypothesis is the anonymous model's own search
            alone = ctx.optimize(within_ancestry=True)
            print("known_af all-zero hypothesis against ctx.optimize(): alpha differs by %.3g" % abs(got[2]["alpha"] - alone["alpha"]))
            assert abs(got[2]["alpha"] - alone["alpha"]) <= 1e-4
            assert abs(got[2]["llk1"] - alone["llk1"]) <= 1e-6 * abs(alone["llk1"])


def test_two_sets_on_two_contexts_in_one_call(cohort):
    a, b, rows, fixed = cohort["target"], cohort["members"][1], cohort["rows"], cohort["fixed"]
    other = np.array([-0.002, 0.006])
    with vb.LikelihoodContext(a) as ca, vb.LikelihoodContext(b) as cb, vb.Conditioned(ca, rows[:2]) as sa, \
            vb.Conditioned(cb, rows[1:]) as sb:
        alone = [sa.optimize(fixed), sb.optimize(other)]
        both = vb.Conditioned.optimize_sets([sa, sb], [fixed, other])
        for s in range(2):
            for g, w in zip(both[s], alone[s]):
                assert g["status"] == 0 and g["alpha"] == w["alpha"] and g["llk1"] == w["llk1"] and g["llk0"] == w["llk0"]
                assert np.array_equal(g["pc2"], w["pc2"])
        assert both[0][0]["alpha"] != both[1][0]["alpha"]


# ---- end to end: --PileupList --FindSource --RefitSource ----

HEADER = ["#SAMPLE", "CANDIDATE", "LLR", "MARKERS", "FREEMIX", "FREELK1", "ALPHA_GIVEN", "LK1_GIVEN", "LK0_GIVEN", "DELTA_LK"]


def _write_cohort(tmp, extra_failing=False):
    from verifybamid_amd import synth
    panel, data = cr.fit_cohort()
    M = data[0].num_marker
    prefix = str(tmp / "panel")
    synth.write_files(data[0], prefix)                           # .UD / .mu / .bed (and sample 0's pileup)
    chrs, poss = ["1"] * M, 1000 + 10 * np.arange(M)
    piles, outs = [], []
    for i, d in enumerate(data):
        p = str(tmp / ("s%02d.pileup" % i))
        synth.write_pileup_text(p, chrs, poss, panel["ref"], d.read_off, d.bases, d.quals)
        piles.append(p)
        outs.append(str(tmp / ("s%02d" % i)))
    if extra_failing:                                            # 300 covered markers: fails the sanity check
        d = data[4]
        off = d.read_off.copy()
        off[301:] = off[300]
        p = str(tmp / "bad.pileup")
        synth.write_pileup_text(p, chrs, poss, panel["ref"], off, d.bases, d.quals)
        piles.insert(5, p)
        outs.insert(5, str(tmp / "bad"))
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        for p, o in zip(piles, outs):
            f.write("%s\t%s\n" % (p, o))
    return data, prefix, piles, outs, lst


def _run_cli(prefix, lst, out, refit, stream):
    env = dict(os.environ)
    if not stream:
        env["VB2_COHORT_STREAM"] = "0"
    args = [CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupList", lst, "--Output", out, "--FindSource"]
    return subprocess.run(args + (["--RefitSource"] if refit else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=600)


def _read_fit(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == HEADER
    return [ln.split("\t") for ln in lines[1:]]


def _fit_row(f, outs, i):
    g = lambda x: "%g" % x
    row = [outs[i], outs[f["candidate"]], g(f["llr"]), str(f["markers"]), g(f["freemix"]), g(f["freelk1"])]
    if f["status"] == 0:
        return row + [g(f["alpha_given"]), g(f["lk1_given"]), g(f["lk0_given"]), g(f["delta_lk"])]
    return row + ["NA"] * 4


@pytest.mark.parametrize("stream", [True, False])
def test_end_to_end_refit_source(tmp_path, stream, tunable):
    tunable("cohort_stream", 1 if stream else 0)               # (the in-process run below, like the command line's)
    data, prefix, piles, outs, lst = _write_cohort(tmp_path)
    n = len(piles)
    found = _run_cli(prefix, lst, str(tmp_path / "run"), refit=False, stream=stream)
    assert found.returncode == 0, found.stderr[-2000:]
    others = [o + ext for o in outs for ext in (".selfSM", ".Ancestry")] + [str(tmp_path / "run.Sources")]
    before = [open(p, "rb").read() for p in others]
    assert not os.path.exists(str(tmp_path / "run.SourceFit"))
    refit = _run_cli(prefix, lst, str(tmp_path / "run"), refit=True, stream=stream)
    assert refit.returncode == 0, refit.stderr[-2000:]
    # stdout, .selfSM, .Ancestry and .Sources: byte for byte what the run without the flag wrote
    assert refit.stdout == found.stdout
    assert [open(p, "rb").read() for p in others] == before
    assert b"stayed on the device for the refit" in refit.stderr
    rows = _read_fit(str(tmp_path / "run.SourceFit"))
    # the fit array of vb2_cohort_run_source_fits on the same files
    res, src = vb.run_cohort_files(prefix, piles, num_pc=2, find_source=True, refit_source=True)
    fit, S = src["fit"], src["score"]
    assert all(r["status"] == 0 for r in res)
    assert rows == [_fit_row(fit[i], outs, i) for i in range(n)]
    for i, f in enumerate(fit):
        assert f["candidate"] == int(np.nanargmax(S[i])) and f["llr"] == S[i, f["candidate"]]
        assert (f["status"] == 0) == (f["llr"] > 0)
        assert f["freelk1"] == res[i]["llk1"]
        if f["status"] == 0:
            assert f["delta_lk"] == (-f["lk1_given"]) - (-f["freelk1"])
        else:
            assert f["status"] == _abi.VB2_SOURCE_FIT_NONE and np.isnan(f["alpha_given"]) and np.isnan(f["delta_lk"])
    # what the restatements give for this seed (tests/test_conditioned_cpu.py): sample 0 is refitted given sample 1 and the
    # conditioned maximum beats the anonymous one; sample 2's contaminant is nobody here: no refit
    want = cr.expected_refit(data, res, 0)                      # (data: the samples with the files' depth filter on)
    zero, two = fit[0], fit[2]
    print("sample 0: candidate %d, LLR %+.2f, FREEMIX %.6f, ALPHA_GIVEN %.6f (restatement %.6f), DELTA_LK %+.2f (restatement %+.2f)"
          % (zero["candidate"], zero["llr"], zero["freemix"], zero["alpha_given"], want["alpha_given"], zero["delta_lk"],
             want["delta_lk"]))
    print("sample 2: candidate %d, LLR %+.2f, status %d" % (two["candidate"], two["llr"], two["status"]))
    assert zero["candidate"] == 1 and want["candidate"] == 1 and zero["status"] == 0 and zero["delta_lk"] > 0
    assert abs(zero["alpha_given"] - want["alpha_given"]) <= 1e-4
    assert two["status"] == _abi.VB2_SOURCE_FIT_NONE and two["llr"] < 0


def test_a_sample_that_fails_its_sanity_check_is_absent_and_disturbs_nobody(tmp_path):
    data, prefix, piles, outs, lst = _write_cohort(tmp_path, extra_failing=True)
    n = len(piles)
    res, src = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, find_source=True, refit_source=True,
                                   sources_prefix=str(tmp_path / "run"))
    assert res[5]["status"] == _abi.VB2_ERR_SANITY and all(r["status"] == 0 for i, r in enumerate(res) if i != 5)
    fit = src["fit"]
    assert fit[5]["candidate"] == -1 and fit[5]["status"] == _abi.VB2_SOURCE_FIT_NONE
    rows = _read_fit(str(tmp_path / "run.SourceFit"))
    assert [r[0] for r in rows] == [o for i, o in enumerate(outs) if i != 5]
    assert outs[5] not in [r[1] for r in rows]
    good = [p for i, p in enumerate(piles) if i != 5]
    res7, src7 = vb.run_cohort_files(prefix, good, num_pc=2, find_source=True, refit_source=True)
    keep = [i for i in range(n) if i != 5]
    for a, i in zip(src7["fit"], keep):
        b = dict(fit[i])
        b["candidate"] = keep.index(b["candidate"])
        assert {k: v for k, v in a.items() if v == v} == {k: v for k, v in b.items() if v == v}, (i, a, b)
