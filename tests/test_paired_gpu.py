"""The likelihood given priors on both components on the MI355X (marker_sum_kernels.hip: PairTerm; paired.cpp; DESIGN.md
section 16): vb2_paired_eval against the np.longdouble restatement (tests/paired_ref.py) in both layouts, the KSEL-compiled
and the general --NumPC, a known-AF column, every kind of hypothesis row and of step; identities 1 to 4 against
Conditioned.eval, ctx.llk, Replicates.eval and the mirror; the bits of a point whatever the step holds; create_from_set
against create under the same rule; the lock-step refits against the same searches on the float64 restatement through the
host seam under three models; two sets on two contexts in one call.

The largest |kernel - restatement| / |restatement| over every evaluation case of this module, per layout, is printed at the
module's end (pytest -s); the checks fail above LLK_RTOL = 1e-12.  Measured on an MI355X:

    layout 0 (run words)           4.1e-16  (17 markers x 30, k = 2, panel marker 7 alone left out)
    layout 1 (probability domain)  4.2e-16  (17 x 30, k = 4, left-out, fallback and walked markers mixed, alpha = 0.03)

Refits (3 000 x 30, k = 2): alpha, llk1 and the evaluation counts are the float64 restatement's under all three models
(97 / 182, 24 / 30, 18 / 30 evaluations for the true normal / a stranger).  End to end (seed 42): tumour 0 FREEMIX 0.054223,
ALPHA_PAIRED 0.030109 over 2 035 markers (restatement 0.030109, 2 035; planted 0.03); tumour 2 FREEMIX 0.046145,
ALPHA_PAIRED 0.046854 over 2 059 markers (planted 0.05).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paired_ref as pr  # noqa: E402
import source_ref as sr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")

LLK_RTOL = 1e-12                  # the project's evaluation tolerance (tests/test_gpu_parity.py)
ALPHAS = [0.0, 1e-6, 0.03, 0.25, 0.5, 1.0]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for layout in sorted(_WORST):
        print("\nlayout %d: worst |kernel - restatement| / |restatement| = %.3g (%s)" % ((layout,) + _WORST[layout]))


def _close(got, want, layout, label, record=True):
    want = float(want)
    rel = abs(got - want) / abs(want) if want != 0 else abs(got)
    if record and rel > _WORST.get(layout, (-1.0, ""))[0]:
        _WORST[layout] = (rel, label)
    assert rel <= LLK_RTOL, (label, got, want, rel)


def _other_q(d, seed):
    """Another sample's genotype posterior as the device would hold it: float32 [M, 3], zeros where it counts nothing."""
    o = vb.synth.make_pileup(d.num_marker, mean_depth=15, num_pc=d.num_pc, alpha_true=0.01, seed=seed, missing_frac=0.1)
    return pr.normal_q(o)


ALL_OUT = 7


def _hyp_rows(d, seed):
    """[10, M, 6]: 0 both sides all zero; 1-3 pi2 one-hot on each genotype; 4 another sample's q as pi2; 5 that row with
    every third marker left out; 6 that row with another third all zero as well (walked, left-out and fallback markers side
    by side); 7 every marker left out; 8 q with exact zeros for two genotypes on a marker whose reads contradict the third;
    9 both pi1 and pi2 given."""
    M = d.num_marker
    q = _other_q(d, seed)
    eye = np.eye(3, dtype=np.float32)
    third = q.copy()
    third[::3] = pr.LEFT_OUT
    mixed = third.copy()
    mixed[1::3] = 0
    contra = q.copy()
    c64 = Counts(d)
    z = np.zeros(d.num_pc)
    m = sr.marginals(c64, z, z, 0.05)
    depth = np.diff(d.read_off)[c64.idx]
    ok = m["live"] & (depth <= 100)
    assert ok.any()
    worst = int(np.argmin(np.where(ok, m["q"].min(axis=1), np.inf)))
    contra[c64.idx[worst]] = eye[int(np.argmin(m["q"][worst]))]
    pi1 = np.random.default_rng(seed).dirichlet(np.ones(3), M).astype(np.float32)
    pi1[::5] = 0                                               # (some fall back on the pi1 side too)
    rows = [pr.hypothesis(M)] + [pr.hypothesis(M, pi2=np.tile(eye[g], (M, 1))) for g in range(3)]
    rows += [pr.hypothesis(M, pi2=x) for x in (q, third, mixed, np.tile(pr.LEFT_OUT, (M, 1)), contra)]
    rows += [pr.hypothesis(M, pi1=pi1, pi2=q)]
    return np.stack(rows)


def _points(k, n, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, (n, k)), rng.normal(0, scale, (n, k)), np.array([ALPHAS[i % len(ALPHAS)] for i in range(n)])


def _check_eval(d, ctx, pair, rows, steps, seed, label):
    """Every point of `steps` (lists of points per hypothesis) against the 80-bit restatement."""
    layout = ctx.info()["layout"]
    c80 = Counts(d, np.longdouble)
    for s, num_point in enumerate(steps):
        P = int(np.sum(num_point))
        pc1, pc2, alpha = _points(d.num_pc, P, seed + s)
        got = pair.eval(num_point, pc1, pc2, alpha)
        assert got.shape == (P,)
        p = 0
        for h, n in enumerate(num_point):
            for _ in range(n):
                where = "%s hypothesis %d alpha=%g" % (label, h, alpha[p])
                _close(got[p], pr.llk(c80, rows[h], pc1[p], pc2[p], alpha[p]), layout, where)
                if h == 0:                                   # identity 2: the anonymous model
                    _close(got[p], ctx.llk(pc1[p], pc2[p], alpha[p])[0], layout, where + " vs ctx.llk", record=False)
                if h == ALL_OUT:
                    assert got[p] == 0.0
                p += 1


# points per hypothesis: 0 (the hypothesis sits the step out), 1, 4, 5 and 8; every row meets every alpha in some step
STEPS = [[8, 1, 4, 8, 4, 1, 0, 5, 8, 4], [5, 5, 5, 0, 5, 8, 5, 1, 5, 8], [1, 0, 0, 1, 0, 0, 1, 0, 1, 1]]


@pytest.mark.parametrize("M, k, pd", [(1, 2, 1), (17, 1, 0), (17, 4, 1), (300, 4, 0), (300, 1, 1), (3000, 2, 0), (3000, 2, 1)])
def test_eval_matches_the_restatement(M, k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=k, alpha_true=0.05, seed=100 + M + k)
    rows = _hyp_rows(d, M + 1)
    c64 = Counts(d)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        with vb.Paired(ctx, rows) as pair:
            info = pair.info()
            assert info["num_hyp"] == 10 and info["num_marker"] == M and info["device_bytes"] > 0
            assert info["given"].tolist() == [pr.given_count(c64, r) for r in rows] and info["given"][ALL_OUT] == 0
            _check_eval(d, ctx, pair, rows, STEPS, seed=M, label="%dx%d k=%d" % (M, 30, k))


@pytest.mark.parametrize("pd", [0, 1])
def test_eval_with_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(300, mean_depth=25, num_pc=2, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, 300), 0.0, 1.0)
    rows = _hyp_rows(d, 3)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["layout"] == pd
        _check_eval(d, ctx, pair, rows, STEPS[:2], seed=5, label="known AF")


def test_eval_of_a_sample_that_takes_run_words_whatever_the_switch(tunable):
    """Three markers deeper than the probability-domain bound (about 900 reads) among 300 ordinary ones, and quality-0 reads."""
    tunable("pd", 1)
    a = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=31, q_lo=0, q_hi=40)
    b = vb.synth.make_pileup(3, mean_depth=1000, num_pc=2, alpha_true=0.05, seed=32)
    d = vb.PileupData(2, np.concatenate([a.ud, b.ud]), np.concatenate([a.means, b.means]),
                      np.concatenate([a.read_off, a.read_off[-1] + b.read_off[1:]]), np.concatenate([a.bases, b.bases]),
                      np.concatenate([a.quals, b.quals]), np.concatenate([a.alt_base, b.alt_base]), None, a.avg_depth, 0.0, True)
    rows = _hyp_rows(d, 9)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["layout"] == 0
        _check_eval(d, ctx, pair, rows, STEPS[:2], seed=6, label="deep + q0")


def test_eval_with_missing_and_depth_filtered_markers():
    d = vb.synth.make_pileup(3000, mean_depth=20, num_pc=2, alpha_true=0.05, seed=21, missing_frac=0.15)
    d = vb.synth.with_sanity_stats(d)
    depth = np.diff(d.read_off)
    gone = (depth == 0) | (depth < d.avg_depth - 3 * d.sd_depth) | (depth > d.avg_depth + 3 * d.sd_depth)
    assert (depth == 0).sum() > 300 and gone.sum() > (depth == 0).sum() and not d.sanity_disabled
    rows = _hyp_rows(d, 4)
    c64 = Counts(d)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert pair.info()["given"].tolist() == [pr.given_count(c64, r) for r in rows]
        _check_eval(d, ctx, pair, rows, STEPS[:2], seed=7, label="missing + filtered")


@pytest.mark.parametrize("M, pd", [(17, 0), (17, 1), (33, 1)])
def test_every_single_marker_left_out_in_turn(M, pd, tunable):
    """Hypothesis m leaves out panel marker m alone: whatever the context's order, one of them is the first marker of a
    16-marker tile, one its last, one the lone marker of the last tile."""
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=2, alpha_true=0.05, seed=40 + M)
    q = _other_q(d, 2)
    rows = np.stack([pr.hypothesis(M, pi2=q) for _ in range(M)])
    for m in range(M):
        rows[m, m, 3:] = pr.LEFT_OUT
    c80 = Counts(d, np.longdouble)
    pc1, pc2, alpha = _points(2, M, 3)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        got = pair.eval([1] * M, pc1, pc2, alpha)
        assert pair.info()["given"].tolist() == [len(c80.idx) - 1] * M
        for m in range(M):
            _close(got[m], pr.llk(c80, rows[m], pc1[m], pc2[m], alpha[m]), pd, "%d markers, marker %d left out" % (M, m))


@pytest.fixture(scope="module")
def sample_3000():
    return vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=77)


@pytest.mark.parametrize("pd", [0, 1])
def test_identities_on_the_device(sample_3000, pd, tunable):
    tunable("pd", pd)
    d = sample_3000
    M = d.num_marker
    q = _other_q(d, 5)
    third = q.copy()
    third[::3] = 0
    w = (np.random.default_rng(9).random(M) < 0.6).astype(np.uint8)
    subset = pr.hypothesis(M)
    subset[w == 0, 3:] = pr.LEFT_OUT
    a = np.random.default_rng(10).dirichlet(np.ones(3), M).astype(np.float32)
    b = q.copy()
    b[::4] = 0
    rows = np.stack([pr.hypothesis(M, pi1=q), pr.hypothesis(M, pi1=third), pr.hypothesis(M), subset,
                     pr.hypothesis(M, pi1=a, pi2=b), pr.hypothesis(M, pi1=b, pi2=a)])
    pc1, pc2, alpha = _points(2, 6, 11)
    rep6 = lambda x: np.concatenate([x] * 6)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        got = pair.eval([6] * 6, rep6(pc1), rep6(pc2), rep6(alpha)).reshape(6, 6)
        with vb.Conditioned(ctx, np.stack([q, third])) as cond:              # 1: pi2 all zero
            want = cond.eval([6, 6], rep6(pc1)[:12], rep6(pc2)[:12], rep6(alpha)[:12]).reshape(2, 6)
        for h in range(2):
            for p in range(6):
                _close(got[h, p], want[h, p], pd, "identity 1", record=False)
        want = ctx.llk(pc1, pc2, alpha)                                       # 2: both all zero
        for p in range(6):
            _close(got[2, p], want[p], pd, "identity 2", record=False)
        with vb.Replicates(ctx, w[None]) as rep:                               # 3: left out = weight 0
            want = rep.eval([6], pc1, pc2, alpha)
        for p in range(6):
            _close(got[3, p], want[p], pd, "identity 3", record=False)
        # 4: the mirror, at alphas whose complement is exact
        al = np.array([0.25, 0.5, 0.75, 0.125, 0.0, 1.0])
        left = pair.eval([0, 0, 0, 0, 6, 0], pc1, pc2, al)
        right = pair.eval([0, 0, 0, 0, 0, 6], pc2, pc1, 1.0 - al)
        for p in range(6):
            assert left[p] != 0.0
            _close(left[p], right[p], pd, "identity 4", record=False)
    # 5: one-hot on the same genotype on both sides: the context's diagonal constants, whatever alpha is
    eye = np.eye(3, dtype=np.float32)
    same = np.stack([pr.hypothesis(M, pi1=np.tile(eye[g], (M, 1)), pi2=np.tile(eye[g], (M, 1))) for g in range(3)])
    c80 = Counts(d, np.longdouble)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, same) as pair:
        got = pair.eval([6] * 3, np.concatenate([pc1] * 3), np.concatenate([pc2] * 3), np.concatenate([alpha] * 3)).reshape(3, 6)
        for g in range(3):
            want = pr.diagonal_constants(c80, g)
            for p in range(6):
                _close(got[g, p], want, pd, "identity 5")


@pytest.mark.parametrize("pd", [0, 1])
def test_a_step_of_49_points_and_the_bits_of_a_point(sample_3000, pd, tunable):
    """10 hypotheses, 49 points cross the launch boundary (48 points); one hypothesis's point gives the same bits alone, as
    the last of the 49, beside three other hypotheses and on a second call."""
    tunable("pd", pd)
    d = sample_3000
    rows = _hyp_rows(d, 12)
    npt = [5] * 9 + [4]
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["layout"] == pd
        before = pair.info()
        _check_eval(d, ctx, pair, rows, [npt], seed=49, label="49 points")
        after = pair.info()
        assert after["num_step"] == before["num_step"] + 1 and after["num_launch"] == before["num_launch"] + 2
        pc1, pc2, alpha = _points(2, 49, 49)
        alpha[-1] = 0.03
        full = pair.eval(npt, pc1, pc2, alpha)
        again = pair.eval(npt, pc1, pc2, alpha)
        assert full.tobytes() == again.tobytes()
        alone = pair.eval([0] * 9 + [1], pc1[-1:], pc2[-1:], alpha[-1:])
        assert alone.tobytes() == full[-1:].tobytes()
        # the same point behind three other hypotheses' points, and twice in one step
        mixed = pair.eval([3, 0, 8, 0, 1, 0, 0, 0, 0, 2], np.concatenate([pc1[:12], pc1[-1:], pc1[-1:]]),
                          np.concatenate([pc2[:12], pc2[-1:], pc2[-1:]]), np.concatenate([alpha[:12], alpha[-1:], alpha[-1:]]))
        assert mixed[-1:].tobytes() == alone.tobytes() and mixed[-2:-1].tobytes() == alone.tobytes()
        # an alpha outside [0, 1] leaves every marker out, as in vb2_llk_eval_batch
        out = pair.eval([1, 0, 0, 0, 1, 0, 0, 0, 0, 0], pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        want = ctx.llk(pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        assert out.tobytes() == want.tobytes() or np.array_equal(out, want)


def test_argument_errors(sample_3000):
    d = sample_3000
    with vb.LikelihoodContext(d) as ctx:
        with pytest.raises(ValueError):
            vb.Paired(ctx, np.ones((2, d.num_marker, 3)))
        with pytest.raises(_abi.Vb2Error):
            vb.Paired(ctx, np.ones((0, d.num_marker, 6)))
        with vb.Paired(ctx, np.ones((2, d.num_marker, 6))) as pair:
            with pytest.raises(_abi.Vb2Error):
                pair.eval([9, 0], np.zeros((9, 2)), np.zeros((9, 2)), np.full(9, 0.1))
            assert pair.eval([0, 0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)).shape == (0,)
            with pytest.raises(_abi.Vb2Error, match="fixed alpha"):
                pair.optimize(np.zeros(2), fix_alpha=0.01)


# ---- a tumour, its normal and a stranger ----

@pytest.fixture(scope="module")
def cohort():
    """3 000 x 30, k = 2: a tumour contaminated at 5 % by an outsider; its normal and another individual's; the same tumour
    with known AF."""
    panel = sr.make_panel(3000, 2, seed=21)
    G = sr.draw_individuals(panel, 4, seed=22)
    tumour = sr.make_sample(panel, G[0], G[1], 30, 0.05, 200)
    tumour_af = sr.make_sample(panel, G[0], G[1], 30, 0.05, 200, known_af=True)
    normals = [sr.make_sample(panel, G[i], G[3], 30, 0.0, 201 + i) for i in (0, 2)]
    qs = [pr.normal_q(n) for n in normals]
    rows = np.stack([pr.normal_rule(x, 0.99) for x in qs])              # the true normal, a stranger
    return dict(tumour=tumour, tumour_af=tumour_af, normals=normals, rows=rows, fixed=np.array([0.004, -0.003]))


@pytest.mark.parametrize("tau", [0.0, 0.99, 1.0])
def test_create_from_set_gives_the_bits_of_create(cohort, tau):
    tumour, normals = cohort["tumour"], cohort["normals"]
    est = dict(pc=np.array([0.002, -0.001]), pc2=np.array([0.001, 0.003]), alpha=0.002)
    c64 = Counts(tumour)
    with vb.LikelihoodContext(tumour) as ctx, vb.SourceSet(tumour.num_marker, 2) as ss:
        host = []
        for n in normals:
            with vb.LikelihoodContext(n) as c:
                assert ss.add(c, est) == len(host)
                host.append(c.marginals(est["pc"], est["pc2"], est["alpha"])[1].astype(np.float32))
        assert all(h.any() for h in host)
        rule = np.stack([pr.normal_rule(host[1], tau), pr.normal_rule(host[0], tau)])
        pc1, pc2, alpha = _points(2, 10, 3)
        with vb.Paired(ctx, source_set=ss, normals=[1, 0], hom_min=tau) as a, vb.Paired(ctx, rule) as b:
            assert a.num_hyp == 2
            given = [pr.given_count(c64, r) for r in rule]
            print("tau = %g: given %r of %d" % (tau, given, len(c64.idx)))
            assert a.info()["given"].tolist() == given and b.info()["given"].tolist() == given
            assert 0 < given[0] < len(c64.idx) or tau == 0.0
            got, want = a.eval([5, 5], pc1, pc2, alpha), b.eval([5, 5], pc1, pc2, alpha)
            assert got.tobytes() == want.tobytes() and got[0] != got[5]
        with pytest.raises(_abi.Vb2Error):
            vb.Paired(ctx, source_set=ss, normals=[2], hom_min=tau)
        with pytest.raises(_abi.Vb2Error):
            vb.Paired(ctx, source_set=ss, normals=[0], hom_min=1.5)


MODELS = {"default": ("tumour", dict()), "fix_pc": ("tumour", dict(fix_pc=[0.01, -0.02])), "known_af": ("tumour_af", dict())}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_refits_match_the_restatements_searches(cohort, name):
    which, model = MODELS[name]
    d, rows, fixed = cohort[which], cohort["rows"], cohort["fixed"]
    c64 = Counts(d)
    nothing = np.zeros_like(rows[0])
    nothing[:, 3:] = pr.LEFT_OUT
    hyps = [rows[0], rows[1], nothing]
    want, _ = pr.search([c64] * 2, hyps[:2], np.tile(fixed, (2, 1)), known_af=d.known_af is not None, **model)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, np.stack(hyps)) as pair:
        got = pair.optimize(fixed, **model)
        assert got[2]["status"] == _abi.VB2_ERR_INVALID                       # no walked marker: fails alone
        assert pair.eval([0, 0, 1], fixed[None], fixed[None], [0.1])[0] == 0.0
        for h in range(2):
            g, w = got[h], want[h]
            print("%s hypothesis %d: alpha %.9g (restatement %.9g), -llk1 %.12g (restatement %.12g), -llk0 %.12g, %d evaluations (%d)"
                  % (name, h, g["alpha"], w["alpha"], -g["llk1"], -w["llk1"], -g["llk0"], g["num_eval"], w["num_eval"]))
            assert g["status"] == 0 and w["status"] == 0 and g["converged"]
            # equal to the printed digits (%g, as <Output>.PairFit prints them), and the same number of evaluations
            assert "%g" % g["alpha"] == "%g" % w["alpha"], (name, h, g["alpha"], w["alpha"])
            assert "%g" % g["llk1"] == "%g" % w["llk1"], (name, h, g["llk1"], w["llk1"])
            assert g["num_eval"] == w["num_eval"]
            npt = [0] * 3
            npt[h] = 1
            at = pair.eval(npt, g["pc"][None], fixed[None], [g["alpha"]])[0]
            assert abs(-at - g["llk1"]) <= LLK_RTOL * abs(g["llk1"]), (name, h, at, g["llk1"])
        # given its true normal the tumour's fit finds the planted contamination
        assert abs(got[0]["alpha"] - 0.05) < 0.01


def test_two_sets_on_two_contexts_in_one_call(cohort):
    a, b, rows, fixed = cohort["tumour"], cohort["normals"][1], cohort["rows"], cohort["fixed"]
    other = np.array([-0.002, 0.006])
    with vb.LikelihoodContext(a) as ca, vb.LikelihoodContext(b) as cb, vb.Paired(ca, rows) as sa, vb.Paired(cb, rows[1:]) as sb:
        alone = [sa.optimize(fixed), sb.optimize(other)]
        both = vb.Paired.optimize_sets([sa, sb], [fixed, other])
        for s in range(2):
            for g, w in zip(both[s], alone[s]):
                assert g["status"] == 0 and g["alpha"] == w["alpha"] and g["llk1"] == w["llk1"] and g["llk0"] == w["llk0"]
                assert np.array_equal(g["pc"], w["pc"])
        assert both[0][0]["alpha"] != both[1][0]["alpha"]


# ---- end to end: --PileupList --MatchedNormal ----

HEADER = ["#TUMOUR", "NORMAL", "NORMAL_FREEMIX", "MARKERS", "FREEMIX", "FREELK1", "ALPHA_PAIRED", "LK1_PAIRED", "LK0_PAIRED"]


def _write_cohort(tmp, extra_failing=False):
    from verifybamid_amd import synth
    panel, data = pr.pair_cohort()
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
        d = data[3]
        off = d.read_off.copy()
        off[301:] = off[300]
        p = str(tmp / "bad.pileup")
        synth.write_pileup_text(p, chrs, poss, panel["ref"], off, d.bases, d.quals)
        piles.append(p)
        outs.append(str(tmp / "bad"))
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        for p, o in zip(piles, outs):
            f.write("%s\t%s\n" % (p, o))
    return data, prefix, piles, outs, lst


def _run_cli(prefix, lst, out, pairs_file, stream, extra=()):
    env = dict(os.environ)
    if not stream:
        env["VB2_COHORT_STREAM"] = "0"
    args = [CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupList", lst, "--Output", out]
    if pairs_file:
        args += ["--MatchedNormal", pairs_file] + list(extra)
    return subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def _read_fit(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == HEADER
    return [ln.split("\t") for ln in lines[1:]]


def _fit_row(f, piles):
    g = lambda x: "%g" % x
    row = [piles[f["tumour"]], piles[f["normal"]]]
    if f["status"] == _abi.VB2_PAIR_FIT_NONE:
        return row + ["NA"] * 7
    row += [g(f["normal_freemix"]), str(f["markers"]), g(f["freemix"]), g(f["freelk1"])]
    return row + ([g(f["alpha_paired"]), g(f["lk1_paired"]), g(f["lk0_paired"])] if f["status"] == 0 else ["NA"] * 3)


@pytest.mark.parametrize("stream", [True, False])
def test_end_to_end_matched_normal(tmp_path, stream, tunable):
    tunable("cohort_stream", 1 if stream else 0)               # (the in-process run below, like the command line's)
    data, prefix, piles, outs, lst = _write_cohort(tmp_path)
    pairs_file = str(tmp_path / "pairs.txt")
    with open(pairs_file, "w") as f:
        for t, n in pr.COHORT_PAIRS:
            f.write("%s\t%s\n" % (piles[t], piles[n]))
    plain = _run_cli(prefix, lst, str(tmp_path / "run"), None, stream)
    assert plain.returncode == 0, plain.stderr[-2000:]
    others = [o + ext for o in outs for ext in (".selfSM", ".Ancestry")]
    before = [open(p, "rb").read() for p in others]
    assert not os.path.exists(str(tmp_path / "run.PairFit"))
    paired = _run_cli(prefix, lst, str(tmp_path / "run"), pairs_file, stream)
    assert paired.returncode == 0, paired.stderr[-2000:]
    # stdout, .selfSM and .Ancestry: byte for byte what the run without the flag wrote
    assert paired.stdout == plain.stdout
    assert [open(p, "rb").read() for p in others] == before
    assert b"the contexts of 2 tumours stayed on the device for the refit" in paired.stderr
    rows = _read_fit(str(tmp_path / "run.PairFit"))
    # the fits array of vb2_cohort_run_paired on the same files
    res, fits = vb.run_cohort_files(prefix, piles, num_pc=2, matched_normal=pr.COHORT_PAIRS)
    assert all(r["status"] == 0 for r in res)
    assert rows == [_fit_row(f, piles) for f in fits]
    gap = {}
    for f, (t, n) in zip(fits, pr.COHORT_PAIRS):
        assert (f["tumour"], f["normal"], f["status"]) == (t, n, 0)
        assert f["freelk1"] == res[t]["llk1"] and f["freemix"] == min(res[t]["alpha"], 1 - res[t]["alpha"])
        assert f["normal_freemix"] == min(res[n]["alpha"], 1 - res[n]["alpha"])
        # what the restatements give from the run's own anonymous fits (tests/test_paired_cpu.py confirms the seed)
        want = pr.expected_pair(data, res, t, n)                  # (data: the samples with the files' depth filter on)
        print("tumour %d: FREEMIX %.6f, ALPHA_PAIRED %.6f (restatement %.6f), MARKERS %d (restatement %d), planted %.3f"
              % (t, f["freemix"], f["alpha_paired"], want["alpha_paired"], f["markers"], want["markers"], pr.COHORT_PLANTED[t]))
        assert f["markers"] == want["markers"]
        assert "%g" % f["alpha_paired"] == "%g" % want["alpha_paired"]
        assert "%g" % f["lk1_paired"] == "%g" % want["lk1_paired"] and "%g" % f["lk0_paired"] == "%g" % want["lk0_paired"]
        gap[t] = (abs(f["freemix"] - pr.COHORT_PLANTED[t]), abs(f["alpha_paired"] - pr.COHORT_PLANTED[t]))
    assert gap[0][1] < gap[0][0]                               # the tumour with the imbalance: closer given its normal
    # --NormalHomMin 0 keeps every marker the normal counts: more markers, and the imbalance is back in the estimate
    loose = _run_cli(prefix, lst, str(tmp_path / "loose"), pairs_file, stream, extra=["--NormalHomMin", "0"])
    assert loose.returncode == 0, loose.stderr[-2000:]
    lrows = _read_fit(str(tmp_path / "loose.PairFit"))
    assert int(lrows[0][3]) > int(rows[0][3]) and lrows[0][:2] == rows[0][:2]


def test_a_normal_that_fails_its_sanity_check_gives_an_na_row_and_disturbs_nobody(tmp_path):
    data, prefix, piles, outs, lst = _write_cohort(tmp_path, extra_failing=True)
    bad = len(piles) - 1
    res, fits = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, matched_normal=[(0, 1), (2, bad)],
                                    sources_prefix=str(tmp_path / "run"))
    assert res[bad]["status"] == _abi.VB2_ERR_SANITY and all(r["status"] == 0 for i, r in enumerate(res) if i != bad)
    assert fits[1]["status"] == _abi.VB2_PAIR_FIT_NONE and np.isnan(fits[1]["alpha_paired"]) and fits[0]["status"] == 0
    rows = _read_fit(str(tmp_path / "run.PairFit"))
    assert rows[1] == [piles[2], piles[bad]] + ["NA"] * 7
    # ... and the other pair's row is what the cohort without the failing sample gives
    res6, fits6 = vb.run_cohort_files(prefix, piles[:bad], num_pc=2, matched_normal=[(0, 1), (2, 3)])
    assert {k: v for k, v in fits6[0].items()} == {k: v for k, v in fits[0].items()}
    assert rows[0] == _fit_row(fits6[0], piles)
    # a tumour that fails: the same
    res, fits = vb.run_cohort_files(prefix, piles, num_pc=2, matched_normal=[(bad, 3), (0, 1)])
    assert fits[0]["status"] == _abi.VB2_PAIR_FIT_NONE and fits[1] == fits6[0]
