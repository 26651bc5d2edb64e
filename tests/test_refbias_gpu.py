"""The reference bias on the MI355X (refbias_kernels.hip, refbias.cpp): vb2_refbias_eval against the
np.longdouble restatement (tests/refbias_ref.py) in both layouts, the KSEL-compiled and the general --NumPC, a known-AF
column, missing and filtered markers, the wide alphabet, a sample that takes run words whatever the switch; the beta = 0.5
row against vb2_llk_eval_batch; the bits of a point whatever the step holds; the deep sample a probability-domain context
refuses; the lock-step refits and the whole estimate of beta against the same procedure on the float64 restatement through
the host seam; the command line with and without --RefBias.

The largest |kernel - restatement| / |restatement| over every evaluation case of this module, per layout, is printed at the
module's end (pytest -s); the checks fail above LLK_RTOL = 1e-12, the rule and allowance of test_conditioned_gpu._close.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refbias_ref as rr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")

LLK_RTOL = 1e-12                  # the project's evaluation tolerance (tests/test_gpu_parity.py)
BETAS = [0.25, 0.5, 0.58, 0.75]
ALPHAS = [0.0, 0.03, 0.5, 1.0, 1e-6]
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


def _points(k, n, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, (n, k)), rng.normal(0, scale, (n, k)), np.array([ALPHAS[i % len(ALPHAS)] for i in range(n)])


def _check_eval(d, ctx, rb, betas, steps, seed, label):
    """Every point of `steps` (lists of points per row) against the 80-bit restatement; the beta = 0.5 row against
    vb2_llk_eval_batch as well."""
    layout = ctx.info()["layout"]
    c80 = Counts(d, np.longdouble)
    for s, num_point in enumerate(steps):
        P = int(np.sum(num_point))
        pc1, pc2, alpha = _points(d.num_pc, P, seed + s)
        got = rb.eval(num_point, pc1, pc2, alpha)
        assert got.shape == (P,)
        p = 0
        for r, n in enumerate(num_point):
            for _ in range(n):
                where = "%s beta=%g alpha=%g" % (label, betas[r], alpha[p])
                _close(got[p], rr.llk(c80, betas[r], pc1[p], pc2[p], alpha[p]), layout, where)
                if betas[r] == 0.5:
                    _close(got[p], ctx.llk(pc1[p], pc2[p], alpha[p])[0], layout, where + " vs ctx.llk")
                p += 1


# points per row: every row meets every alpha in the first step; rows sit the others out
STEPS = [[8, 8, 8, 8], [3, 0, 5, 1], [0, 1, 0, 0]]


@pytest.mark.parametrize("M, k, pd", [(1, 2, 1), (17, 1, 0), (17, 4, 1), (300, 4, 0), (300, 1, 1), (3000, 2, 0), (3000, 2, 1)])
def test_eval_matches_the_restatement(M, k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=k, alpha_true=0.05, seed=100 + M + k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        with vb.RefBias(ctx, BETAS) as rb:
            info = rb.info()
            assert info["num_row"] == 4 and info["num_marker"] == M and info["device_bytes"] > 0
            _check_eval(d, ctx, rb, BETAS, STEPS, seed=M, label="%dx%d k=%d" % (M, 30, k))
            # the bias moves the likelihood: the rows are not each other's values
            z = np.zeros((4, k))
            v = rb.eval([1, 1, 1, 1], z, z, np.full(4, 0.03))
            assert M < 17 or len(set(v.tolist())) == 4


@pytest.mark.parametrize("pd", [0, 1])
def test_eval_with_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(300, mean_depth=25, num_pc=2, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, 300), 0.0, 1.0)
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, BETAS) as rb:
        assert ctx.info()["layout"] == pd
        _check_eval(d, ctx, rb, BETAS, STEPS[:2], seed=5, label="known AF")


@pytest.mark.parametrize("pd", [0, 1])
def test_eval_with_the_wide_alphabet(pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(300, mean_depth=30, num_pc=2, alpha_true=0.05, seed=41, q_lo=2, q_hi=60)
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, BETAS) as rb:
        assert ctx.info()["layout"] == pd and ctx.info()["num_code"] > 100
        _check_eval(d, ctx, rb, BETAS, STEPS[:2], seed=9, label="q 2..60")


def test_eval_of_a_sample_that_takes_run_words_whatever_the_switch(tunable):
    """Three markers deeper than the probability-domain bound (about 900 reads) among 300 ordinary ones, and quality-0 reads.
    The deep markers are homozygous, both ways.  A heterozygous site of 1 000 reads has a likelihood of about 2^-1000 at beta
    = 0.5 and below 2^-1022, the smallest normal double, at 0.58 (500 x (log2 0.58 + log2 0.42) = -1 019 before the priors): the
    reference's doubles, the float64 restatement and the kernel alike lose it gradually there -- the float64 restatement is
    7e-11 nats off the 80-bit one at such a marker, and at 0.25 and 0.75 it underflows to 0 and is left out by h:310 --, so
    1e-12 against 80 bits cannot be asked of any double arithmetic at such a site, with or without a bias (at 0.5: beyond
    about 1 020 reads)."""
    tunable("pd", 1)
    a = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=31, q_lo=0, q_hi=40)
    b = vb.synth.make_pileup(3, mean_depth=1000, num_pc=2, alpha_true=0.05, seed=34)
    cb = Counts(b)
    ref, alt = cb.N[:, :len(cb.quals)].sum(axis=1), cb.N[:, len(cb.quals):].sum(axis=1)
    assert np.all(ref + alt > 950) and np.all(np.minimum(ref, alt) < 100) and ref.max() > 950 and alt.max() > 950
    d = vb.PileupData(2, np.concatenate([a.ud, b.ud]), np.concatenate([a.means, b.means]),
                      np.concatenate([a.read_off, a.read_off[-1] + b.read_off[1:]]), np.concatenate([a.bases, b.bases]),
                      np.concatenate([a.quals, b.quals]), np.concatenate([a.alt_base, b.alt_base]), None, a.avg_depth, 0.0, True)
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, BETAS) as rb:
        assert ctx.info()["layout"] == 0
        _check_eval(d, ctx, rb, BETAS, STEPS[:2], seed=6, label="deep + q0")


def test_eval_with_missing_and_depth_filtered_markers():
    d = vb.synth.make_pileup(3000, mean_depth=20, num_pc=2, alpha_true=0.05, seed=21, missing_frac=0.15)
    d = vb.synth.with_sanity_stats(d)
    depth = np.diff(d.read_off)
    gone = (depth == 0) | (depth < d.avg_depth - 3 * d.sd_depth) | (depth > d.avg_depth + 3 * d.sd_depth)
    assert (depth == 0).sum() > 300 and gone.sum() > (depth == 0).sum() and not d.sanity_disabled
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, BETAS) as rb:
        _check_eval(d, ctx, rb, BETAS, STEPS[:2], seed=7, label="missing + filtered")


@pytest.fixture(scope="module")
def sample_3000():
    return vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=77)


@pytest.mark.parametrize("pd", [0, 1])
def test_a_step_of_49_points_and_the_bits_of_a_point(sample_3000, pd, tunable):
    """7 rows x 7 points cross the launch boundary (48 points); one row's point gives the same bits alone, as the last of the
    49, beside three other rows and on a second call."""
    tunable("pd", pd)
    d = sample_3000
    betas = [0.25, 0.5, 0.58, 0.75, 0.3125, 0.44, 0.66]
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, betas) as rb:
        assert ctx.info()["layout"] == pd
        before = rb.info()
        _check_eval(d, ctx, rb, betas, [[7] * 7], seed=49, label="49 points")
        after = rb.info()
        assert after["num_step"] == before["num_step"] + 1 and after["num_launch"] == before["num_launch"] + 2
        pc1, pc2, alpha = _points(2, 49, 49)
        alpha[-1] = 0.03
        full = rb.eval([7] * 7, pc1, pc2, alpha)
        again = rb.eval([7] * 7, pc1, pc2, alpha)
        assert full.tobytes() == again.tobytes()
        alone = rb.eval([0, 0, 0, 0, 0, 0, 1], pc1[-1:], pc2[-1:], alpha[-1:])
        assert alone.tobytes() == full[-1:].tobytes()
        mixed = rb.eval([3, 0, 8, 0, 1, 0, 2], np.concatenate([pc1[:12], pc1[-1:], pc1[-1:]]),
                        np.concatenate([pc2[:12], pc2[-1:], pc2[-1:]]), np.concatenate([alpha[:12], alpha[-1:], alpha[-1:]]))
        assert mixed[-1:].tobytes() == alone.tobytes() and mixed[-2:-1].tobytes() == alone.tobytes()
        # the same point under another row is another value
        other = rb.eval([0, 0, 0, 0, 0, 1, 0], pc1[-1:], pc2[-1:], alpha[-1:])
        assert other[0] != alone[0]
        # an alpha outside [0, 1] leaves every marker out, as in vb2_llk_eval_batch
        out = rb.eval([1, 0, 0, 0, 1, 0, 0], pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        want = ctx.llk(pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        assert out.tobytes() == want.tobytes() or np.array_equal(out, want)


def test_argument_errors(sample_3000):
    d = sample_3000
    with vb.LikelihoodContext(d) as ctx:
        for bad in ([0.5, 0.2499], [0.7501], [float("nan")]):
            with pytest.raises(_abi.Vb2Error, match="outside"):
                vb.RefBias(ctx, bad)
        with pytest.raises(_abi.Vb2Error):
            vb.RefBias(ctx, np.zeros(0))
        with vb.RefBias(ctx, [0.5, 0.6]) as rb:
            with pytest.raises(_abi.Vb2Error):
                rb.eval([9, 0], np.zeros((9, 2)), np.zeros((9, 2)), np.full(9, 0.1))
            assert rb.eval([0, 0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)).shape == (0,)
            with pytest.raises(_abi.Vb2Error, match="fixed alpha"):
                rb.optimize(fix_alpha=0.01)
        with pytest.raises(_abi.Vb2Error, match="fixed alpha"):
            vb.RefBias.fit(ctx, fix_alpha=0.01)


# ---- the deep sample ----

def test_a_deep_sample_is_refused_in_the_probability_domain_and_evaluated_in_run_words(tunable):
    """17 markers at depth 600: the (het, het) term may lie 2^-450 .. 2^-900 below 1 at beta = 0.5 -- the layout's own bound
    holds, the doubled one of a bias does not."""
    d = vb.synth.make_pileup(17, mean_depth=600, num_pc=2, alpha_true=0.05, seed=61)
    bound = rr.het_bound(d)
    print("deep sample: bound %.1f binary orders of magnitude" % bound)
    assert 450 < bound < 900
    tunable("pd", 1)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        with pytest.raises(_abi.Vb2Error, match="tunable pd = 0") as ei:
            vb.RefBias(ctx, BETAS)
        assert ei.value.code == _abi.VB2_ERR_INVALID
    tunable("pd", 0)
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, BETAS) as rb:
        assert ctx.info()["layout"] == 0
        _check_eval(d, ctx, rb, BETAS, STEPS[:2], seed=3, label="17 x 600")


# ---- refits ----

@pytest.fixture(scope="module")
def planted():
    """3 000 x 30, k = 2, alpha = 0.03, beta planted at 0.58 (refbias_ref.FIT_SEED), and the same with known AF."""
    return dict(target=rr.fit_sample(), target_af=rr.make_sample(3000, 30, 2, 0.03, 0.58, rr.FIT_SEED, known_af=True))


MODELS = {"default": ("target", dict()), "fix_pc": ("target", dict(fix_pc=[0.01, -0.02])), "known_af": ("target_af", dict())}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_refits_match_the_restatements_searches(planted, name):
    which, model = MODELS[name]
    d = planted[which]
    want = rr.search(Counts(d), BETAS, known_af=d.known_af is not None, **model)
    with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, BETAS) as rb:
        got = rb.optimize(**model)
        for r in range(4):
            g, w = got[r], want[r]
            print("%s beta %g: alpha %.9g (restatement %.9g), -llk1 %.12g (restatement %.12g), %d evaluations (%d)"
                  % (name, BETAS[r], g["alpha"], w["alpha"], -g["llk1"], -w["llk1"], g["num_eval"], w["num_eval"]))
            assert g["status"] == 0 and w["status"] == 0 and g["converged"]
            assert abs(g["alpha"] - w["alpha"]) <= 1e-4, (name, r, g["alpha"], w["alpha"])
            assert abs(g["llk1"] - w["llk1"]) <= 1e-6 * abs(w["llk1"]), (name, r, g["llk1"], w["llk1"])
            assert g["num_eval"] == w["num_eval"], (name, r, g["num_eval"], w["num_eval"])
            npt = [0] * 4
            npt[r] = 1
            at = rb.eval(npt, g["pc"][None], g["pc2"][None], [g["alpha"]])[0]
            assert abs(-at - g["llk1"]) <= LLK_RTOL * abs(g["llk1"]), (name, r, at, g["llk1"])
        # the planted bias explains the reads best, and the rows' maxima are ordered like their distance from it
        llk = [-g["llk1"] for g in got]
        assert llk[2] > llk[1] > llk[0] and llk[2] > llk[3]


def test_the_fit_on_the_device_is_the_restatements(tunable):
    """vb2_refbias_fit_ctx against vb2_refbias_lockstep over the float64 restatement, on 1 000 x 30 (the procedure is the
    same code; a third of the planted sample keeps the restatement's 28 searches to seconds).  The grid is the same values
    exactly as long as the searches order the profile alike.  Allowances: every llk1 1e-6 relative, the refit tests' own; the
    searches stop within about 1e-8 |llk| = 2e-4 nats of their maximum, so with second differences of about 0.03 nats at
    spacing 2^-10 and 0.5 at 2^-8 on this sample the vertex moves by less than 0.5 x 2^-10 x 4e-4 / 0.03 < 1e-5 and the
    standard error by less than 8e-4 / 0.5 / 2 < 0.1 %: 1e-4 and 1 % are given."""
    d = rr.make_sample(1000, 30, 2, 0.03, 0.58, rr.FIT_SEED + 100)
    want = vb.refbias_with_evaluator(rr.Evaluator(Counts(d)), 2)
    with vb.LikelihoodContext(d) as ctx:
        got = vb.RefBias.fit(ctx)
    print("device: beta %.6f SE %.6f LRT %.3f (%d steps); restatement: beta %.6f SE %.6f LRT %.3f (%d steps)"
          % (got["beta"], got["beta_se"], got["lrt"], got["num_step"], want["beta"], want["beta_se"], want["lrt"], want["num_step"]))
    assert got["status"] == 0 and len(got["pairs"]) == 28 and got["num_refit"] == 28 and got["num_round"] == 4
    assert [b for b, _ in got["pairs"][:27]] == [b for b, _ in want["pairs"][:27]]
    for (_, g), (_, w) in zip(got["pairs"], want["pairs"]):
        assert abs(g - w) <= 1e-6 * abs(w)
    assert abs(got["beta"] - want["beta"]) <= 1e-4
    assert abs(got["beta_se"] - want["beta_se"]) <= 0.01 * want["beta_se"]
    assert abs(got["lrt"] - want["lrt"]) <= 2e-6 * abs(want["llk1_bias"])
    assert got["at_bound"] == want["at_bound"] and got["num_step"] == want["num_step"]
    assert abs(got["alpha_bias"] - want["alpha_bias"]) <= 1e-4 and abs(got["alpha_at_half"] - want["alpha_at_half"]) <= 1e-4
    assert abs(got["beta"] - 0.58) <= 3 * got["beta_se"] and got["lrt"] > 3.84


# ---- end to end ----

HEADER = ["#SEQ_ID", "FREEMIX", "FREEMIX_BIAS", "REF_BIAS", "REF_BIAS_SE", "LRT", "FREELK1_BIAS", "FREELK1_HALF", "AT_BOUND"]


def _run_cli(prefix, out, extra):
    return subprocess.run([CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupFile", prefix + ".pileup", "--Output", out,
                           "--DisableSanityCheck"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_end_to_end_ref_bias(planted, tmp_path):
    d = planted["target"]
    prefix = vb.synth.write_files(d, str(tmp_path / "planted"))
    out = str(tmp_path / "run")
    plain = _run_cli(prefix, out, [])
    assert plain.returncode == 0, plain.stderr[-2000:]
    others = [out + ext for ext in (".selfSM", ".Ancestry")]
    before = [open(p, "rb").read() for p in others]
    assert not os.path.exists(out + ".RefBias")
    biased = _run_cli(prefix, out, ["--RefBias"])
    assert biased.returncode == 0, biased.stderr[-2000:]
    # stdout, .selfSM and .Ancestry: byte for byte what the run without the flag wrote
    assert biased.stdout == plain.stdout
    assert [open(p, "rb").read() for p in others] == before
    notices = [ln for ln in biased.stderr.decode().splitlines() if "REF_BIAS" in ln]
    assert len(notices) == 1 and notices[0].startswith("NOTICE - REF_BIAS "), notices
    assert b"REF_BIAS" not in plain.stderr and len(biased.stderr.splitlines()) == len(plain.stderr.splitlines()) + 1
    lines = open(out + ".RefBias").read().splitlines()
    assert len(lines) == 2 and lines[0].split("\t") == HEADER
    row = lines[1].split("\t")
    # the struct of vb2_run_refbias on the same files
    res = vb.run_files(prefix, prefix + ".pileup", None, num_pc=2, disable_sanity=True, ref_bias=True)
    f = res["ref_bias"]
    g = lambda x: "%g" % x
    selfsm = open(out + ".selfSM").read().splitlines()
    cols = dict(zip(selfsm[0].split("\t"), selfsm[1].split("\t")))
    assert row == [cols["#SEQ_ID"], cols["FREEMIX"], g(f["freemix_bias"]), g(f["beta"]), g(f["beta_se"]), g(f["lrt"]),
                   g(f["llk1_bias"]), g(f["llk1_at_half"]), "0"]
    assert row[1] == g(min(res["alpha"], 1 - res["alpha"]))
    print("planted 0.58 end to end: " + "  ".join("%s %s" % (h, v) for h, v in zip(HEADER, row)))
    assert f["status"] == 0 and abs(f["beta"] - 0.58) <= 3 * f["beta_se"] and f["lrt"] > 3.84 and len(f["pairs"]) == 28


def test_ref_bias_from_bam_input(golden_dir, tmp_path):
    """expected/result.Pileup turned into a BAM, as test_bam_gpu does: the file is written and its FREEMIX is .selfSM's."""
    from test_bam_gpu import _cli, _golden_bam
    bam, _ = _golden_bam(golden_dir, str(tmp_path), os.path.join("expected", "result.Pileup"))
    out = str(tmp_path / "r")
    _cli(golden_dir, out, ["--BamFile", bam, "--RefBias"])
    lines = open(out + ".RefBias").read().splitlines()
    assert len(lines) == 2 and lines[0].split("\t") == HEADER
    selfsm = open(out + ".selfSM").read().splitlines()
    cols = dict(zip(selfsm[0].split("\t"), selfsm[1].split("\t")))
    row = lines[1].split("\t")
    assert row[0] == cols["#SEQ_ID"] and row[1] == cols["FREEMIX"]
    assert open(out + ".selfSM").read() == open(os.path.join(golden_dir, "expected", "result.selfSM")).read()
