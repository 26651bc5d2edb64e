"""The derivatives of the paired likelihood and the interval of a paired refit without a GPU: the
numpy restatement (tests/paired_deriv_ref.py) against differences of the section 16 restatement and against its own
identities; the library's host side (interval_at's options, the lock-step driver) through vb2_paired_intervals_lockstep
with the restatement as the evaluator; the additions to the ABI; the kernels' resources from the code-object notes."""
import os
import re
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402
import paired_deriv_ref as pdr  # noqa: E402
import paired_ref as pr  # noqa: E402
import source_ref as sr  # noqa: E402
from deriv_ref import Counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vb2_paired_derivs", "vb2_paired_derivs_sets", "vb2_paired_interval", "vb2_paired_intervals_lockstep"]


def test_new_symbols_and_the_abi_is_still_7():
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.vb2_abi_version() == 7
    assert re.search(r"#define VB2_ABI_VERSION 7\b", header)
    assert hasattr(vb.Paired, "derivatives") and hasattr(vb.Paired, "interval") and hasattr(vb.Paired, "interval_sets")
    assert hasattr(vb, "paired_intervals_with_evaluator")


def test_cli_refuses_pair_interval_without_matched_normal(tmp_path):
    """Before any file is read or any device call is made: no panel, pileup or list file exists."""
    import subprocess
    exe = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
    cmd = [exe, "--PairInterval", "--SVDPrefix", str(tmp_path / "nopanel"), "--Reference", "x.fa", "--Output", str(tmp_path / "o"),
           "--PileupList", str(tmp_path / "list.txt")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert p.returncode != 0 and "FATAL ERROR" in p.stderr
    assert "--PairInterval needs --MatchedNormal" in p.stderr and "cannot open --PileupList" not in p.stderr
    assert not (tmp_path / "o.PairCI").exists()
    # ... and with it, --MatchedNormal's own refusals stand
    p = subprocess.run(cmd + ["--MatchedNormal", str(tmp_path / "pairs.txt"), "--FixAlpha", "0.01"], capture_output=True, text=True,
                       timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert p.returncode != 0 and "--MatchedNormal cannot be combined with --FixAlpha" in p.stderr


# ---- the restatement ----

@pytest.fixture(scope="module")
def pair():
    """300 markers x 20, k = 2: a tumour contaminated at 5 % by individual 1, its normal's posterior as the device would hold
    it, and hypotheses of every kind."""
    panel = sr.make_panel(300, 2, seed=3)
    G = sr.draw_individuals(panel, 3, seed=4)
    tumour = sr.make_sample(panel, G[0], G[1], 20, 0.05, 50)
    normal = sr.make_sample(panel, G[0], G[2], 20, 0.0, 51)
    q = pr.normal_q(normal)
    third = q.copy()
    third[::3] = pr.LEFT_OUT
    mixed = third.copy()
    mixed[1::3] = 0
    pi1 = np.random.default_rng(7).dirichlet(np.ones(3), 300).astype(np.float32)
    pi1[::5] = 0
    hyps = dict(zero=pr.hypothesis(300), q=pr.hypothesis(300, pi2=q), mixed=pr.hypothesis(300, pi2=mixed),
                both=pr.hypothesis(300, pi1=pi1, pi2=mixed), rule=pr.normal_rule(q, 0.99))
    return tumour, q, hyps


def _richardson(f, x, h):
    """Central differences of f in the coordinates of x with steps h, Richardson-extrapolated: gradient and Hessian
    (tests/test_derivs_cpu.py's scheme)."""
    n = len(x)

    def unit(i, s):
        e = np.zeros(n)
        e[i] = s
        return e

    def g1(i, s):
        return (f(x + unit(i, s)) - f(x - unit(i, s))) / (2 * s)

    def h1(i, j, s, t):
        ei, ej = unit(i, s), unit(j, t)
        return (f(x + ei + ej) - f(x + ei - ej) - f(x - ei + ej) + f(x - ei - ej)) / (4 * s * t)
    grad = np.array([(4 * g1(i, h[i]) - g1(i, 2 * h[i])) / 3 for i in range(n)])
    hh = 3 * h
    hess = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            hess[i, j] = hess[j, i] = (4 * h1(i, j, hh[i], hh[j]) - h1(i, j, 2 * hh[i], 2 * hh[j])) / 3
    return grad, hess


@pytest.mark.parametrize("name", ["zero", "q", "mixed", "both", "rule"])
def test_restatement_against_differences_of_the_paired_likelihood(pair, name):
    """Gradient 1e-6 and Hessian 1e-4 of the largest entry (tests/test_derivs_cpu.py's tolerances), against differences of
    paired_ref.llk taken in 80-bit floats."""
    tumour, _, hyps = pair
    hyp = hyps[name]
    k = 2
    c64, c80 = Counts(tumour), Counts(tumour, np.longdouble)
    rng = np.random.default_rng(11)
    for alpha in (0.03, 0.3):
        pc1, pc2 = rng.normal(0, 1e-4, k), rng.normal(0, 1e-4, k)
        assert deriv_ref.af_margin(tumour, pc1, pc2) > 1e-3
        llk, grad, hess = pdr.derivs(c64, hyp, pc1, pc2, alpha)
        want = pr.llk(c80, hyp, pc1, pc2, alpha)
        assert abs(llk - want) <= 1e-12 * abs(want)
        x = np.concatenate([pc1, pc2, [alpha]])
        fg, fh = _richardson(lambda v: float(pr.llk(c80, hyp, v[:k], v[k:2 * k], v[2 * k])), x,
                             np.array([1e-5] * (2 * k) + [1e-6]))
        assert np.max(np.abs(grad - fg)) <= 1e-6 * np.max(np.abs(fg)), (name, grad, fg)
        assert np.max(np.abs(hess - fh)) <= 1e-4 * np.max(np.abs(fh)), (name, hess, fh)


def test_the_two_precisions_agree(pair):
    """The float64 restatement against the 80-bit one, per block, in units of the sums of the absolute values of every term
    inside and across the markers (derivs_cond's inner sums: what bounds the rounding error of ANY float64 evaluation --
    the condition sums S_e are themselves noise where a block cancels inside the marker, near alpha = 0 and 1).  1e-12: a
    few hundred operations per entry at 1.1e-16 each is 1e-13; a wrong or missing term shows at 1e-3 or more."""
    tumour, _, hyps = pair
    c64, c80 = Counts(tumour), Counts(tumour, np.longdouble)
    rng = np.random.default_rng(12)
    for name, hyp in hyps.items():
        for alpha in (0.0, 1e-6, 0.03, 0.5, 1.0):
            pc1, pc2 = rng.normal(0, 0.02, 2), rng.normal(0, 0.02, 2)
            ref = pdr.reference(c64, c80, hyp, pc1, pc2, alpha)
            assert ref["l80"].dtype == np.longdouble
            assert abs(ref["l64"] - ref["l80"]) <= 1e-13 * abs(ref["l80"])
            gi, hi = pdr.derivs_cond(c80, hyp, pc1, pc2, alpha, inner=True)
            unit = dict(ref, sg=gi, sh=hi)
            for block, (_, dev64, _) in deriv_ref.block_devs(unit, ref["g64"], ref["h64"], alpha not in (0.0, 1.0)).items():
                assert dev64 <= 1e-12, (name, alpha, block, dev64)


def test_all_zero_priors_are_the_anonymous_derivatives(pair):
    tumour, _, hyps = pair
    rng = np.random.default_rng(13)
    for T in (np.float64, np.longdouble):
        c = Counts(tumour, T)
        for alpha in (0.0, 0.03, 0.5, 1.0):
            pc1, pc2 = rng.normal(0, 0.02, 2), rng.normal(0, 0.02, 2)
            want = deriv_ref.derivs_cond(c, pc1, pc2, alpha)
            for hyp in (hyps["zero"], None):
                got = pdr.derivs_cond(c, hyp, pc1, pc2, alpha)
                for x, y in zip(got, want):
                    assert x.dtype == np.dtype(T) and np.array_equal(x, y)


def test_one_hot_on_the_same_genotype_on_both_sides_has_no_alpha(pair):
    """Identity 5's derivative: L_m = W[g][g], which alpha does not enter; nor do the PCs."""
    tumour, _, _ = pair
    c = Counts(tumour)
    eye = np.eye(3, dtype=np.float32)
    for g in range(3):
        side = np.tile(eye[g], (300, 1))
        llk, grad, hess = pdr.derivs(c, pr.hypothesis(300, pi1=side, pi2=side), [0.01, -0.02], [0.02, 0.01], 0.2)
        assert llk != 0 and np.all(grad == 0) and np.all(hess == 0)


def test_the_mirror_identity_on_derivatives(pair):
    """LLK(pc1, pc2, alpha | a, b) = LLK(pc2, pc1, 1 - alpha | b, a): the pc1 and pc2 blocks change places and every entry
    odd in alpha changes sign.  alpha with an exact complement; 1e-10 of the largest entry of the gradient / the Hessian,
    the derivative tests' figure between two orders of the same float64 arithmetic."""
    tumour, q, _ = pair
    k = 2
    c = Counts(tumour)
    a = np.random.default_rng(6).dirichlet(np.ones(3), 300).astype(np.float32)
    a[::5] = 0                                                # fallback markers on the a side ...
    b = q.copy()
    b[::4] = 0                                                # ... and on the b side
    b[1::7] = pr.LEFT_OUT
    out = b[:, 0] < 0
    ha, hb = pr.hypothesis(300, pi1=a, pi2=b), pr.hypothesis(300, pi1=np.where(out[:, None], np.float32(0), b), pi2=a)
    hb[out, 3:] = pr.LEFT_OUT
    rng = np.random.default_rng(14)
    perm = np.r_[k:2 * k, 0:k, 2 * k]
    sign = np.r_[np.ones(2 * k), -1.0]
    for alpha in (0.25, 0.5, 0.75, 0.125):
        pc1, pc2 = rng.normal(0, 0.02, k), rng.normal(0, 0.02, k)
        l, g, h = pdr.derivs(c, ha, pc1, pc2, alpha)
        lm, gm, hm = pdr.derivs(c, hb, pc2, pc1, 1.0 - alpha)
        assert l != 0 and abs(l - lm) <= 1e-12 * abs(l)
        assert np.max(np.abs(g - sign * gm[perm])) <= 1e-10 * np.max(np.abs(g))
        assert np.max(np.abs(h - np.outer(sign, sign) * hm[np.ix_(perm, perm)])) <= 1e-10 * np.max(np.abs(h))
        assert np.max(np.abs(g[:k])) > 0 and np.max(np.abs(g[k:2 * k])) > 0      # (fallback markers on both sides)


def test_a_left_out_marker_changes_nothing_outside_its_own_term(pair):
    tumour, _, hyps = pair
    c = Counts(tumour)
    base = hyps["both"]
    full = pdr.marker_terms(c, base, [0.01, 0.0], [0.0, 0.02], 0.1)
    walked = np.nonzero(~(base[c.idx, 3] < 0))[0]
    for i in walked[[0, 7, len(walked) - 1]]:
        hyp = base.copy()
        hyp[c.idx[i], 3:] = pr.LEFT_OUT
        got = pdr.marker_terms(c, hyp, [0.01, 0.0], [0.0, 0.02], 0.1)
        assert np.all(got[:, i] == 0) and np.any(full[:, i] != 0)
        keep = np.arange(len(c.idx)) != i
        assert np.array_equal(got[:, keep], full[:, keep])


# ---- the library's host side over the restatement ----

def _same(a, b):
    return (a == b) or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def _check_interval(ci, ref, est, lo_hi, steps):
    assert ci["status"] == 0 and ci["pos_def"] == ref["pos_def"] and ci["num_free"] == ref["num_free"]
    assert ci["freemix"] == est["alpha"] and ci["alpha_free"]
    assert [r["param"] for r in ci["rows"]] == ["FREEMIX"] + [n for n, _, _ in ref["rows"][1:]]
    for row, (_, v, se) in zip(ci["rows"], ref["rows"]):
        assert row["estimate"] == v
        assert abs(row["stderr"] - se) <= 1e-8 * ref["cond"] * se, (row, se)
    assert abs(ci["freemix_se"] - ref["alpha_se"]) <= 1e-8 * ref["cond"] * ref["alpha_se"]
    assert 0.0 <= ci["lo"] <= est["alpha"] <= ci["hi"] <= 1.0
    for got, want in zip((ci["lo"], ci["hi"]), lo_hi):
        assert abs(got - want) <= 1e-5 * max(want, 1e-3), (got, want)
    assert steps == ci["num_launch"] and ci["num_profile"] >= 3


def test_pc2_held_the_paired_refits_interval(pair):
    tumour, _, hyps = pair
    c = Counts(tumour)
    pc2 = np.array([0.004, -0.003])
    (est,), _ = pr.search([c], [hyps["rule"]], pc2[None])
    assert est["status"] == 0
    ev = pdr.Evaluator([c], [hyps["rule"]])
    (ci,), steps = vb.paired_intervals_with_evaluator(ev, 2, [est], pc2[None])
    for _, _, p2, _ in ev.calls:
        assert np.all(p2 == pc2)
    ref = pdr.se_ref(c, hyps["rule"], est, pc2)
    assert ref["num_free"] == 3 and [n for n, _, _ in ref["rows"][1:]] == ["ContaminatingSample.PC1", "ContaminatingSample.PC2"]
    _check_interval(ci, ref, est, pdr.interval_ref(c, hyps["rule"], est, pc2), steps)
    for row in ci["rows"][1:]:
        assert row["method"] == "wald" and abs(row["lo"] - (row["estimate"] - pdr.Z975 * row["stderr"])) <= 1e-15


def test_pc1_held_the_interval_of_a_refit_given_the_contaminant(pair):
    """The side the device does not serve: identity 1 makes a conditioned hypothesis a pair hypothesis with pi2 all zero, and
    the same driver holds pc1."""
    tumour, q, _ = pair
    k = 2
    c = Counts(tumour)
    hyp = pr.hypothesis(300, pi1=q)
    pc1 = np.array([0.002, 0.001])
    (est,) = vb.conditioned_with_evaluator(pr.Evaluator([c], [hyp]), 1, k, pc1[None])
    assert est["status"] == 0
    ev = pdr.Evaluator([c], [hyp])
    (ci,), steps = vb.paired_intervals_with_evaluator(ev, k, [est], pc1[None], held="pc1")
    for _, p1, _, _ in ev.calls:
        assert np.all(p1 == pc1)
    assert ci["status"] == 0 and ci["num_free"] == 3 and ci["pos_def"] and steps == ci["num_launch"]
    assert [r["param"] for r in ci["rows"]] == ["FREEMIX", "IntendedSample.PC1", "IntendedSample.PC2"]
    assert [r["estimate"] for r in ci["rows"][1:]] == list(est["pc2"][:k])
    a = est["alpha"]
    _, g, H = pdr.derivs(c, hyp, pc1, est["pc2"][:k], a)
    s = a * (1 - a)
    J = np.zeros((2 * k + 1, k + 1))
    J[k:2 * k, :k] = np.eye(k)
    J[2 * k, k] = s
    A = -(J.T @ H @ J)
    A[k, k] -= g[2 * k] * s * (1 - 2 * a)
    se = np.sqrt(np.diag(np.linalg.inv(A)))
    cond = np.linalg.cond(A)
    got = [r["stderr"] for r in ci["rows"][1:]] + [ci["freemix_se"] / s]
    assert np.max(np.abs(np.array(got) / se - 1)) <= 1e-8 * cond
    assert 0.0 <= ci["lo"] <= a <= ci["hi"] <= 1.0 and ci["freemix"] == a


def test_fix_pc_and_known_allele_frequencies_leave_alpha_alone(pair):
    tumour, _, hyps = pair
    pc2 = np.array([0.004, -0.003])
    fix = [0.01, -0.01]
    c = Counts(tumour)
    (est,), _ = pr.search([c], [hyps["rule"]], pc2[None], fix_pc=fix)
    (ci,), steps = vb.paired_intervals_with_evaluator(pdr.Evaluator([c], [hyps["rule"]]), 2, [est], pc2[None], fix_pc=fix)
    ref = pdr.se_ref(c, hyps["rule"], est, pc2, fix_pc=True)
    assert ref["num_free"] == 1 and len(ci["rows"]) == 1 and list(est["pc"][:2]) == fix
    _check_interval(ci, ref, est, pdr.interval_ref(c, hyps["rule"], est, pc2, fix_pc=True), steps)

    import copy
    known = copy.deepcopy(tumour)
    known.known_af = np.clip(known.means / 2.0, 0.01, 0.99)
    ck = Counts(known)
    (est,), _ = pr.search([ck], [hyps["rule"]], pc2[None], known_af=True)
    (ci,), steps = vb.paired_intervals_with_evaluator(pdr.Evaluator([ck], [hyps["rule"]]), 2, [est], pc2[None], known_af=[True])
    ref = pdr.se_ref(ck, hyps["rule"], est, pc2)
    assert ref["num_free"] == 1 and len(ci["rows"]) == 1
    _check_interval(ci, ref, est, pdr.interval_ref(ck, hyps["rule"], est, pc2), steps)


def test_a_fixed_alpha_is_refused(pair):
    tumour, _, hyps = pair
    est = dict(alpha=0.1, llk1=1.0, pc=np.zeros(2), pc2=np.zeros(2))
    ev = pdr.Evaluator([Counts(tumour)], [hyps["rule"]])
    with pytest.raises(_abi.Vb2Error) as err:
        vb.paired_intervals_with_evaluator(ev, 2, [est], np.zeros((1, 2)), fix_alpha=0.1)
    assert err.value.code == _abi.VB2_ERR_INVALID and "fixed alpha" in str(err.value) and not ev.calls


def test_the_default_options_are_the_anonymous_interval_bit_for_bit():
    """held = none: vb2_intervals_lockstep's fields on the same evaluator, the fold and the index swap included."""
    k = 2
    d = vb.synth.make_pileup(1500, mean_depth=25, num_pc=k, alpha_true=0.1, seed=21)
    c = Counts(d)
    from oracle.bridge import oracle_data
    est = oracle_data(d).optimize()
    twin = dict(est, alpha=1 - est["alpha"], pc=est["pc2"], pc2=est["pc"])      # alpha >= 0.5: the fold and the swap

    def ev(num_point, pc1, pc2, alpha):
        out = [deriv_ref.derivs(c, pc1[p], pc2[p], alpha[p]) for p in range(len(alpha))]
        return [np.array([o[j] for o in out], dtype=np.float64) for j in range(3)]
    for model in ({}, dict(within_ancestry=True), dict(fix_pc=[0.0, 0.0])):
        for e in (est, twin):
            (want,), s0 = vb.intervals_with_evaluator(ev, k, [e], **model)
            (got,), s1 = vb.paired_intervals_with_evaluator(ev, k, [e], None, held=None, **model)
            assert s0 == s1 and set(got) == set(want)
            for key in want:
                if key == "rows":
                    assert len(got["rows"]) == len(want["rows"])
                    for x, y in zip(got["rows"], want["rows"]):
                        assert all(_same(x[f], y[f]) for f in y), (x, y)
                else:
                    assert _same(got[key], want[key]), (key, got[key], want[key])
            assert got["freemix"] <= 0.5


@pytest.fixture(scope="module")
def stranger():
    """Section 16's alpha ~ 0.975 case: a stranger's genotypes as the normal of pair_case's tumour."""
    panel, shifted_t, plain_t, normal, other = pr.pair_case()
    c = Counts(plain_t)
    hyp = pr.normal_rule(pr.normal_q(other), 0.99)
    pc2 = np.zeros(2)
    (est,), _ = pr.search([c], [hyp], pc2[None])
    return c, hyp, pc2, est


def test_an_estimate_above_one_half_stays_unfolded_and_on_its_side(stranger):
    c, hyp, pc2, est = stranger
    assert est["status"] == 0 and est["alpha"] > 0.9
    (ci,), steps = vb.paired_intervals_with_evaluator(pdr.Evaluator([c], [hyp]), 2, [est], pc2[None])
    assert ci["status"] == 0 and ci["freemix"] == est["alpha"] and ci["rows"][0]["estimate"] == est["alpha"]
    assert 0.5 < ci["lo"] <= est["alpha"] <= ci["hi"] <= 1.0
    assert ci["rows"][0]["lo"] == ci["lo"] and ci["rows"][0]["hi"] == ci["hi"]
    lo, hi = pdr.interval_ref(c, hyp, est, pc2)
    assert abs(ci["lo"] - lo) <= 1e-5 * lo and abs(ci["hi"] - hi) <= 1e-5 * hi
    # the rows keep the contaminant's PCs as fitted: no index swap
    assert [r["param"] for r in ci["rows"][1:]] == ["ContaminatingSample.PC1", "ContaminatingSample.PC2"]
    assert [r["estimate"] for r in ci["rows"][1:]] == list(est["pc"][:2])


# ---- the kernels' resources ----

# vgpr_count of the derivative kernels' instantiations <false> (run words), <true> (probability domain) on the parent commit
PARENT_VGPRS = {"llk_derivs_marker_kernel<false>": 142, "llk_derivs_marker_kernel<true>": 156,
                "llk_derivs_marker_multi_kernel<false>": 142, "llk_derivs_marker_multi_kernel<true>": 154,
                "llk_derivs_reduce_kernel": 16, "llk_derivs_reduce_multi_kernel": 16}
# ... and of the prior-aware ones as first built: 166 is on the last granule (168) with three waves per SIMD
PAIR_VGPRS = {"llk_pair_derivs_marker_kernel<false>": 142, "llk_pair_derivs_marker_kernel<true>": 166,
              "llk_pair_derivs_marker_multi_kernel<false>": 142, "llk_pair_derivs_marker_multi_kernel<true>": 164}


def test_derivative_kernels_resources():
    import test_kernel_resources_cpu as res
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = res.all_kernel_notes(res.LIB)
    short = lambda name: re.search(r"(\w+_kernel(<[^>]*>)?)\(", name).group(1)
    mine = {short(k[1]): (k[0], v) for k, v in notes.items() if re.search(r"llk_(pair_)?derivs_\w+_kernel", k[1])}
    for name, (obj, v) in sorted(mine.items()):
        print("%4d VGPRs %5d B scratch  %s  [%s]" % (v["vgpr_count"], v["private_segment_fixed_size"], name, obj))
    assert set(mine) == set(PARENT_VGPRS) | set(PAIR_VGPRS), sorted(mine)
    assert len({obj for obj, _ in mine.values()}) == 1
    for name, (_, v) in mine.items():
        assert v["private_segment_fixed_size"] == 0, name
        assert v["vgpr_count"] == dict(PARENT_VGPRS, **PAIR_VGPRS)[name], (name, v["vgpr_count"])
