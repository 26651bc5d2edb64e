"""The derivative math of vb2_llk_derivs_batch, restated in numpy (tests/deriv_ref.py), against
central finite differences of the oracle's LLK; and the new entry's place in the C-ABI.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from oracle.bridge import oracle_data

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _finite_differences(od, k, x, h_pc=1e-5, h_a=1e-6):
    """Central differences of the oracle's +LLK in (pc1, pc2, alpha), Richardson-extrapolated: gradient and Hessian.
    (An allele frequency moves by < 1e-3: no clamp is crossed -- _check asserts the margin.)"""
    n = 2 * k + 1
    h = np.array([h_pc] * (2 * k) + [h_a])

    def f(v):
        return od.llk(v[:k], v[k:2 * k], v[2 * k])

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


def _check(d, pc1, pc2, alpha, skip_pc=False):
    k = d.num_pc
    assert deriv_ref.af_margin(d, pc1, pc2) > 1e-3     # no allele frequency within the differences' reach of a clamp
    od = oracle_data(d)
    llk, grad, hess = deriv_ref.derivs(d, pc1, pc2, alpha)
    want = od.llk(pc1, pc2, alpha)
    assert abs(llk - want) <= 1e-11 * abs(want), (llk, want)
    x = np.concatenate([pc1, pc2, [alpha]])
    fg, fh = _finite_differences(od, k, x)
    sel = slice(2 * k, 2 * k + 1) if skip_pc else slice(0, 2 * k + 1)
    g_err = np.max(np.abs(grad[sel] - fg[sel])) / np.max(np.abs(fg[sel]))
    h_err = np.max(np.abs(hess[sel, sel] - fh[sel, sel])) / np.max(np.abs(fh[sel, sel]))
    assert g_err <= 1e-6, (g_err, grad, fg)
    assert h_err <= 1e-4, (h_err, hess, fh)
    if skip_pc:
        assert np.all(grad[:2 * k] == 0) and np.all(hess[:2 * k] == 0)
    return grad, hess


def _point(k, seed, scale=1e-4, alpha=0.1):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, k), rng.normal(0, scale, k), alpha


def test_restatement_on_the_golden_hapmap_panel():
    prefix = os.path.join(GOLDEN, "hapmap", "hapmap_3.3.b37.dat")
    d = vb.PileupData.from_files(prefix, os.path.join(GOLDEN, "expected", "result.Pileup"), 2, disable_sanity=True)
    pc1, pc2, a = _point(2, 3, scale=1e-3, alpha=0.02)
    _check(d, pc1, pc2, a)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_restatement_on_synthetic_samples(k):
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=11 + k)
    for alpha in (0.03, 0.3):
        pc1, pc2, _ = _point(k, k, alpha=alpha)
        _check(d, pc1, pc2, alpha)


def test_restatement_with_clamped_allele_frequencies():
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=5)
    # AF below 0 and above 1 at every point near this one, with panel rows that are not 0: clamped (h:187-188), so the
    # derivative rule -- 0 there -- is what the PC entries see
    rng = np.random.default_rng(2)
    d.means[:100] = -0.05
    d.means[100:200] = 2.05
    d.ud[:200] = rng.normal(0, 1e-2, (200, 2))
    pc1, pc2, a = _point(2, 9, alpha=0.05)
    _check(d, pc1, pc2, a)
    v = deriv_ref.marker_terms(deriv_ref.Counts(d), pc1, pc2, a)
    c = deriv_ref.Counts(d)
    clamped = c.idx < 200
    assert clamped.any() and np.all(v[[1, 2, 4, 5, 6, 7, 8]][:, clamped] == 0)


def test_restatement_with_known_allele_frequencies():
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=6)
    d.known_af = np.clip(d.means / 2.0, 0.01, 0.99)
    pc1, pc2, a = _point(2, 4, alpha=0.07)
    _check(d, pc1, pc2, a, skip_pc=True)


def test_restatement_with_the_sanity_filter():
    d = vb.synth.with_sanity_stats(vb.synth.make_pileup(2000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=8))
    c = deriv_ref.Counts(d)
    assert len(c.idx) < int((np.diff(d.read_off) > 0).sum())     # the filter drops markers
    pc1, pc2, a = _point(2, 6, alpha=0.2)
    _check(d, pc1, pc2, a)


def test_derivs_entry_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "vb2_abi.h")) as fh:
        header = fh.read()
    m = re.search(r"int vb2_llk_derivs_batch\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 8
    assert "vb2_llk_derivs_batch" in _abi.SYMBOLS
    assert hasattr(_abi.lib(), "vb2_llk_derivs_batch")
    assert _abi.lib().vb2_abi_version() == 7


@pytest.mark.parametrize("shape", [(3000, 30, 4, {}), (800, 650, 2, {}), (1500, 30, 2, dict(q_lo=0, q_hi=93)),
                                   (1500, 30, 2, dict(missing_frac=0.3))])
def test_restatement_in_80_bits_agrees_with_float64(shape):
    """The same code in np.longdouble and in float64: outputs of the precision asked for (no silent drop to double), the
    LLK to 1e-14, every entry to (1e-12 + 1e-15 / min(alpha, 1 - alpha)) of its condition sum -- double rounding, times
    the cancellation inside a marker (G1' W: terms of order 1 that cancel to order alpha) that S_e does not count."""
    assert np.finfo(np.longdouble).eps < 2e-19              # the x87 80-bit format: 64 bits of mantissa
    M, depth, k, kw = shape
    d = vb.synth.make_pileup(M, mean_depth=depth, num_pc=k, alpha_true=0.05, seed=44, **kw)
    c64, c80 = deriv_ref.Counts(d), deriv_ref.Counts(d, np.longdouble)
    assert c80.N.dtype == np.longdouble and c80.ud.dtype == np.longdouble and c64.N.dtype == np.float64
    rng = np.random.default_rng(4)
    for a in (1e-6, 0.03, 0.3, 0.5, 0.97):
        pc1, pc2 = rng.normal(0, 0.01, k), rng.normal(0, 0.01, k)
        for c, T in ((c64, np.float64), (c80, np.longdouble)):
            out = deriv_ref.derivs_cond(c, pc1, pc2, a)
            assert all(np.asarray(x).dtype == np.dtype(T) for x in out)
            assert deriv_ref.marker_terms(c, pc1, pc2, a).dtype == np.dtype(T)
        ref = deriv_ref.reference(c64, c80, pc1, pc2, a)
        assert abs(float(ref["l64"] - ref["l80"])) <= 1e-14 * abs(float(ref["l80"]))
        bound = 1e-12 + 1e-15 / min(a, 1 - a)
        for name, (dev, dev64, tol) in deriv_ref.block_devs(ref, ref["g64"], ref["h64"]).items():
            assert dev == dev64 <= bound, (name, a, dev64, bound)
            assert tol == max(32 * dev64, 1e-13)
        # a condition sum is never below the entry it belongs to
        assert np.all(ref["sg"] >= np.abs(ref["g80"]) * (1 - 1e-15)) and np.all(ref["sh"] >= np.abs(ref["h80"]) * (1 - 1e-15))


def test_condition_sums_at_alpha_zero_and_one():
    """At alpha = 0 nothing depends on pc1 (at alpha = 1: on pc2): those entries are 0 up to rounding, S_e with them, and
    the reference measures those blocks in the sums taken inside the markers -- which are never below S_e."""
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=10)
    c64, c80 = deriv_ref.Counts(d), deriv_ref.Counts(d, np.longdouble)
    pc1, pc2 = np.array([0.01, -0.02]), np.array([0.03, 0.01])
    for a, dead in ((0.0, slice(0, k)), (1.0, slice(k, 2 * k))):
        ref = deriv_ref.reference(c64, c80, pc1, pc2, a)
        _, _, _, sg, sh = deriv_ref.derivs_cond(c80, pc1, pc2, a)
        gi, hi = deriv_ref.derivs_cond(c80, pc1, pc2, a, inner=True)
        assert np.all(gi[:2 * k] >= sg[:2 * k]) and np.all(hi[:2 * k, :2 * k] >= sh[:2 * k, :2 * k])
        assert np.max(np.abs(ref["g80"][dead])) <= 1e-12 * np.max(gi[dead])          # 0 up to rounding
        assert np.array_equal(ref["sg"][dead], gi[dead]) and np.array_equal(ref["sh"][dead, dead], hi[dead, dead])
        for name, (_, dev64, _) in deriv_ref.block_devs(ref, ref["g64"], ref["h64"], alpha_entries=False).items():
            assert dev64 <= 1e-12, (name, a, dev64)
    gi, hi = deriv_ref.derivs_cond(c80, pc1, pc2, 0.3, inner=True)
    _, _, _, sg, sh = deriv_ref.derivs_cond(c80, pc1, pc2, 0.3)
    assert np.all(gi >= sg) and np.all(hi >= sh)
