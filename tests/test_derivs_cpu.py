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
