"""Numpy restatement of what vb2_ctx_interval defines, on the restatement of the derivatives
(tests/deriv_ref.py, float64): the standard errors of the model's free parameters and the profile log-likelihood of
FREEMIX.  It shares no code with csrc/interval.cpp.

A model is the keyword set of LikelihoodContext.optimize: within_ancestry, fix_pc, fix_alpha; known allele frequencies
are a property of the sample.  An estimate is the dict optimize returns (alpha, llk1, pc, pc2): its PCs are REPORTED
ones -- when the model is heterogeneous and alpha >= 0.5 the reference swaps indices 0 and 1 of the two samples' PCs
before it prints them, so the point the search ended at (and the likelihood is evaluated at) has them swapped back.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402

Z975 = 1.959963984540054
HALF_CHI2 = 1.9207294103470620


def flags(d, within_ancestry=False, fix_pc=None, fix_alpha=None):
    kaf = d.known_af is not None
    heter = (not within_ancestry) and not kaf
    pc_fixed = fix_pc is not None or kaf
    alpha_fixed = (fix_pc is None) and fix_alpha is not None and not kaf
    return heter, pc_fixed, alpha_fixed


def search_point(d, est, **model):
    """(pc1, pc2, swapped): the estimate's PCs as the likelihood takes them."""
    k = d.num_pc
    heter, _, _ = flags(d, **model)
    pc1, pc2 = np.array(est["pc"], dtype=np.float64)[:k].copy(), np.array(est["pc2"], dtype=np.float64)[:k].copy()
    swapped = bool(heter and est["alpha"] >= 0.5)
    if swapped:
        for j in range(min(k, 2)):
            pc1[j], pc2[j] = pc2[j], pc1[j]
    return pc1, pc2, swapped


def _free_columns(k, heter, pc_fixed):
    """Columns of the map from the free PC coordinates to (pc1, pc2, alpha), and which (sample, index) each one is."""
    n = 2 * k + 1
    eye = np.eye(n)
    if heter:
        cols = [eye[:, i] for i in range(k)] + ([] if pc_fixed else [eye[:, k + i] for i in range(k)])
        what = [(1, i) for i in range(k)] + ([] if pc_fixed else [(2, i) for i in range(k)])
    else:
        cols = [] if pc_fixed else [eye[:, i] + eye[:, k + i] for i in range(k)]
        what = [] if pc_fixed else [(0, i) for i in range(k)]
    return cols, what


def se_ref(d, est, counts=None, **model):
    """Standard errors at an estimate: a dict with pos_def, cond (of A), se per free coordinate, freemix_se and the .CI
    rows [(name, estimate, se)] -- FREEMIX first, then the PCs as .Ancestry prints them, each SE at the row that holds
    its coordinate's value.  A = -J' H J in the free coordinates, alpha as x = logit(alpha) unless it is fixed
    (d alpha / dx = s = alpha (1 - alpha), d2 alpha / dx2 = s (1 - 2 alpha): the gradient's term on the diagonal)."""
    k = d.num_pc
    heter, pc_fixed, alpha_fixed = flags(d, **model)
    pc1, pc2, swapped = search_point(d, est, **model)
    a = float(est["alpha"])
    c = counts or deriv_ref.Counts(d)
    _, g, H = deriv_ref.derivs(c, pc1, pc2, a)
    n = 2 * k + 1
    cols, what = _free_columns(k, heter, pc_fixed)
    s = a * (1 - a)
    if not alpha_fixed:
        e = np.zeros(n)
        e[2 * k] = s
        cols.append(e)
    nf = len(cols)
    out = dict(pos_def=False, cond=float("nan"), se=np.full(nf, np.nan), freemix_se=float("nan"), num_free=nf,
               swapped=swapped)
    if nf:
        J = np.array(cols).T
        A = -(J.T @ H @ J)
        if not alpha_fixed:
            A[-1, -1] -= g[2 * k] * s * (1 - 2 * a)
        w = np.linalg.eigvalsh(A)
        out["A"] = A
        out["eig"] = w
        out["pos_def"] = bool(w.min() > 0)
        if out["pos_def"]:
            out["cond"] = float(w.max() / w.min())
            out["se"] = np.sqrt(np.diag(np.linalg.inv(A)))
            if not alpha_fixed:
                out["freemix_se"] = float(s * out["se"][-1])
    # the rows: a reported PC (sample r, index j) is the search's (sample 3 - r, j) where the swap applies
    se_of = {w_: out["se"][i] for i, w_ in enumerate(what)}
    freemix = a if a < 0.5 else 1 - a
    rows = [("FREEMIX", freemix, out["freemix_se"])]
    rep = {1: np.asarray(est["pc"], dtype=np.float64), 2: np.asarray(est["pc2"], dtype=np.float64)}
    if not heter:
        if not pc_fixed:
            rows += [("PC%d" % (j + 1), rep[1][j], se_of[(0, j)]) for j in range(k)]
    else:
        for r, name in ((1, "ContaminatingSample.PC"), (2, "IntendedSample.PC")):
            for j in range(k):
                src = (3 - r, j) if (swapped and j < 2) else (r, j)
                if r == 2 and pc_fixed and src not in se_of:
                    continue                                  # a fixed coordinate of the intended sample: no row
                rows.append((name + str(j + 1), rep[r][j], se_of.get(src, float("nan"))))
    out["rows"] = rows
    return out


def _newton(c, k, J, x):
    """Maximise the LLK over x + span(J) (J: [2k+1, m]) by Newton steps with step halving; returns (llk, x).  A
    direction in which the likelihood is flat (the contaminant's PCs as alpha -> 0) gets no step."""
    def at(x_):
        llk, g, H = deriv_ref.derivs(c, x_[:k], x_[k:2 * k], x_[2 * k])
        return float(llk), J.T @ g, J.T @ H @ J
    llk, g, H = at(x)
    for _ in range(100):
        w, V = np.linalg.eigh(-H)
        keep = w > 1e-10 * max(w.max(), 1e-300)
        if not keep.any():
            break
        step = J @ (V[:, keep] @ ((V[:, keep].T @ g) / w[keep]))
        if not float(g @ (np.linalg.pinv(J) @ step)) > 1e-12:
            break
        t = 1.0
        while t > 1e-6:
            xn = x + t * step
            cand = at(xn) if 0 < xn[2 * k] < 1 or J[2 * k].max() == 0 else (-np.inf,)
            if cand[0] > llk:
                break
            t *= 0.5
        else:
            break
        x = xn
        llk, g, H = cand
    return llk, x


def profile_ref(d, est, f, counts=None, **model):
    """max over the free PCs of the LLK at FREEMIX = f (alpha = 1 - f on the estimate's side when alpha >= 0.5), by
    Newton steps with step halving from the estimate's PCs; the LLK itself where no PC is free."""
    k = d.num_pc
    heter, pc_fixed, _ = flags(d, **model)
    pc1, pc2, _ = search_point(d, est, **model)
    a = (1 - f) if est["alpha"] >= 0.5 else f
    c = counts or deriv_ref.Counts(d)
    cols, _ = _free_columns(k, heter, pc_fixed)
    if not cols:
        return float(deriv_ref.derivs(c, pc1, pc2, a)[0])
    return _newton(c, k, np.array(cols).T, np.concatenate([pc1, pc2, [a]]))[0]


def optimum_ref(d, pc1, pc2, alpha, counts=None, **model):
    """The model's maximum next to a starting point (free PCs and alpha together), as an estimate dict in the reported
    form: what a search that ended there would hand to the interval."""
    k = d.num_pc
    heter, pc_fixed, alpha_fixed = flags(d, **model)
    assert not alpha_fixed
    c = counts or deriv_ref.Counts(d)
    cols, _ = _free_columns(k, heter, pc_fixed)
    e = np.zeros(2 * k + 1)
    e[2 * k] = 1.0
    llk, x = _newton(c, k, np.array(cols + [e]).T, np.concatenate([pc1, pc2, [alpha]]).astype(np.float64))
    p1, p2, a = x[:k].copy(), x[k:2 * k].copy(), float(x[2 * k])
    if heter and a >= 0.5:
        for j in range(min(k, 2)):
            p1[j], p2[j] = p2[j], p1[j]
    return dict(alpha=a, llk1=-llk, llk0=0.0, pc=p1, pc2=p2, converged=True)
