"""Numpy restatement of the derivatives of the likelihood given genotype priors on both components (DESIGN.md section 17;
what vb2_paired_derivs computes on the device), and of the interval of a paired refit (vb2_paired_interval).

Section 10's math (tests/deriv_ref.py) with section 16's rule (tests/paired_ref.py) per marker and per side:

    L_m = P1' W P2
        P1 = pi1_h[m] where that triple is not all zero, and P1' = P1'' = 0 there; else GF1(pc1), GF1', GF1''
        P2 likewise from pi2_h[m] and GF2(pc2)
        a marker whose pi2_h[m][0] is negative is left out: ten zeros
        the alpha entries W o A', W o (A'' + A' o A') are section 10's

It shares the reading of the pileup (deriv_ref.Counts) and the two tables (deriv_ref._table, _gf) with deriv_ref and no
code with the library.  Like deriv_ref, every function takes the precision it works in from its Counts: np.float64 is the
kernel's, np.longdouble the reference the kernel tests measure against.  derivs_cond returns the condition sums S_e per
entry as deriv_ref.derivs_cond does, and reference() the dict deriv_ref.block_devs takes.

The interval counterpart (se_ref, profile_ref, interval_ref) is interval_ref.py's for a refit with the intended sample's PCs
held: the free coordinates are the contaminant's PCs, then x = logit alpha (alpha alone with fix_pc or known allele
frequencies); alpha is never folded and the profile is a plain Newton climb over the free PCs at a given alpha in [0, 1].
"""
import numpy as np

from deriv_ref import Counts, _assemble, _gf, _table  # noqa: F401

Z975 = 1.959963984540054
HALF_CHI2 = 1.9207294103470620


def marker_terms(c, hyp, pc1, pc2, alpha, inner=False):
    """log L and the nine l_x / l_xy per counted marker of `c` (0 where the marker is left out or L is not > 0), in the
    precision of `c`.  hyp: [M, 6] in panel order (float32 values), or None = both sides all zero.  inner: also the sums
    with every term inside the marker taken by its absolute value (deriv_ref.derivs_cond)."""
    T = c.dtype
    logp, dd = _table(alpha, c.quals, T)
    finite = np.isfinite(logp)
    A = c.N @ np.where(finite, logp, T(0)) + c.other[:, None]
    A = np.where(c.N @ (~finite).astype(T) > 0, T(-np.inf), A)
    A1 = c.N @ dd
    A2 = -(c.N @ (dd * dd))
    if c.kaf is not None:
        af1 = af2 = c.kaf
    else:
        af1 = (c.ud @ np.asarray(pc1, dtype=np.float64).astype(T) + c.mu) / T(2)
        af2 = (c.ud @ np.asarray(pc2, dtype=np.float64).astype(T) + c.mu) / T(2)
    fixed = c.kaf is not None
    P1, P1d, P1dd = _gf(af1, fixed, T)
    P2, P2d, P2dd = _gf(af2, fixed, T)
    n = len(c.idx)
    walked = np.ones(n, dtype=bool)
    if hyp is not None:
        h32 = np.asarray(hyp, dtype=np.float32)[c.idx]
        walked = ~(h32[:, 3] < 0)
        given1 = np.any(h32[:, :3] != 0, axis=1)
        given2 = np.any(h32[:, 3:] != 0, axis=1) & walked
        P1 = np.where(given1[:, None], h32[:, :3].astype(T), P1)
        P2 = np.where(given2[:, None], h32[:, 3:].astype(T), P2)
        zero = T(0)
        P1d, P1dd = np.where(given1[:, None], zero, P1d), np.where(given1[:, None], zero, P1dd)
        P2d, P2dd = np.where(given2[:, None], zero, P2d), np.where(given2[:, None], zero, P2dd)
    A, A1, A2 = A.reshape(-1, 3, 3), A1.reshape(-1, 3, 3), A2.reshape(-1, 3, 3)
    # whether a marker counts is the reference's rule on its double L (h:310), on the unscaled L
    f64 = np.float64
    with np.errstate(under="ignore"):
        lk64 = np.einsum("ma,mab,mb->m", P1.astype(f64), np.exp(A.astype(f64)), P2.astype(f64))
        lk = np.einsum("ma,mab,mb->m", P1, np.exp(A), P2)
    amax = np.max(A.reshape(-1, 9), axis=1)
    amax = np.where(np.isfinite(amax), amax, T(0))
    W = np.exp(A - amax[:, None, None])
    WA, WB = W * A1, W * (A2 + A1 * A1)

    def q(a, w, b):
        return np.einsum("ma,mab,mb->m", a, w, b)
    Ls = q(P1, W, P2)
    live = (lk64 > 0) & (lk > 0) & (Ls > 0) & walked
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(live, T(1) / Ls, T(0))
    l1, l2, la = q(P1d, W, P2) * inv, q(P1, W, P2d) * inv, q(P1, WA, P2) * inv
    out = np.zeros((10, n), dtype=T)
    out[0] = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    out[1], out[2], out[3] = l1, l2, la
    out[4] = q(P1dd, W, P2) * inv - l1 * l1
    out[5] = q(P1, W, P2dd) * inv - l2 * l2
    out[6] = q(P1d, W, P2d) * inv - l1 * l2
    out[7] = q(P1d, WA, P2) * inv - l1 * la
    out[8] = q(P1, WA, P2d) * inv - l2 * la
    out[9] = q(P1, WB, P2) * inv - la * la
    out[:, ~live] = 0
    assert out.dtype == np.dtype(T)
    if not inner:
        return out
    ab = np.abs
    s1, s2, sa = q(ab(P1d), W, P2) * inv, q(P1, W, ab(P2d)) * inv, q(P1, ab(WA), P2) * inv
    tot = np.zeros_like(out)
    tot[1], tot[2], tot[3] = s1, s2, sa
    tot[4] = q(ab(P1dd), W, P2) * inv + s1 * s1
    tot[5] = q(P1, W, ab(P2dd)) * inv + s2 * s2
    tot[6] = q(ab(P1d), W, ab(P2d)) * inv + s1 * s2
    tot[7] = q(ab(P1d), ab(WA), P2) * inv + s1 * sa
    tot[8] = q(P1, ab(WA), ab(P2d)) * inv + s2 * sa
    tot[9] = q(P1, W * (ab(A2) + A1 * A1), P2) * inv + sa * sa
    tot[:, ~live] = 0
    return out, tot


def derivs(c, hyp, pc1, pc2, alpha):
    """(llk, grad [2k+1], hess [2k+1, 2k+1]) of LLK(. | h) with respect to (pc1, pc2, alpha), in the precision of `c`."""
    v = marker_terms(c, hyp, pc1, pc2, alpha)
    grad, hess = _assemble(c, v, c.ud)
    llk = v[0].sum()
    assert llk.dtype == np.dtype(c.dtype)
    return llk, grad, hess


def derivs_cond(c, hyp, pc1, pc2, alpha, inner=False):
    """derivs and the condition sums (S_grad, S_hess) of its entries; inner: the sums inside the markers (both as
    deriv_ref.derivs_cond defines them)."""
    if inner:
        _, tot = marker_terms(c, hyp, pc1, pc2, alpha, inner=True)
        return _assemble(c, tot, np.abs(c.ud))
    v = marker_terms(c, hyp, pc1, pc2, alpha)
    grad, hess = _assemble(c, v, c.ud)
    lx = {1: v[1], 2: v[2], 0: v[3]}
    s = np.zeros_like(v)
    s[1], s[2], s[3] = np.abs(v[1]), np.abs(v[2]), np.abs(v[3])
    for j, (x, y) in {4: (1, 1), 5: (2, 2), 6: (1, 2), 7: (1, 0), 8: (2, 0), 9: (0, 0)}.items():
        prod = lx[x] * lx[y]
        s[j] = np.abs(v[j] + prod) + np.abs(prod)
    sg, sh = _assemble(c, s, np.abs(c.ud))
    return v[0].sum(), grad, hess, sg, sh


def reference(c64, c80, hyp, pc1, pc2, alpha):
    """One point's references in the shape deriv_ref.block_devs takes: the float64 restatement, the 80-bit one and its
    condition sums (at alpha = 0 / 1 the blocks of the side without reads in the sums inside the markers)."""
    assert c64.dtype == np.float64 and c80.dtype == np.longdouble
    l64, g64, h64 = derivs(c64, hyp, pc1, pc2, alpha)
    l80, g80, h80, sg, sh = derivs_cond(c80, hyp, pc1, pc2, alpha)
    assert g80.dtype == np.longdouble and h80.dtype == np.longdouble and sh.dtype == np.longdouble
    if alpha == 0 or alpha == 1:
        gi, hi = derivs_cond(c80, hyp, pc1, pc2, alpha, inner=True)
        k = c64.k
        dead = slice(0, k) if alpha == 0 else slice(k, 2 * k)
        sg, sh = sg.copy(), sh.copy()
        sg[dead] = gi[dead]
        sh[dead, :] = hi[dead, :]
        sh[:, dead] = hi[:, dead]
    return dict(l64=l64, g64=g64, h64=h64, l80=l80, g80=g80, h80=h80, sg=sg, sh=sh, k=c64.k)


class Evaluator:
    """evaluate(num_point, pc1, pc2, alpha) of paired_intervals_with_evaluator over the float64 restatement: slot h is
    (counts[h], hyps[h]).  Keeps what it was called with."""

    def __init__(self, counts, hyps):
        self.counts, self.hyps, self.calls = list(counts), list(hyps), []

    def __call__(self, num_point, pc1, pc2, alpha):
        self.calls.append((num_point.copy(), pc1.copy(), pc2.copy(), alpha.copy()))
        out, p = [], 0
        for h, n in enumerate(num_point):
            for _ in range(int(n)):
                out.append(derivs(self.counts[h], self.hyps[h], pc1[p], pc2[p], alpha[p]))
                p += 1
        return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64),
                np.array([o[2] for o in out], dtype=np.float64))


# ---- the interval of a paired refit ----

def _free(c, fix_pc):
    """Columns of the map from the free PC coordinates to (pc1, pc2, alpha): the contaminant's PCs unless they are fixed."""
    k = c.k
    if fix_pc or c.kaf is not None:
        return np.zeros((2 * k + 1, 0))
    return np.eye(2 * k + 1)[:, :k]


def se_ref(c, hyp, est, pc2_fixed, fix_pc=False):
    """Standard errors at a paired estimate (alpha, pc = the contaminant's PCs): A = -J' H J in the free coordinates, alpha
    as x = logit alpha.  A dict with pos_def, cond, A, se per free coordinate (alpha last), alpha_se and the rows."""
    k = c.k
    a = float(est["alpha"])
    pc1 = np.asarray(est["pc"], dtype=np.float64)[:k]
    _, g, H = derivs(c, hyp, pc1, np.asarray(pc2_fixed, dtype=np.float64), a)
    s = a * (1 - a)
    e = np.zeros((2 * k + 1, 1))
    e[2 * k] = s
    J = np.concatenate([_free(c, fix_pc), e], axis=1)
    A = -(J.T @ H @ J)
    A[-1, -1] -= g[2 * k] * s * (1 - 2 * a)
    nf = J.shape[1]
    out = dict(pos_def=False, cond=float("nan"), se=np.full(nf, np.nan), alpha_se=float("nan"), num_free=nf, A=A)
    if np.all(np.isfinite(A)):
        w = np.linalg.eigvalsh(A)
        out["pos_def"] = bool(w.min() > 0)
        if out["pos_def"]:
            out["cond"] = float(w.max() / w.min())
            out["se"] = np.sqrt(np.diag(np.linalg.inv(A)))
            out["alpha_se"] = float(s * out["se"][-1])
    out["rows"] = [("ALPHA", a, out["alpha_se"])] + [("ContaminatingSample.PC%d" % (j + 1), pc1[j], out["se"][j])
                                                     for j in range(nf - 1)]
    return out


def _newton(c, hyp, J, x):
    """Maximise LLK(. | h) over x + span(J) by Newton steps with step halving (interval_ref._newton's scheme); (llk, x)."""
    k = c.k

    def at(x_):
        llk, g, H = derivs(c, hyp, x_[:k], x_[k:2 * k], x_[2 * k])
        return float(llk), J.T @ g, J.T @ H @ J
    llk, g, H = at(x)
    for _ in range(100):
        w, V = np.linalg.eigh(-H)
        keep = w > 1e-10 * max(w.max(), 1e-300)
        if not keep.any():
            break
        dz = V[:, keep] @ ((V[:, keep].T @ g) / w[keep])
        if not float(g @ dz) > 1e-12:
            break
        t = 1.0
        while t > 1e-6:
            xn = x + t * (J @ dz)
            cand = at(xn)
            if cand[0] > llk:
                break
            t *= 0.5
        else:
            break
        x = xn
        llk, g, H = cand
    return llk, x


def profile_ref(c, hyp, est, pc2_fixed, alpha, fix_pc=False):
    """max over the free PCs of LLK(. | h) at `alpha`, unfolded, from the estimate's PCs; the LLK itself where none is free."""
    k = c.k
    x = np.concatenate([np.asarray(est["pc"], dtype=np.float64)[:k], np.asarray(pc2_fixed, dtype=np.float64), [float(alpha)]])
    J = _free(c, fix_pc)
    if J.shape[1] == 0:
        return float(derivs(c, hyp, x[:k], x[k:2 * k], x[2 * k])[0])
    return _newton(c, hyp, J, x)[0]


def interval_ref(c, hyp, est, pc2_fixed, fix_pc=False, tol=1e-7):
    """(lo, hi) of the profile interval on the restatement: the cut 1.92 below the larger of the estimate's LLK and the
    profile at the estimate; an end is 0 or 1 where the profile there is above the cut; bisection otherwise."""
    a_hat = float(est["alpha"])
    top = max(-float(est["llk1"]), profile_ref(c, hyp, est, pc2_fixed, a_hat, fix_pc))
    cut = top - HALF_CHI2

    def end(edge):
        if profile_ref(c, hyp, est, pc2_fixed, edge, fix_pc) >= cut:
            return float(edge)
        inside, outside = a_hat, float(edge)
        while abs(outside - inside) > tol * max(a_hat, 1e-3):
            mid = 0.5 * (inside + outside)
            if profile_ref(c, hyp, est, pc2_fixed, mid, fix_pc) >= cut:
                inside = mid
            else:
                outside = mid
        return 0.5 * (inside + outside)
    return end(0.0), end(1.0)
