"""Numpy restatement of the LLK's derivatives (what vb2_llk_derivs_batch computes on the device).

derivs(d, pc1, pc2, alpha) -> (llk, grad [2k+1], hess [2k+1, 2k+1]) with respect to (pc1[0..k), pc2[0..k), alpha), for a
PileupData-shaped input, from the reference's expressions (ContaminationEstimator.h): table entries h:223-224, genotype
priors h:186-192 (derivatives 0 where the allele frequency is clamped), AF = (UD pc + mean) / 2 (h:251-267), markers
counted where L > 0 (h:310), the +-3 sd depth filter when it is on (h:239-249).

Every function takes the precision it works in: Counts(d, dtype) fixes it for what is computed from those counts.
np.float64 is the kernel's own precision; np.longdouble (the x87 80-bit format on x86-64, 64 bits of mantissa) is the
reference the kernel tests measure against.  Nothing here calls BLAS for longdouble (numpy's matmul and einsum fall back
to their own loops), and derivs asserts the dtype of what it returns so that a silent drop to double would show.

derivs_cond returns, next to every gradient and Hessian entry e, its condition sum S_e: the sum over the markers of the
absolute values of the terms before they cancel, e.g. (|L_xy / L| + |l_x l_y|) |U_a U_b| / 4 for a PC-PC entry.  An
error in units of S_e is what a correctly rounded evaluation in another order can differ by; relative to the entry itself
(or to its block's largest entry) it is not, because whole blocks cancel to ~0 on deep markers.
"""
import numpy as np

MIN_AF, MAX_AF = 0.00005, 0.99995


def _consts(T):
    """pErr per quality; P(class | genotype, error) and P(class | genotype, no error), class ref / alt (h:164-177)."""
    perr = np.power(T(10), np.arange(94).astype(T) / T(-10))
    err = np.array([[T(0), T(1) / T(6), T(1) / T(3)], [T(1) / T(3), T(1) / T(6), T(0)]], dtype=T)
    ok = np.array([[1.0, 0.5, 0.0], [0.0, 0.5, 1.0]], dtype=T)
    return perr, err, ok


class Counts:
    """Per counted marker: reads per (class ref/alt, quality present in the sample), the log-sum of its class-other
    reads, its panel row; all in `dtype`."""

    def __init__(self, d, dtype=np.float64):
        T = self.dtype = np.dtype(dtype).type
        perr = _consts(T)[0]
        off = np.asarray(d.read_off, dtype=np.int64)
        depth = np.diff(off)
        keep = depth > 0
        if not d.sanity_disabled:
            keep &= ~((depth < d.avg_depth - 3 * d.sd_depth) | (depth > d.avg_depth + 3 * d.sd_depth))
        M = depth.shape[0]
        mk = np.repeat(np.arange(M), depth)
        bases = np.asarray(d.bases)[off[0]:off[-1]]
        alt = np.asarray(d.alt_base)[mk]
        up = bases & 0xDF                                     # toupper for letters
        cls = np.where((bases == ord(".")) | (bases == ord(",")), 0, np.where(up == (alt & 0xDF), 1, 2))
        q = np.clip(np.asarray(d.quals)[off[0]:off[-1]].astype(np.int64) - 33, 0, 93)
        sel = cls < 2
        self.quals = np.unique(q[sel])                        # the table rows the sample uses (ascending)
        nq = len(self.quals)
        N = np.zeros((M, 2 * nq))                             # read counts are exact in any format
        np.add.at(N, (mk[sel], cls[sel] * nq + np.searchsorted(self.quals, q[sel])), 1.0)
        other = np.zeros(M, dtype=T)
        np.add.at(other, mk[~sel], np.log(T(2) / T(3) * perr[q[~sel]]))
        self.idx = np.nonzero(keep)[0]
        self.N = N[self.idx].astype(T)
        self.other = other[self.idx]
        self.ud = np.asarray(d.ud, dtype=np.float64).reshape(M, -1)[self.idx].astype(T)
        self.mu = np.asarray(d.means, dtype=np.float64)[self.idx].astype(T)
        self.kaf = None if d.known_af is None else np.asarray(d.known_af, dtype=np.float64)[self.idx].astype(T)
        self.k = int(d.num_pc)


def _table(alpha, quals, T):
    """log p, d = dp/dalpha / p, per (class, quality of `quals`) x (g1, g2): [2 len(quals), 9] each."""
    perr, err, ok = _consts(T)
    alpha = T(alpha)
    one = T(1)
    e = perr[quals][None, :, None, None]
    err1, err2 = err[:, None, :, None], err[:, None, None, :]
    ok1, ok2 = ok[:, None, :, None], ok[:, None, None, :]
    p = (alpha * err1 + (one - alpha) * err2) * e + (alpha * ok1 + (one - alpha) * ok2) * (one - e)
    u1, u2 = err1 * e + ok1 * (one - e), err2 * e + ok2 * (one - e)
    with np.errstate(divide="ignore", invalid="ignore"):
        logp = np.log(p)
        dd = np.where(p != 0, (u1 - u2) / p, T(0))
    n = 2 * len(quals)
    return logp.reshape(n, 9), np.broadcast_to(dd, (2, len(quals), 3, 3)).reshape(n, 9)


def _gf(af, fixed, T):
    clamped = (af < T(MIN_AF)) | (af > T(MAX_AF)) | fixed
    a = np.clip(af, T(MIN_AF), T(MAX_AF))
    g = np.stack([(1 - a) ** 2, 2 * a * (1 - a), a * a], axis=1)
    g1 = np.stack([-2 * (1 - a), 2 - 4 * a, 2 * a], axis=1)
    g2 = np.broadcast_to(np.array([2.0, -4.0, 2.0], dtype=T), g.shape).copy()
    g1[clamped] = 0
    g2[clamped] = 0
    return g, g1, g2


def marker_terms(c, pc1, pc2, alpha, inner=False):
    """log L and the nine l_x / l_xy per counted marker (0 where L is not > 0), in the precision of `c`.  inner: also the
    same ten sums with every term inside the marker taken by its absolute value (see derivs_cond)."""
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
    G1, G1d, G1dd = _gf(af1, fixed, T)
    G2, G2d, G2dd = _gf(af2, fixed, T)
    A, A1, A2 = A.reshape(-1, 3, 3), A1.reshape(-1, 3, 3), A2.reshape(-1, 3, 3)
    # whether a marker counts is the reference's rule on its double L (h:310): an 80-bit L would not underflow where it does
    f64 = np.float64
    with np.errstate(under="ignore"):
        lk64 = np.einsum("ma,mab,mb->m", G1.astype(f64), np.exp(A.astype(f64)), G2.astype(f64))
    lk = np.einsum("ma,mab,mb->m", G1, np.exp(A), G2)
    amax = np.max(A.reshape(-1, 9), axis=1)
    amax = np.where(np.isfinite(amax), amax, T(0))
    W = np.exp(A - amax[:, None, None])
    WA, WB = W * A1, W * (A2 + A1 * A1)

    def q(a, w, b):
        return np.einsum("ma,mab,mb->m", a, w, b)
    Ls = q(G1, W, G2)
    live = (lk64 > 0) & (lk > 0) & (Ls > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(live, T(1) / Ls, T(0))
    l1, l2, la = q(G1d, W, G2) * inv, q(G1, W, G2d) * inv, q(G1, WA, G2) * inv
    out = np.zeros((10, len(lk)), dtype=T)
    out[0] = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    out[1], out[2], out[3] = l1, l2, la
    out[4] = q(G1dd, W, G2) * inv - l1 * l1
    out[5] = q(G1, W, G2dd) * inv - l2 * l2
    out[6] = q(G1d, W, G2d) * inv - l1 * l2
    out[7] = q(G1d, WA, G2) * inv - l1 * la
    out[8] = q(G1, WA, G2d) * inv - l2 * la
    out[9] = q(G1, WB, G2) * inv - la * la
    out[:, ~live] = 0
    assert out.dtype == np.dtype(T)
    if not inner:
        return out
    ab = np.abs
    s1, s2, sa = q(ab(G1d), W, G2) * inv, q(G1, W, ab(G2d)) * inv, q(G1, ab(WA), G2) * inv
    tot = np.zeros_like(out)
    tot[1], tot[2], tot[3] = s1, s2, sa
    tot[4] = q(ab(G1dd), W, G2) * inv + s1 * s1
    tot[5] = q(G1, W, ab(G2dd)) * inv + s2 * s2
    tot[6] = q(ab(G1d), W, ab(G2d)) * inv + s1 * s2
    tot[7] = q(ab(G1d), ab(WA), G2) * inv + s1 * sa
    tot[8] = q(G1, ab(WA), ab(G2d)) * inv + s2 * sa
    tot[9] = q(G1, W * (ab(A2) + A1 * A1), G2) * inv + sa * sa
    tot[:, ~live] = 0
    return out, tot


def live_share(c, pc1, pc2, alpha):
    """The share of the counted markers with L > 0 at this point."""
    return float(np.mean(marker_terms(c, pc1, pc2, alpha)[0] != 0))


def _assemble(c, v, w):
    """The sums over the markers: scalars v[1..9] with the panel rows U (w = U for the derivatives, |U| for the
    condition sums)."""
    T = c.dtype
    k = c.k
    n = 2 * k + 1
    grad = np.zeros(n, dtype=T)
    hess = np.zeros((n, n), dtype=T)
    grad[2 * k] = v[3].sum()
    hess[2 * k, 2 * k] = v[9].sum()
    if c.kaf is None:
        U = w
        grad[:k] = U.T @ v[1] / 2
        grad[k:2 * k] = U.T @ v[2] / 2
        hess[:k, :k] = (U * v[4][:, None]).T @ U / 4
        hess[k:2 * k, k:2 * k] = (U * v[5][:, None]).T @ U / 4
        hess[:k, k:2 * k] = (U * v[6][:, None]).T @ U / 4
        hess[k:2 * k, :k] = hess[:k, k:2 * k].T
        hess[:k, 2 * k] = hess[2 * k, :k] = U.T @ v[7] / 2
        hess[k:2 * k, 2 * k] = hess[2 * k, k:2 * k] = U.T @ v[8] / 2
    assert grad.dtype == np.dtype(T) and hess.dtype == np.dtype(T)
    return grad, hess


def derivs(d_or_counts, pc1, pc2, alpha):
    c = d_or_counts if isinstance(d_or_counts, Counts) else Counts(d_or_counts)
    v = marker_terms(c, pc1, pc2, alpha)
    grad, hess = _assemble(c, v, c.ud)
    llk = v[0].sum()
    assert llk.dtype == np.dtype(c.dtype)
    return llk, grad, hess


def derivs_cond(c, pc1, pc2, alpha, inner=False):
    """derivs, and the condition sums (S_grad [2k+1], S_hess [2k+1, 2k+1]) of its entries.

    S_e takes each marker's term as it comes out of the marker.  At alpha = 0 the likelihood does not depend on pc1 at all
    (at alpha = 1: on pc2): every marker's l_1, l_11, l_12, l_1a is exactly 0 as a sum GF1'[g] (...) of terms that cancel
    INSIDE the marker, so S_e is itself rounding noise there and no unit for anything (measured: the float64 restatement
    is 1e3 S_e away from the 80-bit one on 2 000 markers).  inner=True returns the sums with the terms inside the marker
    taken by their absolute values as well: the unit for those blocks at those two points, and only there (it is never
    smaller than S_e, so using it elsewhere would loosen the check)."""
    if inner:
        v, tot = marker_terms(c, pc1, pc2, alpha, inner=True)
        return _assemble(c, tot, np.abs(c.ud))
    v = marker_terms(c, pc1, pc2, alpha)
    grad, hess = _assemble(c, v, c.ud)
    lx = {1: v[1], 2: v[2], 0: v[3]}
    s = np.zeros_like(v)
    s[1], s[2], s[3] = np.abs(v[1]), np.abs(v[2]), np.abs(v[3])
    for j, (x, y) in {4: (1, 1), 5: (2, 2), 6: (1, 2), 7: (1, 0), 8: (2, 0), 9: (0, 0)}.items():
        prod = lx[x] * lx[y]
        s[j] = np.abs(v[j] + prod) + np.abs(prod)             # |L_xy / L| + |l_x l_y|
    sg, sh = _assemble(c, s, np.abs(c.ud))
    return v[0].sum(), grad, hess, sg, sh


def blocks(k):
    """Index sets of the three gradient and six Hessian blocks of (pc1, pc2, alpha)."""
    a, b, c = slice(0, k), slice(k, 2 * k), slice(2 * k, 2 * k + 1)
    return ({"pc1": a, "pc2": b, "alpha": c},
            {"pc1.pc1": (a, a), "pc2.pc2": (b, b), "pc1.pc2": (a, b), "pc1.alpha": (a, c), "pc2.alpha": (b, c),
             "alpha.alpha": (c, c)})


def scaled_dev(x, ref, s):
    """max_e |x_e - ref_e| / S_e over a block (entries with S_e = 0 have no terms at all: they must be equal)."""
    x, ref, s = np.asarray(x), np.asarray(ref), np.asarray(s)
    if x.size == 0:
        return 0.0
    diff = np.abs(x.astype(ref.dtype) - ref)
    none = s == 0
    if np.any(diff[none] != 0):
        return float("inf")
    if np.all(none):
        return 0.0
    return float(np.max(diff[~none] / s[~none]))


def af_margin(d, pc1, pc2):
    """Smallest distance of a counted marker's allele frequency to a clamp boundary (unclamped markers only)."""
    c = Counts(d)
    if c.kaf is not None:
        return np.inf
    out = np.inf
    for pc in (pc1, pc2):
        af = (c.ud @ np.asarray(pc, dtype=np.float64) + c.mu) / 2.0
        inside = (af >= MIN_AF) & (af <= MAX_AF)
        if inside.any():
            out = min(out, float(np.min(np.minimum(af[inside] - MIN_AF, MAX_AF - af[inside]))))
    return out


TOL_FACTOR, TOL_FLOOR = 32.0, 1e-13


def reference(c64, c80, pc1, pc2, alpha):
    """One point's references: the float64 restatement (the kernel's precision in another order), the 80-bit one and
    its condition sums."""
    assert c64.dtype == np.float64 and c80.dtype == np.longdouble
    l64, g64, h64 = derivs(c64, pc1, pc2, alpha)
    l80, g80, h80, sg, sh = derivs_cond(c80, pc1, pc2, alpha)
    assert g80.dtype == np.longdouble and h80.dtype == np.longdouble and sh.dtype == np.longdouble
    if alpha == 0 or alpha == 1:
        # the blocks of the sample that has no reads at this alpha: measured in the sums inside the markers (derivs_cond)
        gi, hi = derivs_cond(c80, pc1, pc2, alpha, inner=True)
        k = c64.k
        dead = slice(0, k) if alpha == 0 else slice(k, 2 * k)
        sg, sh = sg.copy(), sh.copy()
        sg[dead] = gi[dead]
        sh[dead, :] = hi[dead, :]
        sh[:, dead] = hi[:, dead]
    return dict(l64=l64, g64=g64, h64=h64, l80=l80, g80=g80, h80=h80, sg=sg, sh=sh, k=c64.k)


def block_devs(ref, grad, hess, alpha_entries=True):
    """Per block: (dev, dev64, tol).  dev = max_e |given_e - ref80_e| / S_e, dev64 the same for the float64 restatement
    (the floor: the same arithmetic in the kernel's precision in another order), tol = max(32 dev64, 1e-13).  The 32
    allows for the device's other order of operations -- products of up to ~800 table rows against one sum of logarithms,
    a strided sum and a tree against numpy's pairwise sums; it is a guess, and tests that need more say so."""
    gb, hb = blocks(ref["k"])
    out = {}
    for name, s in gb.items():
        if not alpha_entries and "alpha" in name:
            continue
        dev64 = scaled_dev(ref["g64"][s], ref["g80"][s], ref["sg"][s])
        out["g:" + name] = (scaled_dev(grad[s], ref["g80"][s], ref["sg"][s]), dev64, max(TOL_FACTOR * dev64, TOL_FLOOR))
    for name, (r, q) in hb.items():
        if not alpha_entries and "alpha" in name:
            continue
        dev64 = scaled_dev(ref["h64"][r, q], ref["h80"][r, q], ref["sh"][r, q])
        out["h:" + name] = (scaled_dev(hess[r, q], ref["h80"][r, q], ref["sh"][r, q]), dev64,
                            max(TOL_FACTOR * dev64, TOL_FLOOR))
    return out
