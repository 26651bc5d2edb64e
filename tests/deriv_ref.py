"""Numpy restatement of the LLK's derivatives (what vb2_llk_derivs_batch computes on the device).

derivs(d, pc1, pc2, alpha) -> (llk, grad [2k+1], hess [2k+1, 2k+1]) with respect to (pc1[0..k), pc2[0..k), alpha), for a
PileupData-shaped input, from the reference's expressions (ContaminationEstimator.h): table entries h:223-224, genotype
priors h:186-192 (derivatives 0 where the allele frequency is clamped), AF = (UD pc + mean) / 2 (h:251-267), markers
counted where L > 0 (h:310), the +-3 sd depth filter when it is on (h:239-249).
"""
import numpy as np

MIN_AF, MAX_AF = 0.00005, 0.99995
_PERR = np.power(10.0, np.arange(94) / -10.0)
# P(class | genotype, error) and P(class | genotype, no error), class ref / alt (h:164-177)
_ERR = np.array([[0.0, 1.0 / 6.0, 1.0 / 3.0], [1.0 / 3.0, 1.0 / 6.0, 0.0]])
_OK = np.array([[1.0, 0.5, 0.0], [0.0, 0.5, 1.0]])


class Counts:
    """Per counted marker: reads per (class ref/alt, quality), the log-sum of its class-other reads, its panel row."""

    def __init__(self, d):
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
        N = np.zeros((M, 2, 94))
        sel = cls < 2
        np.add.at(N, (mk[sel], cls[sel], q[sel]), 1.0)
        other = np.zeros(M)
        np.add.at(other, mk[~sel], np.log(2.0 / 3.0 * _PERR[q[~sel]]))
        self.idx = np.nonzero(keep)[0]
        self.N = N[self.idx].reshape(len(self.idx), 188)
        self.other = other[self.idx]
        self.ud = np.asarray(d.ud, dtype=np.float64).reshape(M, -1)[self.idx]
        self.mu = np.asarray(d.means, dtype=np.float64)[self.idx]
        self.kaf = None if d.known_af is None else np.asarray(d.known_af, dtype=np.float64)[self.idx]
        self.k = int(d.num_pc)


def _table(alpha):
    """log p, d = dp/dalpha / p, per (class, quality) x (g1, g2): [188, 9] each."""
    e = _PERR[None, :, None, None]
    err1, err2 = _ERR[:, None, :, None], _ERR[:, None, None, :]
    ok1, ok2 = _OK[:, None, :, None], _OK[:, None, None, :]
    p = (alpha * err1 + (1 - alpha) * err2) * e + (alpha * ok1 + (1 - alpha) * ok2) * (1 - e)
    u1, u2 = err1 * e + ok1 * (1 - e), err2 * e + ok2 * (1 - e)
    with np.errstate(divide="ignore", invalid="ignore"):
        logp = np.log(p)
        dd = np.where(p != 0, (u1 - u2) / p, 0.0)
    return logp.reshape(188, 9), np.broadcast_to(dd, (2, 94, 3, 3)).reshape(188, 9)


def _gf(af, fixed):
    clamped = (af < MIN_AF) | (af > MAX_AF) | fixed
    a = np.clip(af, MIN_AF, MAX_AF)
    g = np.stack([(1 - a) ** 2, 2 * a * (1 - a), a * a], axis=1)
    g1 = np.stack([-2 * (1 - a), 2 - 4 * a, 2 * a], axis=1)
    g2 = np.broadcast_to(np.array([2.0, -4.0, 2.0]), g.shape).copy()
    g1[clamped] = 0
    g2[clamped] = 0
    return g, g1, g2


def marker_terms(c, pc1, pc2, alpha):
    """log L and the nine l_x / l_xy per counted marker (0 where L is not > 0)."""
    logp, dd = _table(alpha)
    finite = np.isfinite(logp)
    A = c.N @ np.where(finite, logp, 0.0) + c.other[:, None]
    A = np.where(c.N @ (~finite).astype(np.float64) > 0, -np.inf, A)
    A1 = c.N @ dd
    A2 = -(c.N @ (dd * dd))
    if c.kaf is not None:
        af1 = af2 = c.kaf
    else:
        af1 = (c.ud @ np.asarray(pc1, dtype=np.float64) + c.mu) / 2.0
        af2 = (c.ud @ np.asarray(pc2, dtype=np.float64) + c.mu) / 2.0
    fixed = c.kaf is not None
    G1, G1d, G1dd = _gf(af1, fixed)
    G2, G2d, G2dd = _gf(af2, fixed)
    A, A1, A2 = A.reshape(-1, 3, 3), A1.reshape(-1, 3, 3), A2.reshape(-1, 3, 3)
    lk = np.einsum("ma,mab,mb->m", G1, np.exp(A), G2)
    amax = np.max(A.reshape(-1, 9), axis=1)
    amax = np.where(np.isfinite(amax), amax, 0.0)
    W = np.exp(A - amax[:, None, None])
    WA, WB = W * A1, W * (A2 + A1 * A1)

    def q(a, w, b):
        return np.einsum("ma,mab,mb->m", a, w, b)
    Ls = q(G1, W, G2)
    live = (lk > 0) & (Ls > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(live, 1.0 / Ls, 0.0)
    l1, l2, la = q(G1d, W, G2) * inv, q(G1, W, G2d) * inv, q(G1, WA, G2) * inv
    out = np.zeros((10, len(lk)))
    out[0] = np.where(live, np.log(np.where(live, lk, 1.0)), 0.0)
    out[1], out[2], out[3] = l1, l2, la
    out[4] = q(G1dd, W, G2) * inv - l1 * l1
    out[5] = q(G1, W, G2dd) * inv - l2 * l2
    out[6] = q(G1d, W, G2d) * inv - l1 * l2
    out[7] = q(G1d, WA, G2) * inv - l1 * la
    out[8] = q(G1, WA, G2d) * inv - l2 * la
    out[9] = q(G1, WB, G2) * inv - la * la
    out[:, ~live] = 0.0
    return out


def derivs(d_or_counts, pc1, pc2, alpha):
    c = d_or_counts if isinstance(d_or_counts, Counts) else Counts(d_or_counts)
    v = marker_terms(c, pc1, pc2, alpha)
    k = c.k
    n = 2 * k + 1
    grad = np.zeros(n)
    hess = np.zeros((n, n))
    grad[2 * k] = v[3].sum()
    hess[2 * k, 2 * k] = v[9].sum()
    if c.kaf is None:
        U = c.ud
        grad[:k] = U.T @ v[1] / 2
        grad[k:2 * k] = U.T @ v[2] / 2
        hess[:k, :k] = (U * v[4][:, None]).T @ U / 4
        hess[k:2 * k, k:2 * k] = (U * v[5][:, None]).T @ U / 4
        hess[:k, k:2 * k] = (U * v[6][:, None]).T @ U / 4
        hess[k:2 * k, :k] = hess[:k, k:2 * k].T
        hess[:k, 2 * k] = hess[2 * k, :k] = U.T @ v[7] / 2
        hess[k:2 * k, 2 * k] = hess[2 * k, k:2 * k] = U.T @ v[8] / 2
    return v[0].sum(), grad, hess


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
