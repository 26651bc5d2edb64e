"""Numpy restatement of the relatedness statistic (what vb2_ctx_marginals_related and
vb2_source_set_relations compute on the device), from the reference's model as source_ref restates it.

Per counted marker, at the point source_ref.search_point gives, with W, GF1, GF2, L as in source_ref and p the clamped
allele frequency GF2 is formed from:

    h[g]  = (sum_g1 GF1[g1] W[g1][g]) / L        own-genotype likelihood relative to a random individual; q = GF2 h
    t[g'] = sum_g q[g] T_p[g][g']                genotype distribution of a relative sharing one allele by descent
    T_p   = [(1-p, p, 0), ((1-p)/2, 1/2, p/2), (0, 1-p, p)]

and for target i, partner j over the markers both count, d2 = q_i . h_j, d1 = t_i . h_j,

    K_r(i, j) = sum_m log max(k0_r + k1_r d1 + k2_r d2, 1e-30)       r = DUP, PO, FS, D2

Every function takes the precision it works in from its Counts (np.float64: the kernel's; np.longdouble: the reference
the kernel tests measure against).
"""
import numpy as np

import source_ref as sr
from deriv_ref import MAX_AF, MIN_AF, Counts, _gf, _table

DOT_FLOOR = sr.DOT_FLOOR
RELATIONS = ("DUP", "PO", "FS", "D2")
COEF = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.25, 0.5, 0.25], [0.5, 0.5, 0.0]])       # (k0, k1, k2), exact in float32


def transition(p):
    """T_p [n, 3, 3] of allele frequencies p [n]: row = the individual's genotype, column = its IBD-1 relative's."""
    T = p.dtype.type
    z, half = np.zeros_like(p), T(0.5)
    n = 1 - p
    return np.stack([np.stack([n, p, z], axis=1), np.stack([half * n, half + z, half * p], axis=1), np.stack([z, n, p], axis=1)],
                    axis=1)


def marginals(c, pc1, pc2, alpha):
    """dict(q, h, t [n, 3], live [n], gf2, p) over the counted markers of `c` (a Counts), in its precision: source_ref's
    marginals with the sum over the contaminant kept apart from the prior; rows of markers with L not > 0 are 0."""
    T = c.dtype
    logp, _ = _table(alpha, c.quals, T)
    finite = np.isfinite(logp)
    A = c.N @ np.where(finite, logp, T(0)) + c.other[:, None]
    A = np.where(c.N @ (~finite).astype(T) > 0, T(-np.inf), A)
    if c.kaf is not None:
        af1 = af2 = c.kaf
    else:
        af1 = (c.ud @ np.asarray(pc1, dtype=np.float64).astype(T) + c.mu) / T(2)
        af2 = (c.ud @ np.asarray(pc2, dtype=np.float64).astype(T) + c.mu) / T(2)
    G1 = _gf(af1, True, T)[0]
    G2 = _gf(af2, True, T)[0]
    p = np.clip(af2, T(MIN_AF), T(MAX_AF))
    A = A.reshape(-1, 3, 3)
    f64 = np.float64
    with np.errstate(under="ignore"):
        lk64 = np.einsum("ma,mab,mb->m", G1.astype(f64), np.exp(A.astype(f64)), G2.astype(f64))
        lk = np.einsum("ma,mab,mb->m", G1, np.exp(A), G2)
    amax = np.max(A.reshape(-1, 9), axis=1)
    amax = np.where(np.isfinite(amax), amax, T(0))
    with np.errstate(under="ignore"):
        W = np.exp(A - amax[:, None, None])
    r = np.einsum("mab,mb->ma", W, G2)
    s = np.einsum("ma,mab->mb", G1, W)
    Ls = np.einsum("ma,ma->m", G1, r)
    live = (lk64 > 0) & (lk > 0) & (Ls > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(live, T(1) / np.where(live, Ls, T(1)), T(0))
    h = s * inv[:, None]
    q = G2 * s * inv[:, None]
    with np.errstate(under="ignore"):
        t = np.einsum("ma,mab->mb", q, transition(p))
    for x in (h, q, t):
        x[~live] = 0
        assert x.dtype == np.dtype(T)
    return dict(q=q, h=h, t=t, live=live, gf2=G2, p=p)


def panel_order(c, num_marker, m):
    """(q, h, t) [M, 3] in panel order, zeros for the markers the sample does not count."""
    out = []
    for name in ("q", "h", "t"):
        x = np.zeros((num_marker, 3), dtype=c.dtype)
        x[c.idx] = m[name]
        out.append(x)
    return tuple(out)


def rows(d, pc, pc2, alpha, heter=True, dtype=np.float64):
    """A sample's (q, h, t) in panel order at the search's own point of an estimate (source_ref.search_point)."""
    p1, p2, a = sr.search_point(pc, pc2, alpha, heter)
    cn = Counts(d, dtype)
    return panel_order(cn, d.num_marker, marginals(cn, p1, p2, a))


def pair(target, partner):
    """(K [4], shared, bound sums [4]) of one ordered pair of (q, h, t) rows; bound sum = sum (1 + |log v_m|), v the
    floored mixture: the unit of the float32 evaluation's error bound."""
    q, _, t = target
    h = partner[1]
    T = q.dtype.type
    both = (q.sum(axis=1) > 0) & (h.sum(axis=1) > 0)
    hb = h[both].astype(T)
    d2, d1 = (q[both] * hb).sum(axis=1), (t[both] * hb).sum(axis=1)
    K, bound = np.zeros(4, dtype=T), np.zeros(4)
    for r, (k0, k1, k2) in enumerate(COEF):
        lg = np.log(np.maximum(T(k0) + T(k1) * d1 + T(k2) * d2, T(DOT_FLOOR)))
        K[r], bound[r] = lg.sum(), float((1 + np.abs(lg)).sum())
    return K, int(both.sum()), bound


def relations(rows_):
    """(K [n, n, 4] -- NaN on the diagonal --, shared [n, n], bound sums [n, n, 4]) of rows_ = [(q, h, t), ...]; None = a
    sample without a row (NaN row and column)."""
    n = len(rows_)
    K, sh, bs = np.full((n, n, 4), np.nan), np.zeros((n, n), dtype=np.int64), np.zeros((n, n, 4))
    for i in range(n):
        for j in range(n):
            if i == j or rows_[i] is None or rows_[j] is None:
                continue
            K[i, j], sh[i, j], bs[i, j] = pair(rows_[i], rows_[j])
    return K, sh, bs


# ---- seeded families on one panel (source_ref's recipe for the panel and the reads) ----

def gamete(g, rng):
    """One allele per marker from genotypes g [M]: the alternate allele with probability g / 2 (markers unlinked)."""
    return (rng.random(g.shape[0]) < g / 2.0).astype(np.int64)


FAMILY = ("A", "A2", "child", "sib", "grandchild", "B", "U", "V")
# the true relationship of the related pairs of FAMILY (by index, unordered); every other pair is unrelated
TRUE = {(0, 1): "DUP", (0, 2): "PO", (0, 3): "PO", (1, 2): "PO", (1, 3): "PO", (2, 3): "FS", (2, 4): "PO", (0, 4): "D2",
        (1, 4): "D2", (3, 4): "D2"}


def make_family(panel, mean_depth, seed, alpha_dup=0.03, known_af=False):
    """Eight samples of FAMILY on `panel`: an individual A, its second library A2 contaminated at alpha_dup by an
    outsider, a child of A and a spouse outside the cohort, a sib of the child (the same parents), a grandchild (the child
    and another outsider), and three unrelated individuals.  Returns (samples, alphas drawn at)."""
    rng = np.random.default_rng(seed)
    G = sr.draw_individuals(panel, 7, seed=seed + 1)         # A, spouse, in-law, contaminant, B, U, V
    a, spouse, inlaw, foreign = G[0], G[1], G[2], G[3]
    child = gamete(a, rng) + gamete(spouse, rng)
    sib = gamete(a, rng) + gamete(spouse, rng)
    grandchild = gamete(child, rng) + gamete(inlaw, rng)
    geno = [a, a, child, sib, grandchild, G[4], G[5], G[6]]
    alphas = [0.0, alpha_dup, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    data = [sr.make_sample(panel, g, foreign, mean_depth, al, seed + 10 + i, known_af=known_af)
            for i, (g, al) in enumerate(zip(geno, alphas))]
    return data, alphas
