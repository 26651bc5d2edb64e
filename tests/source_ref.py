"""Numpy restatement of the source statistic (what vb2_ctx_marginals and vb2_source_set_scores
compute on the device), from the reference's model (ContaminationEstimator.h:186-192, 285-311).

Per counted marker, with W[g1][g2] = prod_reads P(read | g1, g2, alpha) (g1 the alpha-fraction, contaminating genotype,
g2 the intended one) and GF1, GF2 the genotype priors at the two allele frequencies:

    L     = sum GF1[g1] GF2[g2] W[g1][g2]
    c[g1] = (sum_g2 W[g1][g2] GF2[g2]) / L               sum_g1 GF1[g1] c[g1] = 1
    q[g2] = GF2[g2] (sum_g1 GF1[g1] W[g1][g2]) / L       sum q = 1

and S(i, j) = sum_m log max(c_i[m] . q_j[m], 1e-30) over the markers both samples count.

Like deriv_ref, every function takes the precision it works in from its Counts: np.float64 is the kernel's, np.longdouble
(64 bits of mantissa on x86-64) the reference the kernel tests measure against.
"""
import numpy as np

from deriv_ref import Counts, _gf, _table

DOT_FLOOR = 1e-30


def search_point(pc, pc2, alpha, heter=True):
    """The point the statistic is taken at, from an estimate as reported: the swap of indices 0 and 1 between the two
    samples' PCs (ContaminationEstimator.cpp:146-149: alpha >= 0.5, two-ancestry model) undone, then mirrored so that
    alpha < 0.5: L(pc1, pc2, a) = L(pc2, pc1, 1 - a)."""
    p1, p2 = np.array(pc, dtype=np.float64), np.array(pc2, dtype=np.float64)
    alpha = float(alpha)
    if heter and alpha >= 0.5:
        for j in range(min(2, len(p1))):
            p1[j], p2[j] = p2[j], p1[j]
    if alpha >= 0.5:
        p1, p2, alpha = p2, p1, 1.0 - alpha
    return p1, p2, alpha


def marginals(c, pc1, pc2, alpha):
    """dict(c [n, 3], q [n, 3], log_l [n], live [n], gf1, gf2) over the counted markers of `c` (a Counts), in its
    precision; rows of markers with L not > 0 are 0."""
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
    A = A.reshape(-1, 3, 3)
    # whether a marker counts is the reference's rule on its double L (h:310)
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
    cl = r * inv[:, None]
    q = G2 * s * inv[:, None]
    ll = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    cl[~live] = 0
    q[~live] = 0
    assert cl.dtype == np.dtype(T) and q.dtype == np.dtype(T) and ll.dtype == np.dtype(T)
    return dict(c=cl, q=q, log_l=ll, live=live, gf1=G1, gf2=G2)


def panel_order(c, num_marker, m):
    """(c [M, 3], q [M, 3], log_l [M]) in panel order, zeros for the markers the sample does not count."""
    T = c.dtype
    cl, q, ll = np.zeros((num_marker, 3), dtype=T), np.zeros((num_marker, 3), dtype=T), np.zeros(num_marker, dtype=T)
    cl[c.idx], q[c.idx], ll[c.idx] = m["c"], m["q"], m["log_l"]
    return cl, q, ll


def sample_rows(d, pc, pc2, alpha, heter=True, dtype=np.float64):
    """A sample's (c, q) in panel order at the search's own point of an estimate (search_point)."""
    p1, p2, a = search_point(pc, pc2, alpha, heter)
    cn = Counts(d, dtype)
    cl, q, _ = panel_order(cn, d.num_marker, marginals(cn, p1, p2, a))
    return cl, q


def score(c_i, q_j):
    """(S, shared, bound sum) of one pair: S = sum log max(c_i . q_j, 1e-30) over the markers with a non-zero triple on
    each side; bound sum = sum (1 + |log d_m|) over them, the unit of the float32 evaluation's error bound."""
    T = c_i.dtype.type
    both = (c_i.sum(axis=1) > 0) & (q_j.sum(axis=1) > 0)
    d = np.maximum((c_i[both] * q_j[both].astype(T)).sum(axis=1), T(DOT_FLOOR))
    lg = np.log(d)
    return lg.sum(), int(both.sum()), float((1 + np.abs(lg)).sum())


def score_matrix(rows):
    """score [n, n] (NaN on the diagonal), shared [n, n], bound sums [n, n] of rows = [(c, q), ...]; None = a sample
    without a row (NaN row and column)."""
    n = len(rows)
    S, sh, bs = np.full((n, n), np.nan), np.zeros((n, n), dtype=np.int64), np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i == j or rows[i] is None or rows[j] is None:
                continue
            S[i, j], sh[i, j], bs[i, j] = score(rows[i][0], rows[j][1])
    return S, sh, bs


# ---- seeded cohorts in which the true source is known (verifybamid_amd.synth's recipe) ----

def make_panel(num_marker, num_pc=2, seed=1):
    """A synthetic panel as synth.make_pileup draws it, and the allele frequencies its individuals come from (mu / 2:
    the ancestry at PC = 0)."""
    from verifybamid_amd import synth
    rng = np.random.default_rng(seed)
    M, k = int(num_marker), int(num_pc)
    sd = np.array([synth._SD[i] if i < len(synth._SD) else 0.3 for i in range(k)])
    ud = rng.normal(0.0, 1.0, size=(M, k)) * sd
    mu = np.clip(2.0 * rng.beta(0.8, 0.8, size=M), 0.02, 1.98)
    ref_i = rng.integers(0, 4, size=M)
    alt_i = (ref_i + rng.integers(1, 4, size=M)) % 4
    return dict(num_pc=k, ud=ud, mu=mu, af=np.clip(mu / 2.0, 0.00005, 0.99995), ref=synth._BASES[ref_i], alt=synth._BASES[alt_i])


def draw_individuals(panel, n, seed=1):
    """Genotypes [n, M] ~ Binom(2, AF)."""
    rng = np.random.default_rng(seed)
    return rng.binomial(2, panel["af"][None, :].repeat(n, 0))


def make_sample(panel, g_intended, g_contaminant, mean_depth, alpha, seed, known_af=False):
    """A PileupData of reads drawn from two individuals' genotypes (synth.reads_from_genotypes)."""
    from verifybamid_amd import synth
    from verifybamid_amd.api import PileupData
    off, b, q = synth.reads_from_genotypes(g_intended, g_contaminant, panel["ref"], panel["alt"], mean_depth, alpha, seed)
    depth = np.diff(off)
    nsite = int((depth > 0).sum())
    return PileupData(panel["num_pc"], panel["ud"], panel["mu"], off, b, q, panel["alt"], panel["af"] if known_af else None,
                      float(off[-1]) / max(nsite, 1), 0.0, True, dict(ref_base=panel["ref"]))
