"""Numpy restatement of the error-rate fit's two computations (vb2_abi.h section 3h): the
log-likelihood under an error table eps[94] and the E-step's per-quality statistics (n, s), from the reference's expressions
(ContaminationEstimator.h: table entries h:223-225, genotype priors h:186-192, AF = (UD pc + mean) / 2 h:251-267, markers
counted where L > 0 h:310, the +-3 sd depth filter h:239-249).

It builds on deriv_ref.Counts' conventions -- the same classification, the same quality rows (those of the class ref / alt
reads), the same order of every floating-point operation of the log-likelihood, so that under the nominal table llk() IS
deriv_ref's value, bit for bit -- and keeps its own counts, because the statistics need the class-other reads per quality
as well: a class-other read is an error for certain.

Every function takes the precision of its Counts: np.float64 is the kernel's own, np.longdouble (80-bit on x86-64) the
reference the kernel tests measure against.
"""
import numpy as np

import deriv_ref as dr
import verifybamid_amd as vb

NUM_QUAL = 94


def nominal(T=np.float64):
    """eps0 in the precision T: deriv_ref's pErr (for float64 the bits of pow(10.0, q / -10.0))."""
    return dr._consts(np.dtype(T).type)[0]


class Counts(dr.Counts):
    """deriv_ref.Counts, and per class-other read of a counted marker its marker (index into the counted ones) and clamped
    quality; `other` is recomputed per table (other_sum)."""

    def __init__(self, d, dtype=np.float64):
        super().__init__(d, dtype)
        off = np.asarray(d.read_off, dtype=np.int64)
        depth = np.diff(off)
        M = depth.shape[0]
        mk = np.repeat(np.arange(M), depth)
        bases = np.asarray(d.bases)[off[0]:off[-1]]
        alt = np.asarray(d.alt_base)[mk]
        cls = np.where((bases == ord(".")) | (bases == ord(",")), 0, np.where((bases & 0xDF) == (alt & 0xDF), 1, 2))
        q = np.clip(np.asarray(d.quals)[off[0]:off[-1]].astype(np.int64) - 33, 0, 93)
        self.num_marker = M
        self.other_mk = mk[cls == 2]                          # panel index of every class-other read, in read order
        self.other_q = q[cls == 2]
        pos = np.full(M, -1, dtype=np.int64)
        pos[self.idx] = np.arange(len(self.idx))
        self.pos = pos                                        # panel index -> index among the counted markers, or -1
        self.depth = depth[self.idx]

    def other_sum(self, err):
        """deriv_ref's `other` under a table: per counted marker the sum of log(2/3 eps_q) over its class-other reads, added
        in read order."""
        T = self.dtype
        other = np.zeros(self.num_marker, dtype=T)
        with np.errstate(divide="ignore"):
            np.add.at(other, self.other_mk, np.log(T(2) / T(3) * err[self.other_q]))
        return other[self.idx]


def _err(c, err):
    e = np.asarray(err)
    assert e.shape == (NUM_QUAL,)
    return e.astype(c.dtype)


def _table(err, alpha, quals, T):
    """p and its error part M_E eps per (class, quality of `quals`) x (g1, g2): [2 len(quals), 9] each (deriv_ref._table's
    expression order)."""
    _, cerr, ok = dr._consts(T)
    alpha = T(alpha)
    one = T(1)
    e = err[quals][None, :, None, None]
    err1, err2 = cerr[:, None, :, None], cerr[:, None, None, :]
    ok1, ok2 = ok[:, None, :, None], ok[:, None, None, :]
    me = (alpha * err1 + (one - alpha) * err2) * e
    p = me + (alpha * ok1 + (one - alpha) * ok2) * (one - e)
    n = 2 * len(quals)
    return p.reshape(n, 9), np.broadcast_to(me, p.shape).reshape(n, 9)


def _markers(c, err, pc1, pc2, alpha):
    """Per counted marker: log L (0 where it does not count), whether it counts, the posterior w [.., 9] over the genotype
    pairs (rows of zeros where it does not count), and the table."""
    T = c.dtype
    err = _err(c, err)
    p, me = _table(err, alpha, c.quals, T)
    with np.errstate(divide="ignore"):
        logp = np.log(p)
    finite = np.isfinite(logp)
    A = c.N @ np.where(finite, logp, T(0)) + c.other_sum(err)[:, None]
    A = np.where(c.N @ (~finite).astype(T) > 0, T(-np.inf), A)
    if c.kaf is not None:
        af1 = af2 = c.kaf
    else:
        af1 = (c.ud @ np.asarray(pc1, dtype=np.float64).astype(T) + c.mu) / T(2)
        af2 = (c.ud @ np.asarray(pc2, dtype=np.float64).astype(T) + c.mu) / T(2)
    fixed = c.kaf is not None
    G1 = dr._gf(af1, fixed, T)[0]
    G2 = dr._gf(af2, fixed, T)[0]
    A = A.reshape(-1, 3, 3)
    f64 = np.float64
    # whether a marker counts is the reference's rule on its double L (h:310)
    with np.errstate(under="ignore"):
        lk64 = np.einsum("ma,mab,mb->m", G1.astype(f64), np.exp(A.astype(f64)), G2.astype(f64))
        lk = np.einsum("ma,mab,mb->m", G1, np.exp(A), G2)
        amax = np.max(A.reshape(-1, 9), axis=1)
        amax = np.where(np.isfinite(amax), amax, T(0))
        W = np.exp(A - amax[:, None, None])
    Ls = np.einsum("ma,mab,mb->m", G1, W, G2)
    live = (lk64 > 0) & (lk > 0) & (Ls > 0)
    logl = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = G1[:, :, None] * W * G2[:, None, :] / np.where(live, Ls, T(1))[:, None, None]
    w = np.where(live[:, None, None], w, T(0)).reshape(-1, 9)
    assert logl.dtype == np.dtype(T) and w.dtype == np.dtype(T)
    return logl, live, w, p, me


def llk(c, err, pc1, pc2, alpha):
    """sum log L over the markers that count, in the precision of `c`."""
    return _markers(c, err, pc1, pc2, alpha)[0].sum()


def read_posteriors(c, err, pc1, pc2, alpha):
    """r per (counted marker, class ref / alt x quality of c.quals): [.., 2 nq]; and which markers count."""
    T = c.dtype
    _, live, w, p, me = _markers(c, err, pc1, pc2, alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where(p != 0, me / np.where(p != 0, p, T(1)), T(0))      # a term whose denominator is 0 is 0
    return w @ R.T, live


def stats(c, err, pc1, pc2, alpha):
    """(n [94] int64, s [94] in the precision of `c`): per clamped quality the reads of the markers that count, all three
    classes, and the sum of their r; a class-other read has r = 1."""
    T = c.dtype
    r, live = read_posteriors(c, err, pc1, pc2, alpha)
    nq = len(c.quals)
    n = np.zeros(NUM_QUAL, dtype=np.int64)
    s = np.zeros(NUM_QUAL, dtype=T)
    Nl = c.N[live]
    cnt = Nl.sum(axis=0)
    exp = (Nl * r[live]).sum(axis=0)
    for cl in range(2):
        np.add.at(n, c.quals, np.rint(cnt[cl * nq:(cl + 1) * nq].astype(np.float64)).astype(np.int64))
        np.add.at(s, c.quals, exp[cl * nq:(cl + 1) * nq])
    pos = c.pos[c.other_mk]
    keep = pos >= 0
    keep[keep] = live[pos[keep]]
    oq = np.bincount(c.other_q[keep], minlength=NUM_QUAL).astype(np.int64)
    n += oq
    s += oq.astype(T)
    assert s.dtype == np.dtype(T)
    return n, s


def counted_reads(c, err, pc1, pc2, alpha):
    """The reads of the markers that count at the point."""
    live = _markers(c, err, pc1, pc2, alpha)[1]
    return int(c.depth[live].sum())


class Evaluator:
    """The two callbacks of vb.errfit_with_evaluator over a Counts."""

    def __init__(self, d_or_counts, dtype=np.float64):
        self.c = d_or_counts if isinstance(d_or_counts, Counts) else Counts(d_or_counts, dtype)
        self.num_eval = 0

    def eval(self, err, pc1, pc2, alpha):
        pc1, pc2 = np.atleast_2d(pc1), np.atleast_2d(pc2)
        alpha = np.atleast_1d(alpha)
        self.num_eval += len(alpha)
        return np.array([float(llk(self.c, err, pc1[i], pc2[i], alpha[i])) for i in range(len(alpha))])

    def stats(self, err, pc1, pc2, alpha):
        n, s = stats(self.c, err, pc1, pc2, alpha)
        return n, s.astype(np.float64)

    def nominal_estimate(self, num_pc, known_af, **model_kw):
        e0 = nominal()
        return vb.optimize_with_evaluator(lambda a, b, al: self.eval(e0, a, b, al), num_pc, known_af=known_af, **model_kw)

    def fit(self, num_pc, known_af, nominal_est=None, **kw):
        model_kw = {k: v for k, v in kw.items() if k not in ("prior_reads", "tol", "max_iter")}
        if nominal_est is None:
            nominal_est = self.nominal_estimate(num_pc, known_af, **model_kw)
        return vb.errfit_with_evaluator(self.eval, self.stats, num_pc, nominal_est, known_af=known_af, **kw), nominal_est


# ---- the read sampler: planted error rates per reported quality ----
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
_LOWER = np.frombuffer(b"acgt", dtype=np.uint8)
SAMPLE_QUALS = (20, 30, 37)


def sample(num_marker, seed, depth=30, alpha=0.03, quals=SAMPLE_QUALS, shift=5, num_pc=2, known_af=True):
    """Markers at allele frequencies ~ U(0.05, 0.95) (handed over as known), `depth` reads each, a share alpha from the
    contaminant; reported qualities drawn uniformly from `quals`; a read is an error with the rate of quality q - shift, an
    error shows one of the three other bases uniformly.  Returns (PileupData, planted [94] rates, NaN where no read has the
    quality)."""
    rng = np.random.default_rng(seed)
    M, k = int(num_marker), int(num_pc)
    af = rng.uniform(0.05, 0.95, size=M)
    ud = rng.normal(0.0, 1.0, size=(M, k))
    mu = 2.0 * af
    g2 = rng.binomial(2, af)
    g1 = rng.binomial(2, af)
    ref_i = rng.integers(0, 4, size=M)
    alt_i = (ref_i + rng.integers(1, 4, size=M)) % 4
    dep = np.full(M, int(depth), dtype=np.int64)
    read_off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(dep, out=read_off[1:])
    R = int(read_off[-1])
    mk = np.repeat(np.arange(M), dep)
    g = np.where(rng.random(R) < alpha, g1[mk], g2[mk])
    is_alt = rng.random(R) < (g / 2.0)
    q = np.asarray(quals)[rng.integers(0, len(quals), size=R)]
    planted = np.full(NUM_QUAL, np.nan)
    for qq in quals:
        planted[qq] = 10.0 ** (-(qq - shift) / 10.0)
    is_err = rng.random(R) < planted[q]
    true_base = np.where(is_alt, alt_i[mk], ref_i[mk])
    obs = np.where(is_err, (true_base + rng.integers(1, 4, size=R)) % 4, true_base)
    fwd = rng.random(R) < 0.5
    ch = np.where(fwd, _BASES[obs], _LOWER[obs])
    ch = np.where(obs == ref_i[mk], np.where(fwd, ord("."), ord(",")), ch).astype(np.uint8)
    d = vb.PileupData(k, ud, mu, read_off, ch, (q + 33).astype(np.uint8), _BASES[alt_i], af if known_af else None,
                      float(depth), 0.0, True, dict(seed=seed, alpha_true=alpha, ref_base=_BASES[ref_i]))
    return d, planted


def fit_sample(seed, num_marker=3000, shift=5, **kw):
    """The experiment of DESIGN.md section 23 on one seed: (fit dict, nominal estimate, planted rates, data)."""
    d, planted = sample(num_marker, seed, shift=shift)
    ev = Evaluator(d)
    fit, nom = ev.fit(d.num_pc, True, **kw)
    return fit, nom, planted, d
