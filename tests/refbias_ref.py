"""Numpy restatement of the likelihood under a reference bias (what
vb2_refbias_eval computes on the device), from the reference's model (ContaminationEstimator.h:164-177, 186-192, 223-225,
285-311) in the notation of deriv_ref, with beta = P(an error-free read of a heterozygous genotype shows REF) in place of
the constant 0.5:

    class ref:  u(g; e, beta) = (g/6) e     + {1, beta, 0}[g] (1 - e)
    class alt:  u(g; e, beta) = ((2-g)/6) e + {0, 1 - beta, 1}[g] (1 - e)
    p(read | g1, g2, alpha, beta) = (alpha e1 + (1 - alpha) e2) p_err + (alpha n1 + (1 - alpha) n2) p_ok
    L_m = sum_g1 GF1[g1] sum_g2 GF2[g2] W[g1][g2],   LLK = sum_m log L_m over the markers with L_m > 0

Like deriv_ref and conditioned_ref, every function takes the precision it works in from its Counts: np.float64 is the
kernel's, np.longdouble the reference the kernel tests measure against.  At beta = 0.5 the float64 values are the bits of
conditioned_ref.llk(c, None, ...).
"""
import numpy as np

from deriv_ref import Counts, _consts, _gf

BETA_MIN, BETA_MAX = 0.25, 0.75


def _table(alpha, beta, quals, T):
    """log p per (class, quality of `quals`) x (g1, g2): [2 len(quals), 9] (deriv_ref._table with the heterozygote's share)."""
    perr, err, _ = _consts(T)
    b = T(beta)
    one = T(1)
    ok = np.array([[one, b, T(0)], [T(0), one - b, one]], dtype=T)
    alpha = T(alpha)
    e = perr[quals][None, :, None, None]
    err1, err2 = err[:, None, :, None], err[:, None, None, :]
    ok1, ok2 = ok[:, None, :, None], ok[:, None, None, :]
    p = (alpha * err1 + (one - alpha) * err2) * e + (alpha * ok1 + (one - alpha) * ok2) * (one - e)
    with np.errstate(divide="ignore", invalid="ignore"):
        logp = np.log(p)
    return logp.reshape(2 * len(quals), 9)


def marker_log_l(c, beta, pc1, pc2, alpha):
    """(log L_m [n], live [n]) over the counted markers of `c` (a Counts), in its precision."""
    T = c.dtype
    logp = _table(alpha, beta, c.quals, T)
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
    live = (lk64 > 0) & (lk > 0)
    ll = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    assert ll.dtype == np.dtype(T)
    return ll, live


def llk(c, beta, pc1, pc2, alpha):
    """LLK(pc1, pc2, alpha; beta) in the precision of `c`."""
    assert BETA_MIN <= float(beta) <= BETA_MAX
    if not (0.0 <= float(alpha) <= 1.0):
        return c.dtype(0)                 # a negative table entry: no marker counts (as vb2_llk_eval_batch)
    out = marker_log_l(c, beta, pc1, pc2, alpha)[0].sum()
    assert out.dtype == np.dtype(c.dtype)
    return out


def exchanged(c):
    """The Counts of the sample with REF and ALT exchanged: the classes swapped and every allele frequency AF -> 1 - AF,
    through ud -> -ud and mu -> 2 - mu (or the known frequencies themselves).  llk(exchanged(c), beta, ...) =
    llk(c, 1 - beta, ...)."""
    import copy
    x = copy.copy(c)
    nq = len(c.quals)
    x.N = np.concatenate([c.N[:, nq:], c.N[:, :nq]], axis=1)
    x.ud = -c.ud
    x.mu = c.dtype(2) - c.mu
    x.kaf = None if c.kaf is None else c.dtype(1) - c.kaf
    return x


def het_bound(d):
    """The flatten's bound of a sample (context.cpp: FlattenTables::lhet): the largest number of binary orders of magnitude
    a counted marker's (het, het) term lies below 1 at beta = 0.5 -- what vb2_refbias_create holds against 450 on a
    probability-domain context."""
    c = Counts(d)
    perr = _consts(np.float64)[0][c.quals]
    cost = -np.log2(0.5 * (1 - perr) + perr / 6)
    nq = len(c.quals)
    per = (c.N[:, :nq] + c.N[:, nq:]) @ cost - c.other / np.log(2.0)
    return float(per.max())


class Evaluator:
    """evaluate(beta, num_point, pc1, pc2, alpha) of refbias_with_evaluator over the restatement on ONE Counts (None: a
    sample that counts no marker, every value 0.0).  Keeps what it was called with; fail_at: the call (0-based) that raises."""

    def __init__(self, counts, fail_at=None):
        self.counts, self.calls, self.fail_at = counts, [], fail_at

    def __call__(self, beta, num_point, pc1, pc2, alpha):
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError("the evaluator fails on purpose")
        self.calls.append((beta.copy(), num_point.copy(), pc1.copy(), pc2.copy(), alpha.copy()))
        out, p = [], 0
        for r, n in enumerate(num_point):
            for _ in range(int(n)):
                out.append(0.0 if self.counts is None else float(llk(self.counts, beta[r], pc1[p], pc2[p], alpha[p])))
                p += 1
        return np.array(out, dtype=np.float64)

    def lockstep_calls(self):
        """The row sets of the lock-step calls, in order: a new call begins where the rows change."""
        sets = []
        for b, *_ in self.calls:
            if not sets or not np.array_equal(sets[-1], b):
                sets.append(b)
        return sets


def search(c, betas, known_af=False, **model_kw):
    """The rows' refits on the restatement through the host seam of the replicates (the same driver with no side held):
    one dict per beta."""
    import verifybamid_amd as vb
    betas = np.asarray(betas, dtype=np.float64)

    def ev(num_point, pc1, pc2, alpha):
        out, p = [], 0
        for r, n in enumerate(num_point):
            for _ in range(int(n)):
                out.append(float(llk(c, betas[r], pc1[p], pc2[p], alpha[p])))
                p += 1
        return np.array(out)
    return vb.replicates_with_evaluator(ev, len(betas), c.k, known_af=known_af, **model_kw)


# ---- a read sampler with a planted bias (tests/test_refbias_cpu.py confirms the seeds, the GPU suite runs them) ----

FIT_SEED, NULL_SEED = 11, 12
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
_LOWER = np.frombuffer(b"acgt", dtype=np.uint8)


def make_sample(M, depth, k, alpha, beta, seed, q_lo=30, q_hi=30, known_af=False):
    """synth.make_pileup's recipe with one change: an error-free read of a heterozygous genotype carries the REF allele with
    probability beta.  The markers' allele frequencies are mu / 2 (the sample's true PCs are 0)."""
    import verifybamid_amd as vb
    rng = np.random.default_rng(seed)
    sd = np.array([(7.0, 5.0, 3.0, 1.5)[i] if i < 4 else 0.3 for i in range(k)])
    ud = rng.normal(0.0, 1.0, size=(M, k)) * sd
    mu = np.clip(2.0 * rng.beta(0.8, 0.8, size=M), 0.02, 1.98)
    af = mu / 2.0
    g2, g1 = rng.binomial(2, af), rng.binomial(2, af)
    n = rng.poisson(depth, size=M).astype(np.int64)
    ref_i = rng.integers(0, 4, size=M)
    alt_i = (ref_i + rng.integers(1, 4, size=M)) % 4
    read_off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(n, out=read_off[1:])
    R = int(read_off[-1])
    mk = np.repeat(np.arange(M), n)
    g = np.where(rng.random(R) < alpha, g1[mk], g2[mk])
    is_alt = rng.random(R) < np.where(g == 1, 1.0 - beta, g / 2.0)
    q = rng.integers(q_lo, q_hi + 1, size=R)
    err = rng.random(R) < np.power(10.0, -q / 10.0)
    true_base = np.where(is_alt, alt_i[mk], ref_i[mk])
    obs = np.where(err, (true_base + rng.integers(1, 4, size=R)) % 4, true_base)
    fwd = rng.random(R) < 0.5
    ch = np.where(fwd, _BASES[obs], _LOWER[obs])
    ch = np.where(obs == ref_i[mk], np.where(fwd, ord("."), ord(",")), ch).astype(np.uint8)
    nsite = int((n > 0).sum())
    return vb.PileupData(k, ud, mu, read_off, ch, (q + 33).astype(np.uint8), _BASES[alt_i], af.copy() if known_af else None,
                         float(R) / nsite, 0.0, True, dict(seed=seed, alpha_true=alpha, beta_true=beta, ref_base=_BASES[ref_i]))


def fit_sample(seed=FIT_SEED, beta=0.58):
    """The seeded 3 000 x 30, k = 2 sample of the fit tests: alpha = 0.03, q30 reads, the bias planted."""
    return make_sample(3000, 30, 2, 0.03, beta, seed)
