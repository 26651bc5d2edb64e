"""Numpy restatement of the likelihood given a hypothesised contaminant (what vb2_conditioned_eval
computes on the device), from the reference's model (ContaminationEstimator.h:186-192, 285-311) in the notation of
source_ref:

    L_m(pc1, pc2, alpha | h) = sum_g1 P[g1] sum_g2 GF2[g2] W[g1][g2]
        P = pi_h[m]          where the hypothesis's triple of the marker is not all zero
        P = GF1(pc1)[m]      where it is
    LLK(. | h) = sum_m log L_m   over the markers with L_m > 0

Like deriv_ref and source_ref, every function takes the precision it works in from its Counts: np.float64 is the kernel's,
np.longdouble the reference the kernel tests measure against.  The prior is the float32 values the device gets, widened.
"""
import numpy as np

from deriv_ref import Counts, _gf, _table


def marker_log_l(c, prior, pc1, pc2, alpha):
    """(log L_m [n], live [n]) over the counted markers of `c` (a Counts), in its precision.  prior: [M, 3] in panel
    order (float32 values), or None = the all-zero hypothesis."""
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
    P = _gf(af1, True, T)[0]
    G2 = _gf(af2, True, T)[0]
    if prior is not None:
        pr32 = np.asarray(prior, dtype=np.float32)[c.idx]
        given = np.any(pr32 != 0, axis=1)
        P = np.where(given[:, None], pr32.astype(T), P)
    A = A.reshape(-1, 3, 3)
    # whether a marker counts is the reference's rule on its double L (h:310)
    f64 = np.float64
    with np.errstate(under="ignore"):
        lk64 = np.einsum("ma,mab,mb->m", P.astype(f64), np.exp(A.astype(f64)), G2.astype(f64))
        lk = np.einsum("ma,mab,mb->m", P, np.exp(A), G2)
    live = (lk64 > 0) & (lk > 0)
    ll = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    assert ll.dtype == np.dtype(T)
    return ll, live


def llk(c, prior, pc1, pc2, alpha):
    """LLK(pc1, pc2, alpha | h) in the precision of `c`."""
    if not (0.0 <= float(alpha) <= 1.0):
        return c.dtype(0)                 # a negative table entry: no marker counts (as vb2_llk_eval_batch)
    out = marker_log_l(c, prior, pc1, pc2, alpha)[0].sum()
    assert out.dtype == np.dtype(c.dtype)
    return out


class Evaluator:
    """evaluate(num_point, pc1, pc2, alpha) of conditioned_with_evaluator over the restatement: hypothesis h is
    (counts[h], priors[h]); counts[h] = None: a sample that counts no marker (every value 0.0).  Keeps what it was called
    with."""

    def __init__(self, counts, priors):
        self.counts, self.priors, self.calls = list(counts), list(priors), []

    def __call__(self, num_point, pc1, pc2, alpha):
        self.calls.append((num_point.copy(), pc1.copy(), pc2.copy(), alpha.copy()))
        out, p = [], 0
        for h, n in enumerate(num_point):
            for _ in range(int(n)):
                c = self.counts[h]
                out.append(0.0 if c is None else float(llk(c, self.priors[h], pc1[p], pc2[p], alpha[p])))
                p += 1
        return np.array(out, dtype=np.float64)


def search(counts, priors, pc1_fixed, known_af=False, **model_kw):
    """The refits on the float64 restatement through the host seam; (estimates, the Evaluator)."""
    import verifybamid_amd as vb
    ev = Evaluator(counts, priors)
    k = next(c.k for c in ev.counts if c is not None)
    return vb.conditioned_with_evaluator(ev, len(ev.counts), k, pc1_fixed, known_af=known_af, **model_kw), ev


# ---- a seeded cohort in which one source is known (tests/test_conditioned_cpu.py confirms the seed, the GPU suite runs it) ----

FIT_SEED = 42


def fit_cohort(seed=FIT_SEED, M=3000, depth=30, n=8, k=2):
    """(panel, samples): sample 0 contaminated at 5 % by sample 1's individual, sample 2 at 5 % by an outsider, the rest
    clean (1e-3 of the outsider); the samples as a run through the files sees them (depth filter on)."""
    import source_ref as sr
    panel = sr.make_panel(M, k, seed=seed)
    G = sr.draw_individuals(panel, n + 1, seed=seed + 1)
    plan = {0: (1, 0.05), 2: (n, 0.05)}
    from verifybamid_amd import synth
    data = [sr.make_sample(panel, G[i], G[plan.get(i, (n, 1e-3))[0]], depth, plan.get(i, (n, 1e-3))[1], seed + 10 + i)
            for i in range(n)]
    # with the depth statistics and the +-3 sd marker filter of a run through the files
    return panel, [synth.with_sanity_stats(d) for d in data]


def expected_refit(data, estimates, i):
    """What --RefitSource should give for sample i, on the restatements: the source scores of row i from the samples' float32
    rows at `estimates` (one dict per sample: pc, pc2, alpha of the default model), the best candidate, and -- where its
    score is > 0 -- the float64 refit given it.  dict(candidate, llr, alpha_given, lk1_given, delta_lk); the last three None
    without a refit."""
    import source_ref as sr
    e = estimates[i]
    c_i = sr.sample_rows(data[i], e["pc"], e["pc2"], e["alpha"])[0].astype(np.float32).astype(np.float64)
    qs, scores = {}, {}
    for j, d in enumerate(data):
        if j == i:
            continue
        ej = estimates[j]
        qs[j] = sr.sample_rows(d, ej["pc"], ej["pc2"], ej["alpha"])[1].astype(np.float32)
        scores[j] = float(sr.score(c_i, qs[j].astype(np.float64))[0])
    best = max(scores, key=scores.get)
    out = dict(candidate=best, llr=scores[best], alpha_given=None, lk1_given=None, delta_lk=None)
    if scores[best] > 0:
        pc1 = sr.search_point(e["pc"], e["pc2"], e["alpha"])[0]
        est, _ = search([Counts(data[i])], [qs[best]], pc1[None])
        out.update(alpha_given=est[0]["alpha"], lk1_given=est[0]["llk1"], delta_lk=e["llk1"] - est[0]["llk1"])
    return out
