"""Numpy restatement of the likelihood given genotype priors on both components (what vb2_paired_eval
computes on the device), from the reference's model (ContaminationEstimator.h:186-192, 285-311) in the notation of
source_ref and conditioned_ref:

    L_m(pc1, pc2, alpha | h) = sum_g1 P1[g1] sum_g2 P2[g2] W[g1][g2]
        P1 = pi1_h[m] where that triple is not all zero, else GF1(pc1)[m]
        P2 = pi2_h[m] where that triple is not all zero, else GF2(pc2)[m]
        a marker whose pi2_h[m][0] is negative is left out
    LLK(. | h) = sum_m log L_m   over the walked markers with L_m > 0

A hypothesis is [M, 6] in panel order (pi1 | pi2), the float32 values the device gets, widened.  Like deriv_ref, every
function takes the precision it works in from its Counts: np.float64 is the kernel's, np.longdouble the reference the kernel
tests measure against.

Also here: the matched-normal rule (normal_rule), the paired refit on the restatement through the host seam (search,
paired_fit) and seeded tumour-normal pairs with a planted allelic imbalance (make_tumour, pair_case).
"""
import numpy as np

from deriv_ref import Counts, _gf, _table

LEFT_OUT = np.array([-1.0, 0.0, 0.0], dtype=np.float32)


def hypothesis(M, pi1=None, pi2=None):
    """[M, 6] float32 from the two sides' [M, 3] (None: all zero)."""
    h = np.zeros((M, 6), dtype=np.float32)
    if pi1 is not None:
        h[:, :3] = pi1
    if pi2 is not None:
        h[:, 3:] = pi2
    return h


def marker_log_l(c, hyp, pc1, pc2, alpha):
    """(log L_m [n], live [n], walked [n]) over the counted markers of `c` (a Counts), in its precision.  hyp: [M, 6] in
    panel order, or None = both sides all zero."""
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
    P1 = _gf(af1, True, T)[0]
    P2 = _gf(af2, True, T)[0]
    walked = np.ones(len(c.idx), dtype=bool)
    if hyp is not None:
        h32 = np.asarray(hyp, dtype=np.float32)[c.idx]
        walked = ~(h32[:, 3] < 0)
        given1 = np.any(h32[:, :3] != 0, axis=1)
        given2 = np.any(h32[:, 3:] != 0, axis=1) & walked
        P1 = np.where(given1[:, None], h32[:, :3].astype(T), P1)
        P2 = np.where(given2[:, None], h32[:, 3:].astype(T), P2)
    A = A.reshape(-1, 3, 3)
    # whether a marker counts is the reference's rule on its double L (h:310)
    f64 = np.float64
    with np.errstate(under="ignore"):
        lk64 = np.einsum("ma,mab,mb->m", P1.astype(f64), np.exp(A.astype(f64)), P2.astype(f64))
        lk = np.einsum("ma,mab,mb->m", P1, np.exp(A), P2)
    live = (lk64 > 0) & (lk > 0) & walked
    ll = np.where(live, np.log(np.where(live, lk, T(1))), T(0))
    assert ll.dtype == np.dtype(T)
    return ll, live, walked


def llk(c, hyp, pc1, pc2, alpha):
    """LLK(pc1, pc2, alpha | h) in the precision of `c`."""
    if not (0.0 <= float(alpha) <= 1.0):
        return c.dtype(0)                 # a negative table entry: no marker counts (as vb2_llk_eval_batch)
    out = marker_log_l(c, hyp, pc1, pc2, alpha)[0].sum()
    assert out.dtype == np.dtype(c.dtype)
    return out


def diagonal_constants(c, g):
    """sum_m log W[g][g] over the counted markers: a homozygous pair reads alpha out (g = 0, 2: every read of the pair's
    allele p = 1 - e, of the other e / 3; g = 1 likewise without alpha), from the table at any alpha."""
    T = c.dtype
    logp, _ = _table(0.5, c.quals, T)
    A = c.N @ logp + c.other[:, None]
    return A.reshape(-1, 3, 3)[:, g, g].sum()


def normal_rule(q, hom_min):
    """The matched-normal hypothesis [M, 6] from a normal's genotype posterior q [M, 3] (float32, zeros where it counts
    nothing): pi1 all zero; pi2 = q where the triple is not all zero and max(q[0], q[2]) >= hom_min; the rest left out."""
    q = np.asarray(q, dtype=np.float32)
    keep = np.any(q != 0, axis=1) & (np.maximum(q[:, 0], q[:, 2]).astype(np.float64) >= float(hom_min))
    h = np.zeros((q.shape[0], 6), dtype=np.float32)
    h[:, 3:] = np.where(keep[:, None], q, LEFT_OUT[None, :])
    return h


def given_count(c, hyp):
    """The counted markers of `c` that the hypothesis does not leave out (vb2_paired_info_get's given[h])."""
    return int((~(np.asarray(hyp, dtype=np.float32)[c.idx, 3] < 0)).sum())


class Evaluator:
    """evaluate(num_point, pc1, pc2, alpha) of paired_with_evaluator over the restatement: hypothesis h is (counts[h],
    hyps[h]).  Keeps what it was called with."""

    def __init__(self, counts, hyps):
        self.counts, self.hyps, self.calls = list(counts), list(hyps), []

    def __call__(self, num_point, pc1, pc2, alpha):
        self.calls.append((num_point.copy(), pc1.copy(), pc2.copy(), alpha.copy()))
        out, p = [], 0
        for h, n in enumerate(num_point):
            for _ in range(int(n)):
                out.append(float(llk(self.counts[h], self.hyps[h], pc1[p], pc2[p], alpha[p])))
                p += 1
        return np.array(out, dtype=np.float64)


def search(counts, hyps, pc2_fixed, known_af=False, **model_kw):
    """The paired refits on the float64 restatement through the host seam; (estimates, the Evaluator)."""
    import verifybamid_amd as vb
    ev = Evaluator(counts, hyps)
    return vb.paired_with_evaluator(ev, len(ev.counts), ev.counts[0].k, pc2_fixed, known_af=known_af, **model_kw), ev


# ---- seeded tumour-normal pairs ----

def make_tumour(panel, g_tumour, g_contaminant, mean_depth, alpha, seed, shifted=None, ref_fraction=0.7):
    """source_ref.make_sample's scheme with an allelic imbalance: at the markers of `shifted` (bool [M]) where the tumour is
    heterozygous, a read of the tumour's own DNA shows the reference allele with probability ref_fraction, not one half (a
    copy-number gain or an impure loss of heterozygosity).  The contaminant's reads are drawn as ever."""
    from verifybamid_amd import synth
    from verifybamid_amd.api import PileupData
    rng = np.random.default_rng(seed)
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    ref_i = np.array([code[int(x)] for x in np.asarray(panel["ref"], dtype=np.uint8)])
    alt_i = np.array([code[int(x)] for x in np.asarray(panel["alt"], dtype=np.uint8)])
    g2, g1 = np.asarray(g_tumour), np.asarray(g_contaminant)
    M = g2.shape[0]
    alt_own = g2 / 2.0
    if shifted is not None:
        alt_own = np.where(np.asarray(shifted, dtype=bool) & (g2 == 1), 1.0 - ref_fraction, alt_own)
    depth = rng.poisson(mean_depth, size=M).astype(np.int64)
    off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(depth, out=off[1:])
    R = int(off[-1])
    mk = np.repeat(np.arange(M), depth)
    p_alt = np.where(rng.random(R) < alpha, g1[mk] / 2.0, alt_own[mk])
    is_alt = rng.random(R) < p_alt
    q = rng.integers(20, 41, size=R)
    err = rng.random(R) < np.power(10.0, -q / 10.0)
    true_base = np.where(is_alt, alt_i[mk], ref_i[mk])
    obs = np.where(err, (true_base + rng.integers(1, 4, size=R)) % 4, true_base)
    fwd = rng.random(R) < 0.5
    ch = np.where(fwd, synth._BASES[obs], synth._LOWER[obs])
    ch = np.where(obs == ref_i[mk], np.where(fwd, ord("."), ord(",")), ch).astype(np.uint8)
    nsite = int((depth > 0).sum())
    return PileupData(panel["num_pc"], panel["ud"], panel["mu"], off, ch, (q + 33).astype(np.uint8), panel["alt"], None,
                      float(off[-1]) / max(nsite, 1), 0.0, True, dict(ref_base=panel["ref"]))


PAIR_SEED = 42


def pair_case(seed=PAIR_SEED, M=3000, depth=30, k=2, alpha=0.03, share=0.5, ref_fraction=0.7):
    """(panel, tumour with the imbalance, the same individual's tumour without it, normal, another individual's normal):
    the tumours contaminated at `alpha` by an outsider, a `share` of the markers shifted; the normals clean (1e-3)."""
    import source_ref as sr
    panel = sr.make_panel(M, k, seed=seed)
    G = sr.draw_individuals(panel, 4, seed=seed + 1)        # 0: the patient, 1: the outsider, 2: another person, 3: noise
    shifted = np.random.default_rng(seed + 2).random(M) < share
    shifted_t = make_tumour(panel, G[0], G[1], depth, alpha, seed + 3, shifted, ref_fraction)
    plain_t = make_tumour(panel, G[0], G[1], depth, alpha, seed + 3, None)
    normal = sr.make_sample(panel, G[0], G[3], depth, 1e-3, seed + 4)
    stranger = sr.make_sample(panel, G[2], G[3], depth, 1e-3, seed + 5)
    return panel, shifted_t, plain_t, normal, stranger


def normal_q(normal, estimate=None):
    """The normal's genotype posterior as the device holds it: float32 [M, 3] at its search point (source_ref.sample_rows);
    estimate None: pc = pc2 = 0, alpha = 1e-3."""
    import source_ref as sr
    z = np.zeros(normal.num_pc)
    e = estimate or dict(pc=z, pc2=z, alpha=1e-3)
    return sr.sample_rows(normal, e["pc"], e["pc2"], e["alpha"])[1].astype(np.float32)


def paired_fit(tumour, q, pc2_fixed, hom_min=0.99, **model_kw):
    """The paired refit of one tumour on the float64 restatement: (estimate, given markers)."""
    c = Counts(tumour)
    hyp = normal_rule(q, hom_min)
    est, _ = search([c], [hyp], np.asarray(pc2_fixed, dtype=np.float64)[None], **model_kw)
    return est[0], given_count(c, hyp)


# ---- a seeded cohort with two tumour-normal pairs (tests/test_paired_cpu.py confirms the seed, the GPU suite runs it) ----

COHORT_PAIRS = [(0, 1), (2, 3)]
COHORT_PLANTED = {0: 0.03, 2: 0.05}


def pair_cohort(seed=PAIR_SEED, M=3000, depth=30, k=2):
    """(panel, samples): 0 a tumour contaminated at 3 % by an outsider with half its markers at a reference fraction of 0.7,
    1 its normal; 2 another patient's tumour at 5 % without imbalance, 3 its normal; 4, 5 bystanders; the samples as a run
    through the files sees them (depth filter on)."""
    import source_ref as sr
    from verifybamid_amd import synth
    panel = sr.make_panel(M, k, seed=seed)
    G = sr.draw_individuals(panel, 6, seed=seed + 1)        # 0, 1: the patients; 2: the outsider; 3: noise; 4, 5: bystanders
    shifted = np.random.default_rng(seed + 2).random(M) < 0.5
    data = [make_tumour(panel, G[0], G[2], depth, COHORT_PLANTED[0], seed + 10, shifted, 0.7),
            sr.make_sample(panel, G[0], G[3], depth, 1e-3, seed + 11),
            make_tumour(panel, G[1], G[2], depth, COHORT_PLANTED[2], seed + 12, None),
            sr.make_sample(panel, G[1], G[3], depth, 1e-3, seed + 13),
            sr.make_sample(panel, G[4], G[3], depth, 1e-3, seed + 14),
            sr.make_sample(panel, G[5], G[3], depth, 1e-3, seed + 15)]
    return panel, [synth.with_sanity_stats(d) for d in data]


def expected_pair(data, estimates, t, n, hom_min=0.99):
    """What --MatchedNormal should give for the pair (t, n), on the restatements: the normal's float32 q at its search point
    of `estimates` (one dict per sample: pc, pc2, alpha of the default model), the rule, and the float64 refit with pc2 held
    at the normal's intended PCs.  dict(markers, alpha_paired, lk1_paired, lk0_paired, freemix)."""
    import source_ref as sr
    e = estimates[n]
    q = normal_q(data[n], e)
    pc2 = sr.search_point(e["pc"], e["pc2"], e["alpha"])[1]
    est, given = paired_fit(data[t], q, pc2, hom_min)
    a = estimates[t]["alpha"]
    return dict(markers=given, alpha_paired=est["alpha"], lk1_paired=est["llk1"], lk0_paired=est["llk0"],
                freemix=min(a, 1 - a), status=est["status"])
