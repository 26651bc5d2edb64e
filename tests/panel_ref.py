"""A-posteriori checker of the --RefVCF panel builder (panel_kernels.hip, panel.cpp).

A symmetric eigendecomposition can be verified from its own output: with the centred Gram C known exactly, the residual
C v - lambda v, the defect of V^T V - I and the trace say how good (sigma, V) are without choosing a sign or a basis of a
degenerate subspace, and the projection is checked by feeding the checker the V that the builder itself returned.

Precision.  np.float64 is the builder's own precision.  Everything that is measured here is computed in np.longdouble
(the x87 80-bit format on x86-64, 64 bits of mantissa) from exact integers (S = G^T G in int64) and the exact binary32
mu.  Nothing here calls BLAS for longdouble (numpy's matmul falls back to its own loops), and every measure asserts its
dtype so that a silent drop to double would show.  The float64 restatement (restate) is NOT the truth: it is the
yardstick for the allowances, the same quantities measured on a float64 pipeline in another order.

Allowances (u = 2^-53).  There are three, and none is taken from the result under test:
  * projection, rigorous: |ud - ref| <= (N + 2) u cond, cond = sum_j |g_jm| |V_jq| + |mu_m| sum_j |V_jq| (a sequential sum of
    N terms, one product, one subtraction; g V is exact for g in {-1, 0, 1, 2});
  * projection, customary: 32 u cond, what this project grants a correctly rounded evaluation in another order;
  * residual, orthonormality, spectrum: 32 x the same quantity measured on the float64 restatement of the same G.  The
    floors below are lower limits of those allowances; they decide where the restatement's own value is 0 (C = 0, N = 1)
    or, by luck of cancellation, next to it (the trace is a sum of N signed errors):
      residual, spectrum, trace, order:  s = u (N 4M + ||C||_2), one rounding of the largest intermediate in every entry
                                         (|S_ij|, |c_j| and tau are all <= 4M);
      orthonormality:                    N u.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit format here: the checker would measure nothing"
U = 2.0 ** -53
MARGIN = 32.0           # over the float64 restatement, and over u * cond in the projection
RATIOS = ("proj_rigorous", "proj", "resid", "ortho", "trace", "spec", "order")


class PanelMismatch(AssertionError):
    """A check failed; .quantity names it (one of the exact checks, or one of RATIOS)."""

    def __init__(self, quantity, message):
        AssertionError.__init__(self, "%s: %s" % (quantity, message))
        self.quantity = quantity


def _need(ok, quantity, message):
    if not ok:
        raise PanelMismatch(quantity, message)


def num_pcs(num_svd_pcs, M, N):
    return int(min(num_svd_pcs if num_svd_pcs > 0 else min(M, N), M, N))


def binary32_mean(G):
    """mu as mu_from_sums_kernel defines it: the FP64 quotient of the integer row sum and N, rounded to binary32 (that
    is the correctly rounded binary32 quotient), widened."""
    G = np.asarray(G)
    s = G.astype(np.int64).sum(axis=1)
    return (s.astype(np.float64) / np.float64(G.shape[1])).astype(np.float32).astype(np.float64)


def exact_centred_gram(G):
    """mu (binary32, widened), C = S - c 1^T - 1 c^T + tau in longdouble from exact integers, S = G^T G in int64.  The
    -1 entries stay in the matrix, as in the reference."""
    G = np.asarray(G)
    Gi = G.astype(np.int64)
    mu = binary32_mean(G)
    S = Gi.T @ Gi
    mul = mu.astype(LD)
    c = G.T.astype(LD) @ mul
    tau = (mul * mul).sum()
    C = ((S.astype(LD) - c[:, None]) - c[None, :]) + tau
    assert S.dtype == np.int64 and c.dtype == LD and C.dtype == LD and np.asarray(tau).dtype == LD
    return mu, C, S


# ---- seeded genotypes

def random_geno(M, N, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(M, N), p=[0.05, 0.45, 0.3, 0.2])


def structured_geno(M, N, seed):
    """-1/0/1/2 with two sample groups of different allele frequencies (separated top eigenvalues), 5 % missing."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=(M, 2))
    grp = (np.arange(N) >= N // 2).astype(np.int64)
    g = rng.binomial(2, f[:, grp]).astype(np.int8)
    g[rng.random((M, N)) < 0.05] = -1
    return g


# ---- the float64 restatement: ProcessRefVCF + ComputeSvdGram in numpy, piece by piece (the CPU tests plant faults
# ---- between the pieces)

def restate_gram(G, mu=None):
    """float64 BLAS: S (exact here, |entries| <= 4 M < 2^53), c, tau and the centred Gram."""
    G = np.asarray(G)
    mu = binary32_mean(G) if mu is None else mu
    Gf = G.astype(np.float64)
    S = Gf.T @ Gf
    c = Gf.T @ mu
    tau = mu @ mu
    return mu, S, c, tau


def centre(S, c, tau):
    return ((S - c[:, None]) - c[None, :]) + tau


def restate_eig(C, k, uplo="L"):
    """eigh (of the triangle `uplo`, the lower one as the builder's solver), descending; sigma = sqrt(max(w, 0)); the
    sign convention (the entry of largest magnitude positive).  Returns sigma (all N), V (N x k, signed), and V before
    the sign step."""
    w, Uu = np.linalg.eigh(C, UPLO=uplo)
    sigma = np.sqrt(np.maximum(w[::-1], 0.0))
    raw = Uu[:, ::-1][:, :k].copy()
    V = raw.copy()
    for q in range(k):
        j = int(np.argmax(np.abs(V[:, q])))
        if V[j, q] < 0:
            V[:, q] = -V[:, q]
    return sigma, V, raw


def column_sums(V):
    """1^T V as panel.cpp sums it: samples ascending."""
    s = np.zeros(V.shape[1], dtype=V.dtype)
    for j in range(V.shape[0]):
        s = s + V[j]
    return s


def project_in_kernel_order(G, mu, V, vsum=None, dtype=np.float64, samples=None):
    """UD = G V - mu (1^T V) as project_kernel evaluates it: one accumulator per entry, samples ascending, then
    acc - mu * vsum; in `dtype`."""
    G = np.asarray(G)
    T = np.dtype(dtype).type
    Vt = V.astype(T)
    vsum = column_sums(V) if vsum is None else vsum
    acc = np.zeros((G.shape[0], V.shape[1]), dtype=T)
    for j in range(G.shape[1] if samples is None else samples):
        acc = acc + G[:, j].astype(T)[:, None] * Vt[j][None, :]
    return (acc - mu.astype(T)[:, None] * vsum.astype(T)[None, :]).astype(np.float64)


def restate(G, num_svd_pcs):
    """A result dict shaped like the builder's, from the float64 pipeline."""
    G = np.asarray(G)
    M, N = G.shape
    k = num_pcs(num_svd_pcs, M, N)
    mu, S, c, tau = restate_gram(G)
    sigma, V, _ = restate_eig(centre(S, c, tau), k)
    return dict(ud=project_in_kernel_order(G, mu, V), v=V, mu=mu, sigma=sigma, gram=np.rint(S).astype(np.int64),
                row_sum=G.astype(np.int64).sum(axis=1), num_pc=k)


# ---- the measures

def projection_reference(G, mu, V):
    """ref = (G - mu 1^T) V and cond = |G| |V| + |mu| sum_j |V_j|, both in longdouble, for the V given."""
    G = np.asarray(G)
    Vl = V.astype(LD)
    A = G.astype(LD) - mu.astype(LD)[:, None]
    ref = A @ Vl
    aV = np.abs(Vl)
    cond = np.abs(G).astype(LD) @ aV + np.abs(mu).astype(LD)[:, None] * aV.sum(axis=0)[None, :]
    assert ref.dtype == LD and cond.dtype == LD
    return ref, cond


def _argmax(a):
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(a)), a.shape))


def eigen_measures(C, w, sigma, v):
    """Residual, orthonormality defect, trace and spectrum errors of (sigma, v) against the exact C (longdouble) and
    w = the clamped eigenvalues of the float64-rounded C, descending.  Returns {name: (value, entry)}."""
    N, k = v.shape
    Vl = v.astype(LD)
    lam = sigma.astype(LD) ** 2
    CV = C @ Vl
    R = CV - Vl * lam[None, :k]
    resid = np.sqrt((R * R).sum(axis=0))
    rayleigh = (Vl * CV).sum(axis=0)
    order = np.abs(rayleigh - lam[:k])
    O = np.abs(Vl.T @ Vl - np.eye(k, dtype=LD))
    trace = np.abs(lam.sum() - np.trace(C))
    spec = np.abs(lam - w.astype(LD))
    for a in (resid, order, O, trace, spec):
        assert np.asarray(a).dtype == LD
    return dict(resid=(float(resid.max()), _argmax(resid)), order=(float(order.max()), _argmax(order)),
                ortho=(float(O.max()), _argmax(O)), trace=(float(trace), ()), spec=(float(spec.max()), _argmax(spec)))


def check_panel(G, r, num_svd_pcs):
    """Check a result dict of the builder (or of restate) for G.  The exact checks raise PanelMismatch; the rest comes
    back as a record: rec[name] for name in RATIOS is the measured value divided by its allowance (inside: <= 1),
    rec["where"][name] the entry, rec["value"], rec["allow"] and rec["ref"] the measured value, the allowance and the
    float64 restatement's own value.  assert_inside(rec) raises on the first ratio above 1."""
    G = np.asarray(G)
    M, N = G.shape
    k = num_pcs(num_svd_pcs, M, N)
    mu, C, S = exact_centred_gram(G)

    # exact equalities
    ud, v, sigma = np.asarray(r["ud"]), np.asarray(r["v"]), np.asarray(r["sigma"])
    _need(ud.shape == (M, k) and v.shape == (N, k) and sigma.shape == (N,), "shape",
          "ud %s v %s sigma %s for M %d N %d k %d" % (ud.shape, v.shape, sigma.shape, M, N, k))
    _need(ud.dtype == np.float64 and v.dtype == np.float64 and sigma.dtype == np.float64, "shape", "not float64")
    rmu = np.ascontiguousarray(r["mu"], dtype=np.float64)
    bad = np.nonzero(rmu.view(np.uint64) != mu.view(np.uint64))[0] if rmu.shape == mu.shape else [-1]
    _need(len(bad) == 0, "mu", "%d markers differ from the binary32 mean, first at %d" % (len(bad), bad[0] if len(bad) else 0))
    _need(np.array_equal(np.asarray(r["row_sum"]).astype(np.int64), G.astype(np.int64).sum(axis=1)), "row_sum", "differs")
    gd = np.asarray(r["gram"]).astype(np.int64) != S
    _need(not gd.any(), "gram", "%d entries differ, first at %s" % (int(gd.sum()), _argmax(gd)))
    _need(np.isfinite(sigma).all() and (sigma >= 0).all(), "sigma", "not finite or negative")
    _need((np.diff(sigma) <= 0).all(), "sigma", "not non-increasing at %s" % (np.nonzero(np.diff(sigma) > 0)[0][:1],))
    _need(np.isfinite(v).all() and np.isfinite(ud).all(), "finite", "v or ud holds a non-finite value")

    # sign: some entry of largest magnitude is positive (which one, on ties, is not reproducible)
    for q in range(k):
        a = np.abs(v[:, q])
        _need((v[a == a.max(), q] > 0).any(), "sign", "column %d: its entry of largest magnitude is not positive" % q)

    rec = dict(M=M, N=N, k=k, where={}, value={}, allow={}, ref={})

    def put(name, value, allow, where, ref=None):
        rec["value"][name], rec["allow"][name], rec["where"][name], rec["ref"][name] = value, allow, where, ref
        rec[name] = value / allow if allow > 0 else (0.0 if value == 0 else np.inf)

    # projection, with the result's own V
    ref, cond = projection_reference(G, mu, v)
    err = np.abs(ud.astype(LD) - ref)
    zero = cond == 0
    _need(not (ud[zero] != 0).any(), "proj_zero", "ud is not exactly 0 where its condition sum is 0")
    ratio = np.where(zero, LD(0), err / np.where(zero, LD(1), cond)) / LD(U)
    assert ratio.dtype == LD
    worst = _argmax(ratio) if ratio.size else ()
    top = float(ratio.max()) if ratio.size else 0.0
    put("proj_rigorous", top, float(N + 2), worst)
    put("proj", top, MARGIN, worst)

    # eigenpairs against the exact C; allowances from the float64 restatement of the same G
    C64 = C.astype(np.float64)
    w = np.maximum(np.linalg.eigvalsh(C64)[::-1], 0.0)
    norm2 = float(np.linalg.norm(C64, 2))
    s = U * (N * 4.0 * M + norm2)
    floors = dict(resid=s, order=s, trace=s, spec=s, ortho=N * U)
    rmu_, rS, rc, rtau = restate_gram(G)
    rsigma, rV, _ = restate_eig(centre(rS, rc, rtau), k)
    got = eigen_measures(C, w, sigma, v)
    own = eigen_measures(C, w, rsigma, rV)
    for name in ("resid", "ortho", "trace", "spec", "order"):
        yard = own["resid" if name == "order" else name][0]         # the order check shares the residual's allowance
        put(name, got[name][0], max(MARGIN * yard, floors[name]), got[name][1], own[name][0])
    rec["scale"] = dict(s=s, norm2=norm2, u=U)
    return rec


def assert_inside(rec):
    for name in RATIOS:
        _need(rec[name] <= 1.0, name, "%.3g of its allowance (value %.3g, allowed %.3g, the float64 restatement's own %s) "
              "at entry %s; M %d N %d k %d" % (rec[name], rec["value"][name], rec["allow"][name], rec["ref"][name],
                                                rec["where"][name], rec["M"], rec["N"], rec["k"]))


def ratios_line(rec):
    return "  ".join("%s %.3g" % (n, rec[n]) for n in RATIOS)
