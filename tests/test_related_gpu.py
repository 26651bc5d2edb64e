"""--FindRelated on the MI355X (source_kernels.hip's related instantiation, related_kernels.hip) against the numpy
restatement (tests/related_ref.py).

Marginals (vb2_ctx_marginals_related): h and t per marker against the restatement in 80-bit floats, under the rule of the
derivative and source tests -- the worst relative deviation of an output must not exceed max(32 x dev64, 1e-13), dev64
being the float64 restatement's own worst relative deviation from the 80-bit one on the same sample and point, applied a
second time to the values >= 1e-280 alone -- in both layouts, for --NumPC 2, 4 and 10, known allele frequencies, markers
100, 400 and 950 reads deep, missing and depth-filtered markers; vb2_ctx_marginals returns in the same session the bits it
returns before and after the new entry was called, and q = GF2 h ties the two entries together.

Relations (vb2_source_set_relations): against the float64 restatement, per ordered pair and relation

    |K_gpu - K_64|  <=  8 x 2^-24 x sum_m (1 + |log v_m|)        v_m: the floored mixture of marker m

The 8, with u = 2^-24: two roundings from the stored float32 inputs (2u), the product and the two additions of a dot
(3u), the multiplication by k exact, two additions of the mixture (2u) -- 7u relative on v, so 7u on log v -- and the
logarithm's result 2u relative, 2u |log v|: together within 8u (1 + |log v|); FMAs only lower it.
`shared` must be exact; a pair's four values the same bits in a set of 4 and of 17, and from call to call.

End to end: eight samples of one family and three outsiders through --PileupList --FindRelated, in both cohort modes.

Measured on an MI355X (the tests print these, pytest -s): see the figures DESIGN.md section 15 records.
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402
import related_ref as rr  # noqa: E402
import source_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
TOL_FACTOR, TOL_FLOOR = deriv_ref.TOL_FACTOR, deriv_ref.TOL_FLOOR      # 32, 1e-13
K_FACTOR = 8
RELATED, BOTH = vb.SourceSet.RELATED, vb.SourceSet.SOURCE | vb.SourceSet.RELATED
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    print("\nworst figures of this module:")
    for key in sorted(_WORST):
        print("  %-44s %.4g  (%s)" % ((key,) + _WORST[key]))


def _note(key, value, where):
    if value > _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (float(value), where)


def _rel_dev(x, ref):
    """worst |x - ref| / |ref| over the values (where the 80-bit reference is 0 the value must be 0)."""
    x, ref = np.asarray(x), np.asarray(ref)
    zero = ref == 0
    assert np.all(np.asarray(x)[zero] == 0)
    if np.all(zero):
        return 0.0
    return float(np.max(np.abs(x[~zero].astype(ref.dtype) - ref[~zero]) / np.abs(ref[~zero])))


def _check_marginals(d, ctx, pc1, pc2, alpha, label):
    M = d.num_marker
    layout = ctx.info()["layout"]
    before = ctx.marginals(pc1, pc2, alpha)
    c, q, ll, h, t = ctx.marginals(pc1, pc2, alpha, related=True)
    after = ctx.marginals(pc1, pc2, alpha)
    for a, b, e in zip(before, (c, q, ll), after):                      # vb2_ctx_marginals: the same bits throughout
        assert np.array_equal(a, b) and np.array_equal(a, e), label
    assert h.shape == (M, 3) and t.shape == (M, 3)
    c64, c80 = deriv_ref.Counts(d), deriv_ref.Counts(d, np.longdouble)
    m64, m80 = rr.marginals(c64, pc1, pc2, alpha), rr.marginals(c80, pc1, pc2, alpha)
    r64, r80 = rr.panel_order(c64, M, m64), rr.panel_order(c80, M, m80)
    counted = np.zeros(M, dtype=bool)
    counted[c80.idx[m80["live"]]] = True
    assert np.array_equal(h.sum(axis=1) > 0, counted), label
    assert np.array_equal(t.sum(axis=1) > 0, counted), label
    assert np.array_equal(q.sum(axis=1) > 0, counted), label
    assert np.all(h[~counted] == 0) and np.all(t[~counted] == 0)
    # the two entries agree: q = GF2 h, sum t = 1.  GF2 is the float64 restatement's: its allele frequency is a sum of k + 2
    # terms in another order than the kernel's, and 1 - af of an af within MIN_AF of 1 magnifies that by 1 / MIN_AF, twice
    # in the square
    gf2 = np.zeros((M, 3))
    gf2[c64.idx] = m64["gf2"]
    tol = 4 * (d.num_pc + 2) * np.finfo(np.float64).eps / deriv_ref.MIN_AF
    normal = counted[:, None] & (q >= 1e-280)                           # (below, a double has not all its bits: the rule's second pass)
    assert np.all(np.abs(q - gf2 * h)[normal] <= tol * q[normal]), label
    assert np.max(np.abs(t.sum(axis=1)[counted] - 1)) <= 1e-14, label
    failures = []
    for name, got, a, b in (("h", h, r64[1], r80[1]), ("t", t, r64[2], r80[2])):
        dev, dev64 = _rel_dev(got, b), _rel_dev(a, b)
        tol = max(TOL_FACTOR * dev64, TOL_FLOOR)
        ratio = dev / max(dev64, TOL_FLOOR / TOL_FACTOR)
        print("related marginals %-22s layout %d %-2s dev %.3g dev64 %.3g tol %.3g ratio %.3g" % (label, layout, name, dev, dev64, tol, ratio))
        _note("marginals %s layout %d: dev / floor" % (name, layout), ratio, "%s alpha=%g" % (label, alpha))
        if not dev <= tol:
            failures.append((name, label, dev, dev64, tol))
        big = np.abs(b) >= 1e-280
        if not np.all(big | (b == 0)):
            dev, dev64 = _rel_dev(np.where(big, got, 0), np.where(big, b, 0)), _rel_dev(np.where(big, a, 0), np.where(big, b, 0))
            tol = max(TOL_FACTOR * dev64, TOL_FLOOR)
            print("related marginals %-22s layout %d %-2s normal values only: dev %.3g dev64 %.3g tol %.3g" % (label, layout, name, dev, dev64, tol))
            _note("marginals %s layout %d: dev / floor" % (name, layout), dev / max(dev64, TOL_FLOOR / TOL_FACTOR), "%s alpha=%g, normal values" % (label, alpha))
            if not dev <= tol:
                failures.append((name + " (normal values)", label, dev, dev64, tol))
    assert not failures, failures
    return h, t


def _point(k, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, k), rng.normal(0, scale, k)


@pytest.mark.parametrize("pd", [0, 1])
@pytest.mark.parametrize("k", [2, 4, 10])
def test_marginals_match_the_restatement(k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(1500, mean_depth=30, num_pc=k, alpha_true=0.05, seed=60 + k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        for alpha in (1e-6, 0.03, 0.3):
            _check_marginals(d, ctx, *_point(k, k), alpha, "1500x30 k=%d" % k)


@pytest.mark.parametrize("pd", [0, 1])
def test_marginals_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    k = 2
    d = vb.synth.make_pileup(1500, mean_depth=30, num_pc=k, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0, 0.0, 1.0)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        a = _check_marginals(d, ctx, *_point(k, 1), 0.04, "known AF")
        b = ctx.marginals(*_point(k, 2), 0.04, related=True)[3:]         # the PCs do not enter
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("pd", [0, 1])
@pytest.mark.parametrize("depth", [100, 400, 950])
def test_marginals_deep_markers(depth, pd, tunable):
    tunable("pd", pd)
    k = 2
    d = vb.synth.make_pileup(400, mean_depth=depth, num_pc=k, alpha_true=0.1, seed=depth)
    with vb.LikelihoodContext(d) as ctx:
        print("400 x %d asked for layout %d, got %d" % (depth, pd, ctx.info()["layout"]))
        if depth == 950:
            assert ctx.info()["layout"] == 0                             # the run-word fallback
        for alpha in (0.01, 0.2):
            _check_marginals(d, ctx, *_point(k, 3), alpha, "400x%d" % depth)


@pytest.mark.parametrize("pd", [0, 1])
def test_marginals_missing_and_depth_filtered_markers(pd, tunable):
    tunable("pd", pd)
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=20, num_pc=k, alpha_true=0.05, seed=21, missing_frac=0.15)
    depth = np.diff(d.read_off)
    d = vb.synth.with_sanity_stats(d)
    lo, hi = d.avg_depth - 3 * d.sd_depth, d.avg_depth + 3 * d.sd_depth
    filtered = (depth > 0) & ((depth < lo) | (depth > hi))
    assert (depth == 0).sum() > 200 and filtered.sum() > 0 and not d.sanity_disabled
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        h, t = _check_marginals(d, ctx, *_point(k, 4), 0.05, "missing + filtered")
    gone = (depth == 0) | filtered
    assert np.all(h[gone] == 0) and np.all(t[gone] == 0)
    assert np.all(t[~gone].sum(axis=1) > 0.999)


def test_marginals_outputs_are_optional_and_nan_counts_nothing():
    import ctypes as C
    k = 2
    d = vb.synth.make_pileup(1000, mean_depth=20, num_pc=k, alpha_true=0.05, seed=2)
    p1, p2 = _point(k, 1)
    with vb.LikelihoodContext(d) as ctx:
        h, t = ctx.marginals(p1, p2, 0.05, related=True)[3:]
        only_h, only_t = np.zeros((1000, 3)), np.zeros((1000, 3))
        args = (ctx._h, p1.ctypes.data_as(C.c_void_p), p2.ctypes.data_as(C.c_void_p), 0.05)
        _abi.check(ctx._lib.vb2_ctx_marginals_related(*args, only_h.ctypes.data_as(C.c_void_p), None), "vb2_ctx_marginals_related")
        _abi.check(ctx._lib.vb2_ctx_marginals_related(*args, None, only_t.ctypes.data_as(C.c_void_p)), "vb2_ctx_marginals_related")
        _abi.check(ctx._lib.vb2_ctx_marginals_related(*args, None, None), "vb2_ctx_marginals_related")
        assert np.array_equal(only_h, h) and np.array_equal(only_t, t) and h.any() and t.any()
        hn, tn = ctx.marginals(p1, p2, float("nan"), related=True)[3:]
        assert not hn.any() and not tn.any()


# ---- relations ----

def _head(d, M):
    """The first M markers of a PileupData."""
    return dataclasses.replace(d, ud=d.ud[:M], means=d.means[:M], read_off=d.read_off[:M + 1], alt_base=d.alt_base[:M],
                               known_af=None if d.known_af is None else d.known_af[:M],
                               meta=dict(ref_base=d.meta["ref_base"][:M]))


def _estimates(n, k, seed, alphas=None):
    """Made-up estimates (the statistic is a function of the point, whatever search found it)."""
    rng = np.random.default_rng(seed)
    return [dict(alpha=float(alphas[i]) if alphas is not None and alphas[i] > 0 else 0.001 + 0.0005 * (i % 7), llk1=0.0, llk0=0.0,
                 pc=rng.normal(0, 0.01, k), pc2=rng.normal(0, 0.01, k)) for i in range(n)]


@pytest.fixture(scope="module")
def family():
    """The eight samples of related_ref.FAMILY on a panel of 8 193 markers, about 8 reads deep; shared, never changed."""
    panel = sr.make_panel(8193, 2, seed=11)
    data, alphas = rr.make_family(panel, 8, 111)
    return data, alphas


def _check_relations(K, shared, rows, label):
    K64, sh64, bound = rr.relations(rows)
    n = len(rows)
    assert K.shape == (n, n, 4) and shared.shape == (n, n)
    assert np.all(np.isnan(K[np.eye(n, dtype=bool)]))
    assert np.array_equal(np.isnan(K), np.isnan(K64)), label
    assert np.array_equal(shared, sh64.astype(shared.dtype)), label
    off = ~np.isnan(K64)
    if not off.any():
        return
    unit = 2.0 ** -24 * bound[off]
    err = np.abs(K[off] - K64[off])
    assert np.all(err[unit == 0] == 0), label                          # (a pair that shares no marker: no evidence, exactly)
    ratio = np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), 0.0)
    print("relations %-28s n=%d: worst |K_gpu - K_64| / (2^-24 sum (1 + |log v|)) = %.3g (allowed %d), largest |K| %.4g" %
          (label, n, ratio.max(), K_FACTOR, np.nanmax(np.abs(K64))))
    _note("K error / (2^-24 sum(1+|log v|))", ratio.max(), label)
    assert np.all(ratio <= K_FACTOR), (label, ratio.max())


def _fill(s, data, est, tunable=None):
    for i, (d, e) in enumerate(zip(data, est)):
        if tunable is not None:
            tunable("pd", i % 2)                                         # both layouts feed one set
        with vb.LikelihoodContext(d) as ctx:
            assert s.add(ctx, e) == i


@pytest.mark.parametrize("M", [1, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_relations_over_chunk_and_stripe_boundaries(M, family, tunable):
    data = [_head(family[0][i], M) for i in (0, 1, 2, 5)]                # A, its second library, the child, an outsider
    est = _estimates(4, 2, seed=M, alphas=[0, 0.03, 0, 0])
    rows = [rr.rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    with vb.SourceSet(M, 4, planes=RELATED) as s:
        _fill(s, data, est, tunable)
        K, shared = s.relations()
        K2, shared2 = s.relations()
    _check_relations(K, shared, rows, "%d markers" % M)
    assert np.array_equal(K, K2, equal_nan=True) and np.array_equal(shared, shared2)          # call to call
    if M >= 4095:       # the statistic does its job on these made-up points too
        assert np.argmax(K[0, 1]) == 0 and np.argmax(K[0, 2]) == 1 and np.all(K[0, 3] < 0)


@pytest.mark.parametrize("n", [1, 2, 16, 17, 33])
def test_relations_over_tile_boundaries(n, family):
    M = 130
    data = [_head(family[0][i % 8], M) for i in range(n)]
    est = _estimates(n, 2, seed=n)
    rows = [rr.rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    with vb.SourceSet(M, n, planes=RELATED) as s:
        _fill(s, data, est)
        K, shared = s.relations()
    _check_relations(K, shared, rows, "%d samples" % n)


def test_the_same_pair_in_a_set_of_4_and_of_17_and_both_planes_keep_the_source_scores(family, tunable):
    M, n = 4097, 17
    data = [_head(family[0][i % 8], M) for i in range(n)]
    est = _estimates(n, 2, seed=5, alphas=[0, 0.03] + [0] * 15)
    pick = [0, 1, 9, 16]
    with vb.SourceSet(M, n, planes=BOTH) as big, vb.SourceSet(M, 4, planes=RELATED) as small, vb.SourceSet(M, 4) as source:
        for i, (d, e) in enumerate(zip(data, est)):
            tunable("pd", i % 2)
            with vb.LikelihoodContext(d) as ctx:
                big.add(ctx, e)
                if i in pick:
                    small.add(ctx, e)
                    source.add(ctx, e)
        K, shared = big.relations()
        Ks, shs = small.relations()
        assert np.array_equal(Ks, K[np.ix_(pick, pick)], equal_nan=True)                          # whatever else the set holds
        assert np.array_equal(shs, shared[np.ix_(pick, pick)])
        # a set with both planes gives the source scores the bits of a source-only set
        S, sh = big.scores()
        Ss, shss = source.scores()
        assert np.array_equal(Ss, S[np.ix_(pick, pick)], equal_nan=True) and np.array_equal(shss, sh[np.ix_(pick, pick)])
        # the entries refuse a set without their planes
        for call in (small.scores, source.relations):
            with pytest.raises(_abi.Vb2Error) as e:
                call()
            assert e.value.code == _abi.VB2_ERR_INVALID
    rows = [rr.rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    _check_relations(K, shared, rows, "17 samples, both planes")


def test_an_empty_slot_is_nan_and_disturbs_nobody(family):
    M = 1000
    data = [_head(family[0][i], M) for i in range(4)]
    est = _estimates(4, 2, seed=9)
    wrong = _head(family[0][4], M - 1)                                    # another panel size: the add fails, its slot stays
    with vb.SourceSet(M, 5, planes=RELATED) as s, vb.SourceSet(M, 4, planes=RELATED) as ref:
        for i in range(4):
            if i == 2:
                with vb.LikelihoodContext(wrong) as ctx, pytest.raises(_abi.Vb2Error):
                    s.add(ctx, est[0])
            with vb.LikelihoodContext(data[i]) as ctx:
                s.add(ctx, est[i])
                ref.add(ctx, est[i])
        assert s.count == 5
        K, shared = s.relations()
        Kr, shr = ref.relations()
    assert np.all(np.isnan(K[2])) and np.all(np.isnan(K[:, 2])) and not shared[2].any() and not shared[:, 2].any()
    keep = [0, 1, 3, 4]
    assert np.array_equal(K[np.ix_(keep, keep)], Kr, equal_nan=True) and np.array_equal(shared[np.ix_(keep, keep)], shr)


def test_samples_that_miss_each_others_markers(family):
    M = 600
    a, b, c = (_head(family[0][i], M) for i in (0, 2, 5))

    def without(d, lo, hi):                                               # no reads on markers [lo, hi)
        off = d.read_off.copy()
        keep = np.ones(int(off[-1] - off[0]), dtype=bool)
        keep[off[lo] - off[0]:off[hi] - off[0]] = False
        depth = np.diff(off)
        depth[lo:hi] = 0
        new = np.concatenate([[0], np.cumsum(depth)])
        return dataclasses.replace(d, read_off=new, bases=d.bases[off[0]:off[-1]][keep], quals=d.quals[off[0]:off[-1]][keep])

    data = [without(a, 0, 300), without(b, 250, 600), without(c, 100, 170)]
    est = _estimates(3, 2, seed=4)
    rows = [rr.rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    with vb.SourceSet(M, 3, planes=RELATED) as s:
        _fill(s, data, est)
        K, shared = s.relations()
    _check_relations(K, shared, rows, "disjoint markers")
    assert shared[0, 1] == 0 and np.all(K[0, 1] == 0) and np.all(K[1, 0] == 0)      # nothing shared: no evidence
    assert 0 < shared[1, 2] < 250 and 0 < shared[0, 2] <= 300


def test_relations_with_mixtures_below_the_floor():
    """Deep samples of different individuals: where the target is surely one homozygote and the partner's reads allow only
    the other, d2 and d1 fall far below 1e-30 (and below the float32 range) and the floor takes over."""
    panel = sr.make_panel(600, 2, seed=41)
    G = sr.draw_individuals(panel, 3, seed=42)
    data = [sr.make_sample(panel, G[0], G[2], 300, 0.0, 43), sr.make_sample(panel, G[1], G[2], 300, 0.0, 44),
            sr.make_sample(panel, G[0], G[2], 300, 0.05, 45)]
    est = [dict(alpha=0.001, pc=np.zeros(2), pc2=np.zeros(2)), dict(alpha=0.001, pc=np.zeros(2), pc2=np.zeros(2)),
           dict(alpha=0.05, pc=np.zeros(2), pc2=np.zeros(2))]
    rows = [rr.rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    both = (rows[0][0].sum(axis=1) > 0) & (rows[1][1].sum(axis=1) > 0)
    d2 = (rows[0][0] * rows[1][1]).sum(axis=1)[both]
    d1 = (rows[0][2] * rows[1][1]).sum(axis=1)[both]
    print("pair (0, 1): %d markers with d2 below the floor, %d with d1, of %d" % ((d2 < rr.DOT_FLOOR).sum(), (d1 < rr.DOT_FLOOR).sum(), both.sum()))
    assert (d2 < rr.DOT_FLOOR).sum() >= 10 and (d1 < rr.DOT_FLOOR).sum() >= 10
    with vb.SourceSet(600, 3, planes=RELATED) as s:
        _fill(s, data, est)
        K, shared = s.relations()
    _check_relations(K, shared, rows, "floored mixtures")
    assert K[0, 1, 0] < 10 * np.log(rr.DOT_FLOOR) * 0.5 and np.argmax(K[0, 2]) == 0 and K[0, 2, 0] > 0


def test_a_target_fitted_above_one_half_relates_as_its_mirrored_twin(family):
    M, k = 3000, 2
    data = [_head(family[0][i], M) for i in (0, 2)]
    rng = np.random.default_rng(5)
    pc1, pc2 = rng.normal(0, 0.01, k), rng.normal(0, 0.01, k)
    rep1, rep2 = pc1.copy(), pc2.copy()
    rep1[:2], rep2[:2] = pc2[:2], pc1[:2]                       # as the estimator reports an alpha >= 0.5
    high = dict(alpha=0.96, pc=rep1, pc2=rep2)
    twin = dict(alpha=1.0 - 0.96, pc=pc2, pc2=pc1)
    other = dict(alpha=0.02, pc=np.zeros(k), pc2=np.zeros(k))
    with vb.SourceSet(M, 3, planes=RELATED) as s:
        with vb.LikelihoodContext(data[0]) as ctx:
            s.add(ctx, high)
            s.add(ctx, twin)
        with vb.LikelihoodContext(data[1]) as ctx:
            s.add(ctx, other)
        K, shared = s.relations()
    assert np.array_equal(K[0, 2], K[1, 2]) and np.array_equal(K[2, 0], K[2, 1]) and shared[0, 2] == shared[1, 2]
    rows = [rr.rows(data[0], rep1, rep2, 0.96), rr.rows(data[0], pc2, pc1, 1.0 - 0.96), rr.rows(data[1], other["pc"], other["pc2"], 0.02)]
    _check_relations(K, shared, rows, "alpha 0.96 and its twin")


@pytest.mark.parametrize("planes,per_marker", [(RELATED, 36), (BOTH, 48), (vb.SourceSet.SOURCE, 24)])
def test_a_set_that_cannot_fit_says_how_much_it_needs(planes, per_marker):
    with pytest.raises(_abi.Vb2Error) as e:
        vb.SourceSet(1 << 24, 1 << 20, planes=planes)
    assert e.value.code == _abi.VB2_ERR_NOMEM
    assert str((1 << 44) * per_marker) in str(e.value)
    with pytest.raises(_abi.Vb2Error) as e:
        vb.SourceSet(100, 2, planes=4)
    assert e.value.code == _abi.VB2_ERR_INVALID


# ---- end to end: --PileupList --FindRelated ----

def _write_cohort(tmp, M=3000, depth=30, seed=11, extra_failing=False):
    from verifybamid_amd import synth
    panel = sr.make_panel(M, 2, seed=seed)
    data, _ = rr.make_family(panel, depth, seed + 100)
    prefix = str(tmp / "panel")
    synth.write_files(data[0], prefix)                           # .UD / .mu / .bed (and sample 0's pileup)
    chrs, poss = ["1"] * M, 1000 + 10 * np.arange(M)
    piles, outs = [], []
    for i, d in enumerate(data):
        p = str(tmp / ("%s.pileup" % rr.FAMILY[i]))
        synth.write_pileup_text(p, chrs, poss, panel["ref"], d.read_off, d.bases, d.quals)
        piles.append(p)
        outs.append(str(tmp / rr.FAMILY[i]))
    if extra_failing:                                            # 300 covered markers: fails the sanity check
        d = data[5]
        off = d.read_off.copy()
        off[301:] = off[300]
        p = str(tmp / "bad.pileup")
        synth.write_pileup_text(p, chrs, poss, panel["ref"], off, d.bases, d.quals)
        piles.insert(3, p)
        outs.insert(3, str(tmp / "bad"))
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        for p, o in zip(piles, outs):
            f.write("%s\t%s\n" % (p, o))
    return prefix, piles, outs, lst, data


def _run_cli(prefix, lst, out, related=False, source=False, stream=True, top=None):
    env = dict(os.environ)
    if not stream:
        env["VB2_COHORT_STREAM"] = "0"
    args = [CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupList", lst, "--Output", out]
    if related:
        args.append("--FindRelated")
    if source:
        args.append("--FindSource")
    if top is not None:
        args += ["--RelatedTop", str(top)]
    return subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


HEADER = ["#SAMPLE", "PARTNER", "RANK", "RELATION", "LLR", "LLR_DUP", "LLR_PO", "LLR_FS", "LLR_D2", "MARKERS"]


def _read_related(path):
    rows = {}
    with open(path) as f:
        assert f.readline().rstrip("\n").split("\t") == HEADER
        for line in f:
            t = line.rstrip("\n").split("\t")
            assert len(t) == len(HEADER)
            rows.setdefault(t[0], []).append(dict(partner=t[1], rank=int(t[2]), relation=t[3], llr=t[4], k=t[5:9], markers=int(t[9])))
    return rows


def _outputs(outs):
    return [open(o + ext, "rb").read() for o in outs for ext in (".selfSM", ".Ancestry")]


def _last_digit(x):
    """One unit of the last of the six digits %g prints of x."""
    return 10.0 ** (np.floor(np.log10(max(abs(x), 1e-300))) - 5)


@pytest.mark.parametrize("stream", [True, False])
def test_end_to_end_find_related(tmp_path, stream, tunable):
    tunable("cohort_stream", 1 if stream else 0)               # (the in-process run below, like the command line's)
    prefix, piles, outs, lst, data = _write_cohort(tmp_path)
    n = len(piles)
    run = str(tmp_path / "run")
    plain = _run_cli(prefix, lst, run, stream=stream)
    assert plain.returncode == 0, plain.stderr[-2000:]
    files_plain = _outputs(outs)
    assert not os.path.exists(run + ".Related")
    src = _run_cli(prefix, lst, run, source=True, stream=stream)
    assert src.returncode == 0, src.stderr[-2000:]
    sources_alone = open(run + ".Sources", "rb").read()
    os.remove(run + ".Sources")
    found = _run_cli(prefix, lst, run, related=True, stream=stream)
    assert found.returncode == 0, found.stderr[-2000:]
    # stdout, .selfSM and .Ancestry: byte for byte what the run without the flag wrote; no .Sources unasked
    assert found.stdout == plain.stdout
    assert _outputs(outs) == files_plain
    assert not os.path.exists(run + ".Sources")
    table = _read_related(run + ".Related")
    # with --FindSource as well: .Sources is what --FindSource alone writes, .Related what --FindRelated alone writes
    related_alone = open(run + ".Related", "rb").read()
    both = _run_cli(prefix, lst, run, related=True, source=True, stream=stream)
    assert both.returncode == 0, both.stderr[-2000:]
    assert both.stdout == plain.stdout and _outputs(outs) == files_plain
    assert open(run + ".Sources", "rb").read() == sources_alone
    assert open(run + ".Related", "rb").read() == related_alone
    # the matrix of vb2_cohort_run_related on the same files
    res, rel = vb.run_cohort_files(prefix, piles, num_pc=2, find_related=True, group_size=0)
    K, shared = rel["llr"], rel["shared"]
    assert all(r["status"] == 0 for r in res)
    off = ~np.eye(n, dtype=bool)
    assert np.all(np.isnan(K[~off])) and not np.isnan(K[off]).any()
    # ... and vb2_source_set_relations on the same estimates, from the same reads in memory
    with vb.SourceSet(len(data[0].means), n, planes=RELATED) as s:
        for d, e in zip(data, res):
            with vb.LikelihoodContext(vb.synth.with_sanity_stats(d)) as ctx:       # (the files' run filters by depth)
                s.add(ctx, e)
        Kset, shset = s.relations()
    assert np.array_equal(shset, shared)
    assert sorted(table) == sorted(outs)
    for i, o in enumerate(outs):
        rows = table[o]
        assert [r["rank"] for r in rows] == [1, 2, 3]                                 # --RelatedTop defaults to 3
        order = sorted((j for j in range(n) if j != i), key=lambda j: -K[i, j].max())[:3]
        assert [r["partner"] for r in rows] == [outs[j] for j in order]
        for r, j in zip(rows, order):
            best = int(np.argmax(K[i, j]))
            assert r["llr"] == "%g" % K[i, j, best] and r["k"] == ["%g" % x for x in K[i, j]] and r["markers"] == shared[i, j]
            assert r["relation"] == (rr.RELATIONS[best] if K[i, j, best] > 0 else "UN")
            for got, want in zip([float(x) for x in r["k"]], Kset[i, j]):
                assert abs(got - want) <= _last_digit(want), (o, outs[j], got, want)
    # the conditions of the feature: every related pair named, in both directions; every unrelated pair UN
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            true = rr.TRUE.get((min(i, j), max(i, j)), "UN")
            best = int(np.argmax(K[i, j]))
            name = rr.RELATIONS[best] if K[i, j, best] > 0 else "UN"
            print("%-10s %-10s %-3s -> %-3s %s" % (rr.FAMILY[i], rr.FAMILY[j], true, name, " ".join("%+9.1f" % x for x in K[i, j])))
            assert name == true, (rr.FAMILY[i], rr.FAMILY[j], K[i, j])
            listed = [r for r in table[outs[i]] if r["partner"] == outs[j]]
            assert all(r["relation"] == true for r in listed)
    first = {rr.FAMILY[i]: (os.path.basename(table[o][0]["partner"]), table[o][0]["relation"]) for i, o in enumerate(outs)}
    assert first["A"] == ("A2", "DUP") and first["A2"] == ("A", "DUP") and first["child"][1] in ("PO", "FS")
    assert all(first[u][1] == "UN" for u in ("B", "U", "V"))


@pytest.mark.parametrize("top", [1, 2])
def test_related_top_sets_the_partners_listed(tmp_path, top):
    prefix, piles, outs, lst, data = _write_cohort(tmp_path, M=2000, depth=20)
    r = _run_cli(prefix, lst, str(tmp_path / "run"), related=True, top=top)
    assert r.returncode == 0, r.stderr[-2000:]
    table = _read_related(str(tmp_path / "run.Related"))
    assert sorted(table) == sorted(outs)
    for o in outs:
        assert [x["rank"] for x in table[o]] == list(range(1, top + 1))
        llr = [float(x["llr"]) for x in table[o]]
        assert llr == sorted(llr, reverse=True) and o not in [x["partner"] for x in table[o]]
    assert table[outs[0]][0]["partner"] == outs[1] and table[outs[0]][0]["relation"] == "DUP"


def test_a_sample_that_fails_its_sanity_check_is_absent_and_disturbs_nobody(tmp_path):
    prefix, piles, outs, lst, data = _write_cohort(tmp_path, M=2000, depth=20, extra_failing=True)
    n = len(piles)
    res, rel = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, find_related=True,
                                   sources_prefix=str(tmp_path / "run"))
    K, shared = rel["llr"], rel["shared"]
    assert res[3]["status"] == _abi.VB2_ERR_SANITY and all(r["status"] == 0 for i, r in enumerate(res) if i != 3)
    assert np.all(np.isnan(K[3])) and np.all(np.isnan(K[:, 3])) and not shared[3].any() and not shared[:, 3].any()
    keep = [i for i in range(n) if i != 3]
    good = [p for i, p in enumerate(piles) if i != 3]
    res8, rel8 = vb.run_cohort_files(prefix, good, num_pc=2, find_related=True)
    assert np.array_equal(K[np.ix_(keep, keep)], rel8["llr"], equal_nan=True)
    assert np.array_equal(shared[np.ix_(keep, keep)], rel8["shared"])
    table = _read_related(str(tmp_path / "run.Related"))
    assert outs[3] not in table and sorted(table) == sorted(outs[i] for i in keep)
    assert all(outs[3] not in [x["partner"] for x in table[o]] for o in table)
