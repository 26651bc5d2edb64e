"""vb2_llk_derivs_batch on the MI355X (deriv_kernels.hip) against the numpy restatement (tests/deriv_ref.py) and against
vb2_llk_eval_batch: both layouts, several --NumPC, batch sizes, deep and quality-0 pileups, clamped and known allele
frequencies; determinism of the fixed-order reductions; and the shapes where the layouts differ -- a second stripe of
the marker kernel's loop, deep live markers in the probability domain, window rows of every kind, markers that do not
count, wide parameter rows, tiny samples, the error paths of the host entry, a seeded sweep.

Every comparison (_compare) makes two checks per point.  The first is the original one: 1e-10 of the largest entry of
the whole gradient / Hessian against the float64 restatement.  It cannot see the small blocks (at alpha = 1e-6 the
contaminant's whole block is about the accepted error).  The second is per block -- 3 of the gradient, 6 of the Hessian
-- against the restatement in 80-bit floats, in units of each entry's condition sum S_e (deriv_ref.derivs_cond):

    max_e |kernel_e - ref80_e| / S_e  <=  tol(block) = max(32 x dev64(block), 1e-13)

where dev64 is the float64 restatement's own deviation from the 80-bit one in the same units, computed per case, point
and block inside the test.  The 32 is a guess at what another order of the same double arithmetic may cost (products
of up to ~800 table rows against one sum of logarithms; a strided sum and a tree against numpy's pairwise sums).

Measured on an MI355X, worst kernel deviation over the floor max(dev64, 1e-13 / 32) per block and layout (the check
fails above 32); the module prints this table at its end (pytest -s):

    block         layout 0 (run words)              layout 1 (probability domain)
    g:pc1          6.6  (sweep, 150 deep, a=1e-6)    2.9  (sweep, a=1e-6)
    g:pc2          4.2  (sweep, a=0.97)              1.9  (1 marker, a=0.97)
    g:alpha        4.4  (400 x 950, a=1e-6)          7.6  (sweep, 400 deep, a=0.5)
    h:pc1.pc1     12.1  (sweep, 400 deep, a=0.5)     6.8  (100 000 x 30, a=0.3)
    h:pc2.pc2      3.5  (sweep, a=0.97)              2.5  (sweep, a=1e-6)
    h:pc1.pc2     10.3  (binned q, a=1e-6)          16.9  (binned q, window rows, a=1e-6)
    h:pc1.alpha    5.8  (sweep, a=0.5)               4.5  (sweep, a=0.18)
    h:pc2.alpha    5.0  (sweep, a=0.74)              3.7  (sweep, a=0.5)
    h:alpha.alpha  3.8  (sweep, a=0.3)               3.9  (sweep, a=0.03)

No block needed more than 32 x dev64.  Before the log-domain kernel summed the diagonal pairs itself (it took the
logarithm of the context's diagonal constants, which are subnormal doubles past ~1 000 reads) the 400 x 950 sample
stood at 250 - 980 x the floor in six blocks.
"""
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHAS = [1e-6, 0.03, 0.3, 0.5, 0.97]
_WORST = {}                      # (layout, block) -> (kernel deviation / floor, label): the docstring's table


@pytest.fixture(scope="module", autouse=True)
def _print_kernel_to_floor_table():
    yield
    names = sorted({b for _, b in _WORST})
    print("\nkernel deviation / max(dev64, 1e-13 / 32), worst per block and layout (the check fails above 32)")
    for b in names:
        print("  %-14s" % b + "".join("  layout %d: %8.3g (%s)" % ((lay,) + _WORST[(lay, b)])
                                      for lay in (0, 1) if (lay, b) in _WORST))


def _points(k, alphas, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    B = len(alphas)
    return rng.normal(0, scale, (B, k)), rng.normal(0, scale, (B, k)), np.asarray(alphas, dtype=np.float64)


def _mixed_points(k, alphas, seed):
    """Random PCs of scale 0.01 and 0.05 in turn."""
    p1, p2, a = _points(k, alphas, seed)
    p1[1::2] *= 5
    p2[1::2] *= 5
    return p1, p2, a


class Refs:
    """The CPU side of a sample: its counts in both precisions and the references of the points asked for, computed
    once and shared by the contexts (layouts, tunables) the sample is run in."""

    def __init__(self, d):
        self.d = d
        self.c64 = deriv_ref.Counts(d)
        self.c80 = deriv_ref.Counts(d, np.longdouble)
        self.memo = {}

    def at(self, pc1, pc2, alpha):
        key = (np.asarray(pc1).tobytes(), np.asarray(pc2).tobytes(), float(alpha))
        if key not in self.memo:
            self.memo[key] = deriv_ref.reference(self.c64, self.c80, pc1, pc2, alpha)
        return self.memo[key]


def _compare(d, ctx, pc1, pc2, alpha, alpha_entries=True, refs=None, label="", got=None):
    k = d.num_pc
    n = 2 * k + 1
    layout = ctx.info()["layout"]
    llk, grad, hess = ctx.derivatives(pc1, pc2, alpha) if got is None else got
    assert llk.shape == (len(alpha),) and grad.shape == (len(alpha), n) and hess.shape == (len(alpha), n, n)
    want_llk = ctx.llk(pc1, pc2, alpha)
    refs = refs or Refs(d)
    sel = slice(0, n) if alpha_entries else slice(0, 2 * k)
    failures = []
    for b in range(len(alpha)):
        assert abs(llk[b] - want_llk[b]) <= 1e-13 * abs(want_llk[b]), (b, llk[b], want_llk[b])
        ref = refs.at(pc1[b], pc2[b], alpha[b])
        rg, rh = ref["g64"], ref["h64"]
        assert np.array_equal(hess[b], hess[b].T)
        g_scale = max(np.max(np.abs(rg[sel])), 1e-300)
        h_scale = max(np.max(np.abs(rh[sel, sel])), 1e-300)
        assert np.max(np.abs(grad[b, sel] - rg[sel])) <= 1e-10 * g_scale, (b, grad[b], rg)
        assert np.max(np.abs(hess[b][sel, sel] - rh[sel, sel])) <= 1e-10 * h_scale, (b, hess[b], rh)
        # per block, in units of the condition sums, against the 80-bit restatement
        for name, (dev, dev64, tol) in deriv_ref.block_devs(ref, grad[b], hess[b], alpha_entries).items():
            ratio = dev / max(dev64, deriv_ref.TOL_FLOOR / deriv_ref.TOL_FACTOR)
            where = "%s alpha=%g" % (label, alpha[b])
            if ratio > _WORST.get((layout, name), (-1.0, ""))[0]:
                _WORST[(layout, name)] = (ratio, where)
            if not dev <= tol:
                failures.append((ratio, name, where, "layout %d" % layout, "dev %.3g dev64 %.3g tol %.3g" % (dev, dev64, tol)))
    assert not failures, sorted(failures, reverse=True)[:6]
    return llk, grad, hess


def _agree(refs, pc1, pc2, alpha, a, b, alpha_entries=True):
    """Two variants of one sample (layouts, window rows on and off) agree within the sum of their tolerances."""
    for i in range(len(alpha)):
        ref = refs.at(pc1[i], pc2[i], alpha[i])
        fake = dict(ref, g80=np.asarray(b[1][i], dtype=np.longdouble), h80=np.asarray(b[2][i], dtype=np.longdouble))
        for name, (dev, _, _) in deriv_ref.block_devs(fake, a[1][i], a[2][i], alpha_entries).items():
            tol = deriv_ref.block_devs(ref, a[1][i], a[2][i], alpha_entries)[name][2]
            assert dev <= 2 * tol, (name, alpha[i], dev, tol)


@pytest.mark.parametrize("pd", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 4, 6])
def test_kernel_matches_the_restatement(k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=40 + k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        _compare(d, ctx, *_points(k, ALPHAS, seed=k), label="3000x30 k=%d" % k)


@pytest.mark.parametrize("B", [1, 2, 7, 16, 49])
def test_any_batch_size(B, tunable):
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=25, num_pc=k, alpha_true=0.05, seed=3)
    rng = np.random.default_rng(B)
    with vb.LikelihoodContext(d) as ctx:
        _compare(d, ctx, *_points(k, rng.uniform(0.001, 0.99, B), seed=B), label="batch %d" % B)


@pytest.mark.parametrize("pd", [0, 1])
def test_deep_markers_and_quality_zero_reads(pd, tunable):
    tunable("pd", pd)
    k = 2
    deep = vb.synth.make_pileup(200, mean_depth=1500, num_pc=k, alpha_true=0.1, seed=5)       # L underflows: dropped
    q0 = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.1, seed=6, q_lo=0, q_hi=93)
    for d, layout, label in ((deep, 0, "200x1500"), (q0, pd, "q 0..93")):   # (the deep sample takes the run words whatever the switch)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == layout
            _compare(d, ctx, *_points(k, [0.01, 0.2, 0.6], seed=7), label=label)


@pytest.mark.parametrize("pd", [0, 1])
def test_clamped_and_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=8)
    # AF below 0 / above 1 with panel rows that are not 0: a kernel that differentiated the clamped branch would show
    rng = np.random.default_rng(4)
    d.means[:150] = -0.05
    d.means[150:300] = 2.05
    d.ud[:300] = rng.normal(0, 1e-2, (300, k))
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        _compare(d, ctx, *_points(k, [0.02, 0.4], seed=9, scale=0.05), label="clamped AF")
    d.known_af = np.clip(d.means / 2.0, 0.0, 1.0)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        llk, grad, hess = _compare(d, ctx, *_points(k, [0.02, 0.4], seed=9), label="known AF")
    assert np.all(grad[:, :2 * k] == 0) and np.all(hess[:, :2 * k, :] == 0)


def test_alpha_outside_its_range_drops_the_markers_as_the_evaluation_does(tunable):
    """alpha outside [0, 1]: the evaluation takes the table entries as NaN and leaves every marker out; so do the
    derivatives (an even power of a negative entry must not count a marker)."""
    k = 2
    for pd in (0, 1):
        tunable("pd", pd)
        d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=14)
        pc1, pc2, a = _points(k, [-0.2, 1.3], seed=15)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == pd
            llk, grad, hess = ctx.derivatives(pc1, pc2, a)
            np.testing.assert_array_equal(llk, ctx.llk(pc1, pc2, a))
            assert np.all(grad == 0) and np.all(hess == 0)


@pytest.mark.parametrize("pd", [0, 1])
def test_alpha_at_its_bounds_llk_and_pc_entries(pd, tunable):
    tunable("pd", pd)
    k = 4
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=10)
    with vb.LikelihoodContext(d) as ctx:
        _compare(d, ctx, *_points(k, [0.0, 1.0], seed=11), alpha_entries=False, label="alpha 0 / 1")


def test_deterministic_and_independent_of_the_batch():
    k = 4
    d = vb.synth.make_pileup(5000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=12)
    pc1, pc2, a = _points(k, [0.01, 0.05, 0.2, 0.45, 0.03, 0.7, 0.1], seed=13)
    with vb.LikelihoodContext(d) as ctx:
        first = ctx.derivatives(pc1, pc2, a)
        again = ctx.derivatives(pc1, pc2, a)
        for x, y in zip(first, again):
            assert np.array_equal(x, y)
        for b in range(len(a)):
            alone = ctx.derivatives(pc1[b:b + 1], pc2[b:b + 1], a[b:b + 1])
            for x, y in zip(first, alone):
                assert np.array_equal(x[b], y[0]), b


# ---- the shapes where the layouts differ ----

def _num_cu(ctx):
    import torch
    return torch.cuda.get_device_properties(ctx.info()["device"]).multi_processor_count


def _stripes(ctx, chunk_points):
    """The marker kernel's launch geometry (launch_llk_derivs): groups of 16 micro-tiles, and the grid's width for a
    chunk of that many points.  More groups than workgroups: some workgroup walks a second stripe."""
    ntile_grp = (ctx.info()["num_tile"] + 15) // 16
    gx = max(1, min((4 * _num_cu(ctx) + chunk_points - 1) // chunk_points, ntile_grp))
    return ntile_grp, gx


def _same_bits(x, y, what):
    for u, v in zip(x, y):
        assert np.array_equal(u, v), what


def test_second_stripe_of_the_marker_loop_at_100000_markers(tunable):
    """100 000 markers: 391 groups of 16 micro-tiles against a grid 256 wide for a chunk of 4 points and 342 wide for a
    chunk of 3 -- workgroups walk a second stripe.  Batches of 3, 4 and 7 (chunks 3; 4; 4 + 3) give the bits of the
    points evaluated one at a time (a grid 391 wide: one stripe each)."""
    k = 4
    d = vb.synth.make_pileup(100000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=51)
    refs = Refs(d)
    pc1, pc2, a = _mixed_points(k, ALPHAS + [0.1, 0.01], seed=52)
    for pd in (1, 0):
        tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == pd
            for chunk in (3, 4):
                ntile_grp, gx = _stripes(ctx, chunk)
                assert ntile_grp > gx, (ntile_grp, gx)           # a second stripe exists
            assert _stripes(ctx, 1)[0] == _stripes(ctx, 1)[1]    # one at a time: another grid width, no second stripe
            all7 = ctx.derivatives(pc1, pc2, a)
            _same_bits(ctx.derivatives(pc1[:3], pc2[:3], a[:3]), [x[:3] for x in all7], "batch of 3")
            _same_bits(ctx.derivatives(pc1[3:], pc2[3:], a[3:]), [x[3:] for x in all7], "batch of 4")
            for b in range(7):
                _same_bits(ctx.derivatives(pc1[b:b + 1], pc2[b:b + 1], a[b:b + 1]), [x[b:b + 1] for x in all7], b)
            # the restatement in 80 bits costs a second per point here: the five alphas of the set
            _compare(d, ctx, pc1[:5], pc2[:5], a[:5], refs=refs, label="100000x30", got=[x[:5] for x in all7])


def test_second_stripe_of_a_single_point_above_262144_markers():
    """One point's grid is 4 x CUs = 1 024 wide: a second stripe needs more than 1 024 x 256 = 262 144 counted markers.
    (Float64 restatement and the whole-matrix tolerance only: the count matrix of this sample is large.)"""
    k = 2
    d = vb.synth.make_pileup(285000, mean_depth=4, num_pc=k, alpha_true=0.05, seed=53)
    c = deriv_ref.Counts(d)
    pc1, pc2, a = _points(k, [0.03], seed=54)
    with vb.LikelihoodContext(d) as ctx:
        ntile_grp, gx = _stripes(ctx, 1)
        assert ntile_grp > gx, (ntile_grp, gx)
        assert ctx.info()["num_active_marker"] == len(c.idx)
        llk, grad, hess = ctx.derivatives(pc1, pc2, a)
        want = ctx.llk(pc1, pc2, a)
    assert abs(llk[0] - want[0]) <= 1e-13 * abs(want[0])
    _, rg, rh = deriv_ref.derivs(c, pc1[0], pc2[0], a[0])
    assert np.max(np.abs(grad[0] - rg)) <= 1e-10 * np.max(np.abs(rg))
    assert np.max(np.abs(hess[0] - rh)) <= 1e-10 * np.max(np.abs(rh))


@pytest.mark.parametrize("depth,layout", [(100, 1), (400, 1), (650, 1), (950, 0)])
def test_deep_live_markers(depth, layout):
    """Many reads of one quality per marker: power rows P^n with n d and n d^2, runs split into several steps, products
    of unlikely pairs that go subnormal -- on markers that still count (L > 0), unlike the 1 500-deep sample above."""
    k = 2
    d = vb.synth.make_pileup(400, mean_depth=depth, num_pc=k, alpha_true=0.1, seed=5)
    refs = Refs(d)
    pc1, pc2, a = _mixed_points(k, ALPHAS, seed=55)
    for b in range(len(a)):
        assert deriv_ref.live_share(refs.c64, pc1[b], pc2[b], a[b]) >= 0.95, (depth, a[b])
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == layout
        _compare(d, ctx, pc1, pc2, a, refs=refs, label="400x%d" % depth)
        e1, e2, ea = _mixed_points(k, [0.0, 1.0], seed=56)
        _compare(d, ctx, e1, e2, ea, alpha_entries=False, refs=refs, label="400x%d" % depth)


def _profile(name):
    rng = np.random.default_rng(77)
    if name == "q2-60":
        return vb.synth.make_pileup(5000, 60, 2, seed=72, q_lo=2, q_hi=60)
    if name == "q10-45":
        return vb.synth.make_pileup(5000, 30, 2, seed=75, q_lo=10, q_hi=45)
    if name == "binned":
        d = vb.synth.make_pileup(5000, 40, 2, seed=73)
        d.quals[:] = np.array([2, 12, 23, 37], dtype=np.uint8)[(d.quals - 33) % 4] + 33
        return d
    d = vb.synth.make_pileup(5000, 30, 3, seed=74, q_lo=10, q_hi=40)
    d.quals[rng.random(d.quals.size) < 0.85] = 37 + 33
    return d


@pytest.mark.parametrize("name", ["q2-60", "q10-45", "binned", "dominant"])
def test_quality_profiles_with_and_without_window_rows(name, tunable):
    """The window rows of the probability domain (products of two power rows, and of those: d and d^2 add) on wide
    alphabets, binned qualities (several steps per window) and one dominant quality; without them (pd_pairs = 0) and in
    the run words.  The window rows are really there: fewer steps with them than without (but see below)."""
    d = _profile(name)
    k = d.num_pc
    refs = Refs(d)
    pc1, pc2, a = _mixed_points(k, ALPHAS, seed=57)
    got, steps, rows = {}, {}, {}
    for variant, pd, pairs in (("windows", 1, 1), ("powers", 1, 0), ("runs", 0, 1)):
        tunable("pd", pd)
        tunable("pd_pairs", pairs)
        with vb.LikelihoodContext(d) as ctx:
            info = ctx.info()
            assert info["layout"] == pd, variant
            steps[variant], rows[variant] = info["num_step"], info["num_table_row"]
            got[variant] = _compare(d, ctx, pc1, pc2, a, refs=refs, label="%s %s" % (name, variant))
    # (the dictionary gives the dominant-quality profile no window rows -- the same table either way, measured: its point
    # here is the long power rows of q 37, P^n with n d and n d^2, beside 30 rare qualities)
    assert steps["windows"] <= steps["powers"], steps
    assert (steps["windows"] < steps["powers"]) == (name != "dominant"), (steps, rows)
    assert (rows["windows"] != rows["powers"]) == (name != "dominant"), (steps, rows)
    _agree(refs, pc1, pc2, a, got["windows"], got["powers"])
    _agree(refs, pc1, pc2, a, got["windows"], got["runs"])
    _agree(refs, pc1, pc2, a, got["powers"], got["runs"])


@pytest.mark.parametrize("pd", [0, 1])
def test_markers_that_do_not_count(pd, tunable):
    """Markers without reads (30 %) and markers the +-3 sd depth filter drops: the kernel counts the restatement's."""
    tunable("pd", pd)
    k = 2
    plain = vb.synth.make_pileup(3000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=58, missing_frac=0.3)
    filtered = vb.synth.with_sanity_stats(vb.synth.make_pileup(3000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=59,
                                                               missing_frac=0.3))
    for d, label in ((plain, "missing"), (filtered, "missing + filter")):
        refs = Refs(d)
        present = int((np.diff(d.read_off) > 0).sum())
        assert present < 0.75 * d.num_marker
        assert (len(refs.c64.idx) < present) == (d is filtered)           # the filter drops markers
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == pd
            assert ctx.info()["num_active_marker"] == len(refs.c64.idx)
            _compare(d, ctx, *_mixed_points(k, ALPHAS, seed=60), refs=refs, label=label)
            _compare(d, ctx, *_mixed_points(k, [0.0, 1.0], seed=61), alpha_entries=False, refs=refs, label=label)


@pytest.mark.parametrize("k", [10, 24])
def test_wide_parameter_rows(k):
    """1 + n + n (n + 1) / 2 outputs per point (output_terms, the reduce kernel's grid): 253 at k = 10, 1 225 at k = 24."""
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=62)
    with vb.LikelihoodContext(d) as ctx:
        _compare(d, ctx, *_points(k, ALPHAS, seed=63, scale=0.003), label="k=%d" % k)


@pytest.mark.parametrize("pd", [0, 1])
def test_tiny_samples(pd, tunable):
    tunable("pd", pd)
    k = 2
    for M, depth in ((1, 30), (17, 5)):
        d = vb.synth.make_pileup(M, mean_depth=depth, num_pc=k, alpha_true=0.05, seed=64)
        assert int((np.diff(d.read_off) > 0).sum()) >= 1
        refs = Refs(d)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == pd
            _compare(d, ctx, *_mixed_points(k, ALPHAS, seed=65), refs=refs, label="%d markers" % M)
            _compare(d, ctx, *_mixed_points(k, [0.0, 1.0], seed=66), alpha_entries=False, refs=refs,
                     label="%d markers" % M)


def test_no_points_and_the_refusal_inside_a_search_bracket():
    """Context::derivs_host: num_point = 0 returns without touching the outputs; between vb2_ctx_search_begin and
    vb2_ctx_search_end (the resident kernel holds the stream) the call is refused with VB2_ERR_INVALID -- an argument
    check -- while evaluations inside the bracket and derivative calls after it give their usual values."""
    if os.environ.get("VB2_RESIDENT") == "0" or os.environ.get("VB2_SPIN_WAIT") == "0":
        pytest.skip("resident search mode switched off through the environment")
    import ctypes as C
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=67)
    pc1, pc2, a = _points(k, [0.04, 0.3], seed=68)
    n = 2 * k + 1
    lib = _abi.lib()

    def ptr(x):
        return x.ctypes.data_as(C.c_void_p)
    with vb.LikelihoodContext(d) as ctx:
        before = ctx.derivatives(pc1, pc2, a)
        plain = ctx.llk(pc1, pc2, a)
        llk, grad, hess = np.full(2, 7.0), np.full((2, n), 7.0), np.full((2, n, n), 7.0)
        assert lib.vb2_llk_derivs_batch(ctx._h, 0, ptr(pc1), ptr(pc2), ptr(a), ptr(llk), ptr(grad), ptr(hess)) == 0
        assert np.all(llk == 7.0) and np.all(grad == 7.0) and np.all(hess == 7.0)
        with ctx.search():
            with pytest.raises(_abi.Vb2Error) as err:
                ctx.derivatives(pc1, pc2, a)
            assert err.value.code == _abi.VB2_ERR_INVALID
            assert "vb2_ctx_search_begin" in str(err.value)
            inside = np.array([ctx.llk(pc1[b:b + 1], pc2[b:b + 1], a[b:b + 1])[0] for b in range(2)])
        assert np.array_equal(inside, plain)
        _same_bits(ctx.derivatives(pc1, pc2, a), before, "after the bracket")
        _compare(d, ctx, pc1, pc2, a, label="after a bracket")


SWEEP_SEED, SWEEP_CASES = 20261, 40


def test_seeded_sweep(tunable):
    """Random shapes in the spirit of tools/llk_fuzz.py: markers, depth, k, quality range and profile, missing
    markers, layout, window rows, batch size -- every case through the per-block check."""
    rng = np.random.default_rng(SWEEP_SEED)
    worst = (-1.0, None)
    for case in range(SWEEP_CASES):
        depth = int(rng.choice([2, 10, 30, 60, 150, 400, 700]))
        M = int(rng.integers(1, max(2, min(3000, 120000 // depth))))
        k = int(rng.integers(1, 11))
        q_lo = int(rng.integers(0, 40))
        q_hi = int(rng.integers(q_lo, min(93, q_lo + 60) + 1))
        profile = ("uniform", "binned", "dominant")[int(rng.integers(0, 3))]
        missing = float(rng.choice([0.0, 0.0, 0.1, 0.5]))
        B = int(rng.integers(1, 10))
        pd, pairs = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        seed = int(rng.integers(1, 1 << 30))
        d = vb.synth.make_pileup(M, mean_depth=depth, num_pc=k, alpha_true=float(rng.choice([0.0, 0.02, 0.2])),
                                 seed=seed, q_lo=q_lo, q_hi=q_hi, missing_frac=missing)
        if profile == "binned":
            d.quals[:] = np.array([2, 12, 23, 37], dtype=np.uint8)[(d.quals - 33) % 4] + 33
        elif profile == "dominant":
            d.quals[rng.random(d.quals.size) < 0.85] = 37 + 33
        if int((np.diff(d.read_off) > 0).sum()) == 0:
            d = vb.synth.make_pileup(M, mean_depth=depth + 3, num_pc=k, seed=seed, q_lo=q_lo, q_hi=q_hi)
        if rng.random() < 0.25:
            d = vb.synth.with_sanity_stats(d)
        alphas = np.where(rng.random(B) < 0.5, rng.choice(ALPHAS, B), rng.uniform(1e-4, 0.999, B))
        pc1, pc2, a = _mixed_points(k, alphas, seed=seed)
        what = dict(case=case, M=M, depth=depth, k=k, q=(q_lo, q_hi), profile=profile, missing=missing, B=B, pd=pd,
                    pairs=pairs, seed=seed, filter=not d.sanity_disabled)
        tunable("pd", pd)
        tunable("pd_pairs", pairs)
        refs = Refs(d)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["num_active_marker"] == len(refs.c64.idx), what
            before = dict(_WORST)
            try:
                _compare(d, ctx, pc1, pc2, a, refs=refs, label="sweep %d" % case)
            except AssertionError:
                print("seeded sweep: failing case", what)
                raise
            for key, (ratio, _) in _WORST.items():
                if before.get(key, (None,))[0] != ratio and ratio > worst[0]:
                    worst = (ratio, dict(what, block=key[1], layout=key[0]))
    print("seeded sweep: worst kernel deviation / floor %.3g at %s" % worst)
