"""vb2_llk_derivs_batch on the MI355X (deriv_kernels.hip) against the numpy restatement (tests/deriv_ref.py) and against
vb2_llk_eval_batch: both layouts, several --NumPC, batch sizes, deep and quality-0 pileups, clamped and known allele
frequencies; determinism of the fixed-order reductions."""
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _points(k, alphas, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    B = len(alphas)
    return rng.normal(0, scale, (B, k)), rng.normal(0, scale, (B, k)), np.asarray(alphas, dtype=np.float64)


def _compare(d, ctx, pc1, pc2, alpha, alpha_entries=True):
    k = d.num_pc
    n = 2 * k + 1
    llk, grad, hess = ctx.derivatives(pc1, pc2, alpha)
    assert llk.shape == (len(alpha),) and grad.shape == (len(alpha), n) and hess.shape == (len(alpha), n, n)
    want_llk = ctx.llk(pc1, pc2, alpha)
    c = deriv_ref.Counts(d)
    sel = slice(0, n) if alpha_entries else slice(0, 2 * k)
    for b in range(len(alpha)):
        assert abs(llk[b] - want_llk[b]) <= 1e-13 * abs(want_llk[b]), (b, llk[b], want_llk[b])
        _, rg, rh = deriv_ref.derivs(c, pc1[b], pc2[b], alpha[b])
        assert np.array_equal(hess[b], hess[b].T)
        g_scale = max(np.max(np.abs(rg[sel])), 1e-300)
        h_scale = max(np.max(np.abs(rh[sel, sel])), 1e-300)
        assert np.max(np.abs(grad[b, sel] - rg[sel])) <= 1e-10 * g_scale, (b, grad[b], rg)
        assert np.max(np.abs(hess[b][sel, sel] - rh[sel, sel])) <= 1e-10 * h_scale, (b, hess[b], rh)
    return llk, grad, hess


ALPHAS = [1e-6, 0.03, 0.3, 0.5, 0.97]


@pytest.mark.parametrize("pd", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 4, 6])
def test_kernel_matches_the_restatement(k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=40 + k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        _compare(d, ctx, *_points(k, ALPHAS, seed=k))


@pytest.mark.parametrize("B", [1, 2, 7, 16, 49])
def test_any_batch_size(B, tunable):
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=25, num_pc=k, alpha_true=0.05, seed=3)
    rng = np.random.default_rng(B)
    with vb.LikelihoodContext(d) as ctx:
        _compare(d, ctx, *_points(k, rng.uniform(0.001, 0.99, B), seed=B))


@pytest.mark.parametrize("pd", [0, 1])
def test_deep_markers_and_quality_zero_reads(pd, tunable):
    tunable("pd", pd)
    k = 2
    deep = vb.synth.make_pileup(200, mean_depth=1500, num_pc=k, alpha_true=0.1, seed=5)       # L underflows: dropped
    q0 = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.1, seed=6, q_lo=0, q_hi=93)
    for d, layout in ((deep, 0), (q0, pd)):          # (the deep sample takes the run words whatever the switch)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == layout
            _compare(d, ctx, *_points(k, [0.01, 0.2, 0.6], seed=7))


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
        _compare(d, ctx, *_points(k, [0.02, 0.4], seed=9, scale=0.05))
    d.known_af = np.clip(d.means / 2.0, 0.0, 1.0)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        llk, grad, hess = _compare(d, ctx, *_points(k, [0.02, 0.4], seed=9))
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
        _compare(d, ctx, *_points(k, [0.0, 1.0], seed=11), alpha_entries=False)


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
