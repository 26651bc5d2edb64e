"""vb2_paired_derivs on the MI355X (deriv_kernels.hip: PairPrior; paired.cpp) against the np.longdouble
restatement (tests/paired_deriv_ref.py) and against vb2_paired_eval and vb2_llk_derivs_batch: both layouts, several --NumPC, a
known-AF column, a sample that takes the run words whatever the switch, every kind of hypothesis row, 0 to 9 points per
hypothesis; the blocks that are exactly zero; the bits of a point whatever the launch pair holds.

The per-block rule is tests/test_derivs_gpu.py's, unchanged: max_e |kernel_e - ref80_e| / S_e <= max(32 x dev64, 1e-13),
dev64 the float64 restatement's own deviation in the same units, computed per case, point and block in the test.  The
module prints the worst kernel deviation over the floor max(dev64, 1e-13 / 32) per block and layout at its end (pytest -s);
the check fails above 32.
"""
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402
import paired_deriv_ref as pdr  # noqa: E402
import paired_ref as pr  # noqa: E402
from deriv_ref import Counts  # noqa: E402
from test_paired_gpu import ALL_OUT, ALPHAS, _hyp_rows, _other_q  # noqa: E402

pytestmark = pytest.mark.gpu

_WORST = {}                      # (layout, block) -> (kernel deviation / floor, label)
SLOTS = 8                        # points of a hypothesis per vb2_paired_eval step


@pytest.fixture(scope="module", autouse=True)
def _print_kernel_to_floor_table():
    yield
    print("\nkernel deviation / max(dev64, 1e-13 / 32), worst per block and layout (the check fails above 32)")
    for b in sorted({b for _, b in _WORST}):
        print("  %-14s" % b + "".join("  layout %d: %8.3g (%s)" % ((lay,) + _WORST[(lay, b)])
                                      for lay in (0, 1) if (lay, b) in _WORST))


def _points(k, n, seed):
    """The alphas in turn, with the PCs of tests/test_derivs_gpu.py's _mixed_points -- scale 0.01 and 0.05 in turn --: the rule
    below is that module's, and its factor 32 was sized on points of that scheme."""
    rng = np.random.default_rng(seed)
    pc1, pc2 = rng.normal(0, 0.01, (n, k)), rng.normal(0, 0.01, (n, k))
    pc1[1::2] *= 5
    pc2[1::2] *= 5
    return pc1, pc2, np.array([ALPHAS[i % len(ALPHAS)] for i in range(n)])


def _eval(pair, num_point, pc1, pc2, alpha):
    """Paired.eval for any number of points per hypothesis (its steps take at most eight)."""
    num_point = np.asarray(num_point)
    first = np.concatenate([[0], np.cumsum(num_point)])
    out = np.zeros(int(first[-1]))
    for done in range(0, int(num_point.max(initial=0)), SLOTS):
        cnt = np.clip(num_point - done, 0, SLOTS)
        idx = np.concatenate([np.arange(first[h] + done, first[h] + done + cnt[h]) for h in range(len(cnt))]).astype(int)
        out[idx] = pair.eval(cnt, pc1[idx], pc2[idx], alpha[idx])
    return out


def _given_everywhere(c, hyp, side):
    """The side's triple is not all zero at every walked marker of the sample."""
    h = np.asarray(hyp, dtype=np.float32)[c.idx]
    walked = ~(h[:, 3] < 0)
    return bool(np.all(np.any(h[walked][:, 3 * side:3 * side + 3] != 0, axis=1)))


def _check(d, ctx, pair, rows, num_point, seed, label, anonymous=0, all_out=ALL_OUT):
    """Every point of one call (num_point per hypothesis) against the restatement, vb2_paired_eval and the exact zeros.
    anonymous, all_out: the rows (None: no such row) with both sides all zero / with every marker left out."""
    k = d.num_pc
    n = 2 * k + 1
    layout = ctx.info()["layout"]
    c64, c80 = Counts(d), Counts(d, np.longdouble)
    P = int(np.sum(num_point))
    pc1, pc2, alpha = _points(k, P, seed)
    llk, grad, hess = pair.derivatives(num_point, pc1, pc2, alpha)
    assert llk.shape == (P,) and grad.shape == (P, n) and hess.shape == (P, n, n)
    want_llk = _eval(pair, num_point, pc1, pc2, alpha)
    failures, p = [], 0
    for h, cnt in enumerate(num_point):
        zero1, zero2 = _given_everywhere(c64, rows[h], 0), _given_everywhere(c64, rows[h], 1)
        for _ in range(cnt):
            where = "%s hypothesis %d alpha=%g" % (label, h, alpha[p])
            assert abs(llk[p] - want_llk[p]) <= 1e-13 * abs(want_llk[p]), (where, llk[p], want_llk[p])
            assert np.array_equal(hess[p], hess[p].T)
            ref = pdr.reference(c64, c80, rows[h], pc1[p], pc2[p], alpha[p])
            for name, (dev, dev64, tol) in deriv_ref.block_devs(ref, grad[p], hess[p], alpha[p] not in (0.0, 1.0)).items():
                ratio = dev / max(dev64, deriv_ref.TOL_FLOOR / deriv_ref.TOL_FACTOR)
                if ratio > _WORST.get((layout, name), (-1.0, ""))[0]:
                    _WORST[(layout, name)] = (ratio, where)
                if not dev <= tol:
                    failures.append((ratio, name, where, "dev %.3g dev64 %.3g tol %.3g" % (dev, dev64, tol)))
            if zero1 or d.known_af is not None:
                assert np.all(grad[p, :k] == 0.0) and np.all(hess[p, :k, :] == 0.0), where
            if zero2 or d.known_af is not None:
                assert np.all(grad[p, k:2 * k] == 0.0) and np.all(hess[p, k:2 * k, :] == 0.0), where
            if h == all_out:
                assert llk[p] == 0.0 and np.all(grad[p] == 0.0) and np.all(hess[p] == 0.0), where
            p += 1
    assert not failures, sorted(failures, reverse=True)[:6]
    # both sides all zero and nothing left out: the anonymous kernels' bits
    first = np.concatenate([[0], np.cumsum(num_point)])
    if anonymous is not None and num_point[anonymous]:
        s = slice(int(first[anonymous]), int(first[anonymous + 1]))
        for x, y in zip((llk[s], grad[s], hess[s]), ctx.derivatives(pc1[s], pc2[s], alpha[s])):
            assert np.array_equal(x, y), label
    return llk, grad, hess


# points per hypothesis: 0 (it sits the call out), 1, 4 (a full chunk), 5 and 9 (a chunk and one; two chunks and one); the
# second call moves them round so that every row meets every alpha
CALLS = [[9, 1, 4, 5, 4, 1, 0, 5, 4, 9], [5, 4, 0, 1, 9, 5, 4, 1, 1, 0]]


def _one_hot_rows_are_given_everywhere(d, rows):
    c = Counts(d)
    return all(_given_everywhere(c, rows[h], 1) and not _given_everywhere(c, rows[h], 0) for h in (1, 2, 3))


@pytest.mark.parametrize("M, k, pd", [(1, 2, 1), (17, 1, 0), (17, 4, 1), (33, 2, 0), (33, 2, 1), (300, 4, 0), (3000, 2, 0),
                                      (3000, 2, 1)])
def test_derivatives_match_the_restatement(M, k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=k, alpha_true=0.05, seed=100 + M + k)
    rows = _hyp_rows(d, M + 1)
    assert _one_hot_rows_are_given_everywhere(d, rows)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["layout"] == pd
        before = pair.info()["device_bytes"]
        for s, num_point in enumerate(CALLS if M <= 300 else CALLS[:1]):
            _check(d, ctx, pair, rows, num_point, seed=M + s, label="%dx30 k=%d" % (M, k))
        # the per-hypothesis marker scratch is counted
        assert pair.info()["device_bytes"] >= before + 10 * 4 * 10 * 8 * ctx.info()["num_active_marker"]


@pytest.mark.parametrize("pd", [0, 1])
def test_derivatives_with_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(300, mean_depth=25, num_pc=2, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, 300), 0.0, 1.0)
    rows = _hyp_rows(d, 3)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["layout"] == pd
        _check(d, ctx, pair, rows, CALLS[0], seed=5, label="known AF")


def test_derivatives_of_a_sample_that_takes_run_words_whatever_the_switch(tunable):
    """Three markers deeper than the probability-domain bound among 300 ordinary ones, and quality-0 reads."""
    tunable("pd", 1)
    a = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=31, q_lo=0, q_hi=40)
    b = vb.synth.make_pileup(3, mean_depth=1000, num_pc=2, alpha_true=0.05, seed=32)
    d = vb.PileupData(2, np.concatenate([a.ud, b.ud]), np.concatenate([a.means, b.means]),
                      np.concatenate([a.read_off, a.read_off[-1] + b.read_off[1:]]), np.concatenate([a.bases, b.bases]),
                      np.concatenate([a.quals, b.quals]), np.concatenate([a.alt_base, b.alt_base]), None, a.avg_depth, 0.0, True)
    rows = _hyp_rows(d, 9)
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["layout"] == 0
        _check(d, ctx, pair, rows, CALLS[0], seed=6, label="deep + q0")


@pytest.mark.parametrize("M, pd", [(17, 0), (17, 1), (33, 1)])
def test_every_single_marker_left_out_in_turn(M, pd, tunable):
    """Hypothesis m leaves out panel marker m alone: whatever the context's order, one of them is the first marker of a
    16-marker tile, one its last, one the lone marker of the last tile."""
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30, num_pc=2, alpha_true=0.05, seed=40 + M)
    q = _other_q(d, 2)
    rows = np.stack([pr.hypothesis(M, pi2=q) for _ in range(M)])
    for m in range(M):
        rows[m, m, 3:] = pr.LEFT_OUT
    with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
        assert ctx.info()["num_active_marker"] == M
        _check(d, ctx, pair, rows, [1] * M, seed=3, label="%d markers, one left out" % M, anonymous=None, all_out=None)


def _same_bits(x, y, what):
    for u, v in zip(x, y):
        assert np.array_equal(u, v), what


@pytest.mark.parametrize("pd", [0, 1])
def test_the_bits_of_a_point(pd, tunable):
    """One hypothesis's point gives the same bits alone (the single-sample launch), as the ninth point of its hypothesis,
    beside three other hypotheses (the job-table launch), beside a hypothesis on another context and on a second call."""
    tunable("pd", pd)
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=77)
    rows = _hyp_rows(d, 5)
    H = len(rows)
    pc1, pc2, alpha = _points(2, 9, 21)
    mine = 6                                                      # walked, left-out and fallback markers side by side
    tunable("pd", 1 - pd)
    other = vb.synth.make_pileup(700, mean_depth=25, num_pc=2, alpha_true=0.1, seed=78)
    with vb.LikelihoodContext(other) as octx, vb.Paired(octx, _hyp_rows(other, 6)[4:6]) as opair:
        assert octx.info()["layout"] == 1 - pd                    # (the other layout class: two marker launches, one reduction)
        tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
            assert ctx.info()["layout"] == pd

            def only(h, n):
                return [n if i == h else 0 for i in range(H)]
            nine = pair.derivatives(only(mine, 9), pc1, pc2, alpha)
            for b in (0, 3, 4, 8):
                alone = pair.derivatives(only(mine, 1), pc1[b:b + 1], pc2[b:b + 1], alpha[b:b + 1])
                _same_bits(alone, [x[b:b + 1] for x in nine], "alone / point %d of nine" % b)
            _same_bits(pair.derivatives(only(mine, 9), pc1, pc2, alpha), nine, "a second call")
            # beside three other hypotheses, one point each, the ninth of mine last
            num = [1 if i in (0, 4, 9) else 0 for i in range(H)]
            num[mine] = 1
            order = sorted(i for i in range(H) if num[i])
            at = order.index(mine)
            sel = [0, 1, 2, 8]
            sel[at], sel[3] = sel[3], sel[at]
            beside = pair.derivatives(num, pc1[sel], pc2[sel], alpha[sel])
            _same_bits([x[at:at + 1] for x in beside], [x[8:9] for x in nine], "beside three hypotheses")
            # beside a hypothesis on another context
            both = vb.Paired.derivatives_sets([opair, pair], [2, 1] + only(mine, 9), np.concatenate([pc1[:3], pc1]),
                                              np.concatenate([pc2[:3], pc2]), np.concatenate([alpha[:3], alpha]))
            _same_bits([x[3:] for x in both], nine, "beside another context")
            _same_bits([x[:3] for x in both], opair.derivatives([2, 1], pc1[:3], pc2[:3], alpha[:3]), "the other context's own")


def test_alpha_outside_its_range_and_no_points(tunable):
    """alpha outside [0, 1] leaves every marker out, as in section 10; a call without points touches nothing."""
    d = vb.synth.make_pileup(300, mean_depth=30, num_pc=2, alpha_true=0.05, seed=14)
    rows = _hyp_rows(d, 2)[[0, 4, 6]]
    pc1, pc2, _ = _points(2, 6, 15)
    a = np.array([-0.2, 1.3] * 3)
    for pd in (0, 1):
        tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, rows) as pair:
            llk, grad, hess = pair.derivatives([2, 2, 2], pc1, pc2, a)
            np.testing.assert_array_equal(llk, pair.eval([2, 2, 2], pc1, pc2, a))
            assert np.all(llk == 0) and np.all(grad == 0) and np.all(hess == 0)
            llk, grad, hess = pair.derivatives([0, 0, 0], pc1[:0], pc2[:0], a[:0])
            assert llk.shape == (0,)
