"""--FindSource on the MI355X (source_kernels.hip) against the numpy restatement (tests/source_ref.py).

Marginals (vb2_ctx_marginals): c, q and log L per marker against the restatement in 80-bit floats, under the derivative
tests' rule -- the worst relative deviation of an output must not exceed max(32 x dev64, 1e-13), dev64 being the float64
restatement's own worst relative deviation from the 80-bit one on the same sample and point -- in both layouts, for
--NumPC 2, 4 and 10, known allele frequencies, markers 100 to 950 reads deep, a sample that falls back to run words,
missing and depth-filtered markers; panel order with zeros exactly where the sample counts no marker; and sum_m log_l
against vb2_llk_eval_batch at 1e-12 relative.

Scores (vb2_source_set_scores): against the float64 restatement, per pair

    |S_gpu - S_64|  <=  4 x 2^-24 x sum_m (1 + |log d_m|)        d_m: the floored dot of marker m

The 4: two roundings of the stored float32 inputs, two of the products and the three-term sum of non-negative terms,
and 2^-23 relative of the logarithm's result.  The kernel takes one logarithm per marker (source_kernels.h:
kPairLogBatch = 1), so the bound has no batching term: BATCH below is the factor this test allows for, 1.  `shared`
must be exact; a pair's score the same bits in a set of 4 and in a set of 12, and from call to call.

End to end: twelve samples drawn on one synthetic panel through --PileupList --FindSource.

Measured on an MI355X (the tests print these, pytest -s): see the figures DESIGN.md section 11 records.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref  # noqa: E402
import source_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
TOL_FACTOR, TOL_FLOOR = deriv_ref.TOL_FACTOR, deriv_ref.TOL_FLOOR      # 32, 1e-13
BATCH = 1                                                               # dots per logarithm the score bound allows for
SCORE_FACTOR = 4 + (BATCH - 1)
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
    c, q, ll = ctx.marginals(pc1, pc2, alpha)
    assert c.shape == (M, 3) and q.shape == (M, 3) and ll.shape == (M,)
    c64, c80 = deriv_ref.Counts(d), deriv_ref.Counts(d, np.longdouble)
    r64 = sr.panel_order(c64, M, sr.marginals(c64, pc1, pc2, alpha))
    m80 = sr.marginals(c80, pc1, pc2, alpha)
    r80 = sr.panel_order(c80, M, m80)
    # panel order, zeros exactly where the sample counts no marker
    counted = np.zeros(M, dtype=bool)
    counted[c80.idx[m80["live"]]] = True
    assert np.array_equal(c.sum(axis=1) > 0, counted), label
    assert np.array_equal(q.sum(axis=1) > 0, counted), label
    assert np.all(c[~counted] == 0) and np.all(q[~counted] == 0) and np.all(ll[~counted] == 0)
    failures = []
    for name, got, a, b in (("c", c, r64[0], r80[0]), ("q", q, r64[1], r80[1]), ("log_l", ll, r64[2], r80[2])):
        dev, dev64 = _rel_dev(got, b), _rel_dev(a, b)
        tol = max(TOL_FACTOR * dev64, TOL_FLOOR)
        ratio = dev / max(dev64, TOL_FLOOR / TOL_FACTOR)
        print("marginals %-28s layout %d %-5s dev %.3g dev64 %.3g tol %.3g ratio %.3g" % (label, layout, name, dev, dev64, tol, ratio))
        _note("marginals %s layout %d: dev / floor" % (name, layout), ratio, "%s alpha=%g" % (label, alpha))
        if not dev <= tol:
            failures.append((name, label, dev, dev64, tol))
        # Where a value is too small for a double (q of a genotype a deep marker rules out), the float64 restatement
        # itself is 100 % off and the rule above says nothing: the same rule again over the values a double holds
        # with all its bits
        big = np.abs(b) >= 1e-280
        if name != "log_l" and not np.all(big | (b == 0)):
            dev, dev64 = _rel_dev(np.where(big, got, 0), np.where(big, b, 0)), _rel_dev(np.where(big, a, 0), np.where(big, b, 0))
            tol = max(TOL_FACTOR * dev64, TOL_FLOOR)
            print("marginals %-28s layout %d %-5s normal values only: dev %.3g dev64 %.3g tol %.3g" % (label, layout, name, dev, dev64, tol))
            _note("marginals %s layout %d: dev / floor" % (name, layout), dev / max(dev64, TOL_FLOOR / TOL_FACTOR), "%s alpha=%g, normal values" % (label, alpha))
            if not dev <= tol:
                failures.append((name + " (normal values)", label, dev, dev64, tol))
    # tied to the evaluation kernel (which is pinned to the oracle)
    want = ctx.llk(pc1, pc2, alpha)[0]
    rel = abs(ll.sum() - want) / abs(want) if want != 0 else abs(ll.sum())
    print("marginals %-28s layout %d sum log_l vs vb2_llk_eval_batch: %.3g relative" % (label, layout, rel))
    _note("sum log_l vs eval, relative", rel, label)
    assert rel <= 1e-12, (label, ll.sum(), want)
    assert not failures, failures
    return c, q, ll


def _point(k, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, k), rng.normal(0, scale, k)


@pytest.mark.parametrize("pd", [0, 1])
@pytest.mark.parametrize("k", [2, 4, 10])
def test_marginals_match_the_restatement(k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=60 + k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        for alpha in (1e-6, 0.03, 0.3):
            _check_marginals(d, ctx, *_point(k, k), alpha, "3000x30 k=%d" % k)


@pytest.mark.parametrize("pd", [0, 1])
def test_marginals_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    k = 2
    d = vb.synth.make_pileup(2000, mean_depth=30, num_pc=k, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0, 0.0, 1.0)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        a = _check_marginals(d, ctx, *_point(k, 1), 0.04, "known AF")
        b = ctx.marginals(*_point(k, 2), 0.04)                    # the PCs do not enter
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
        for alpha in (0.01, 0.2):
            _check_marginals(d, ctx, *_point(k, 3), alpha, "400x%d" % depth)


def test_marginals_of_a_sample_that_falls_back_to_run_words(tunable):
    tunable("pd", 1)
    k = 2
    d = vb.synth.make_pileup(200, mean_depth=1500, num_pc=k, alpha_true=0.1, seed=5)     # (most markers' L underflows: not counted)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 0
        _check_marginals(d, ctx, *_point(k, 7), 0.2, "200x1500 fallback")


@pytest.mark.parametrize("pd", [0, 1])
def test_marginals_missing_and_depth_filtered_markers(pd, tunable):
    tunable("pd", pd)
    k = 2
    d = vb.synth.make_pileup(3000, mean_depth=20, num_pc=k, alpha_true=0.05, seed=21, missing_frac=0.15)
    # a few markers far too deep for the +-3 sd filter
    depth = np.diff(d.read_off)
    d = vb.synth.with_sanity_stats(d)
    lo, hi = d.avg_depth - 3 * d.sd_depth, d.avg_depth + 3 * d.sd_depth
    filtered = (depth > 0) & ((depth < lo) | (depth > hi))
    assert (depth == 0).sum() > 300 and filtered.sum() > 0 and not d.sanity_disabled
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        c, q, ll = _check_marginals(d, ctx, *_point(k, 4), 0.05, "missing + filtered")
    gone = (depth == 0) | filtered
    assert np.all(c[gone] == 0) and np.all(q[gone] == 0) and np.all(ll[gone] == 0)
    assert np.all(q[~gone].sum(axis=1) > 0.999)


def test_marginals_outputs_are_optional_and_nan_counts_nothing():
    import ctypes as C
    k = 2
    d = vb.synth.make_pileup(1000, mean_depth=20, num_pc=k, alpha_true=0.05, seed=2)
    p1, p2 = _point(k, 1)
    with vb.LikelihoodContext(d) as ctx:
        c, q, ll = ctx.marginals(p1, p2, 0.05)
        only = np.zeros(1000)
        _abi.check(ctx._lib.vb2_ctx_marginals(ctx._h, p1.ctypes.data_as(C.c_void_p), p2.ctypes.data_as(C.c_void_p), 0.05,
                                              None, None, only.ctypes.data_as(C.c_void_p)), "vb2_ctx_marginals")
        assert np.array_equal(only, ll)
        cn, qn, ln = ctx.marginals(p1, p2, float("nan"))
        assert not cn.any() and not qn.any() and not ln.any()
        again = ctx.marginals(p1, p2, 0.05)
        assert np.array_equal(again[0], c) and np.array_equal(again[1], q) and np.array_equal(again[2], ll)


# ---- scores ----

def _cohort(M=4000, depth=20, seed=31, n=12, k=2):
    """n samples of one panel: 0, 1, 2 contaminated by members 5, 6, 7; sample 3 by an outsider; the rest clean."""
    panel = sr.make_panel(M, k, seed=seed)
    G = sr.draw_individuals(panel, n + 1, seed=seed + 1)
    plan = {0: (5, 0.01), 1: (6, 0.03), 2: (7, 0.10), 3: (n, 0.05)}
    data = []
    for i in range(n):
        src, alpha = plan.get(i, (n, 0.0))
        data.append(sr.make_sample(panel, G[i], G[src], depth, alpha, seed + 10 + i))
    return panel, data, plan


def _estimates(n, k, plan, seed):
    """Made-up estimates (the scores are a function of the point, whatever search found it)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        alpha = plan.get(i, (0, 0.002 + 0.001 * i))[1]
        out.append(dict(alpha=float(alpha), llk1=0.0, llk0=0.0, pc=rng.normal(0, 0.01, k), pc2=rng.normal(0, 0.01, k)))
    return out


def _check_scores(S, shared, rows, label):
    S64, sh64, bound = sr.score_matrix(rows)
    n = len(rows)
    assert np.all(np.isnan(np.diag(S)))
    assert np.array_equal(np.isnan(S), np.isnan(S64))
    assert np.array_equal(shared, sh64.astype(shared.dtype)), label
    off = ~np.isnan(S64)
    unit = 2.0 ** -24 * bound[off]
    ratio = np.abs(S[off] - S64[off]) / unit
    print("scores %-24s n=%d: worst |S_gpu - S_64| / (2^-24 sum (1 + |log d|)) = %.3g (allowed %d), largest |S| %.4g" %
          (label, n, ratio.max(), SCORE_FACTOR, np.nanmax(np.abs(S64))))
    _note("score error / (2^-24 sum(1+|log d|))", ratio.max(), label)
    assert np.all(ratio <= SCORE_FACTOR), (label, ratio.max())


def test_scores_match_the_restatement_and_do_not_depend_on_the_set(tunable):
    panel, data, plan = _cohort()
    n, k, M = len(data), panel["num_pc"], len(panel["mu"])
    est = _estimates(n, k, plan, seed=3)
    rows = [sr.sample_rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    with vb.SourceSet(M, n) as big, vb.SourceSet(M, 4) as small:
        for i, (d, e) in enumerate(zip(data, est)):
            tunable("pd", i % 2)                                      # both layouts feed one set
            with vb.LikelihoodContext(d) as ctx:
                assert big.add(ctx, e) == i
                if i in (0, 5, 6, 9):
                    small.add(ctx, e)
        S, shared = big.scores()
        _check_scores(S, shared, rows, "12 samples")
        S2, shared2 = big.scores()
        assert np.array_equal(S, S2, equal_nan=True) and np.array_equal(shared, shared2)          # call to call
        Ss, shs = small.scores()
        pick = [0, 5, 6, 9]
        assert np.array_equal(Ss, S[np.ix_(pick, pick)], equal_nan=True)                         # whatever else the set holds
        assert np.array_equal(shs, shared[np.ix_(pick, pick)])
    # the statistic does its job on these made-up points too: every contaminated target ranks its true source first
    for i, (src, _) in plan.items():
        if src < n:
            assert np.nanargmax(S[i]) == src and S[i, src] > 0


def test_scores_with_dots_below_the_floor():
    """Deep samples with a large foreign share: where the target's contaminant is surely one homozygote and the candidate
    surely the other, the dot falls far below 1e-30 (and below the float32 range) and the floor takes over."""
    panel = sr.make_panel(600, 2, seed=41)
    G = sr.draw_individuals(panel, 4, seed=42)
    data = [sr.make_sample(panel, G[0], G[1], 300, 0.3, 43), sr.make_sample(panel, G[2], G[3], 300, 0.0, 44),
            sr.make_sample(panel, G[1], G[3], 300, 0.0, 45)]
    est = [dict(alpha=0.3, pc=np.zeros(2), pc2=np.zeros(2)), dict(alpha=0.001, pc=np.zeros(2), pc2=np.zeros(2)),
           dict(alpha=0.001, pc=np.zeros(2), pc2=np.zeros(2))]
    rows = [sr.sample_rows(d, e["pc"], e["pc2"], e["alpha"]) for d, e in zip(data, est)]
    dots = (rows[0][0] * rows[1][1]).sum(axis=1)
    both = (rows[0][0].sum(axis=1) > 0) & (rows[1][1].sum(axis=1) > 0)
    floored = int((dots[both] < sr.DOT_FLOOR).sum())
    print("markers of pair (0, 1) below the floor: %d of %d" % (floored, int(both.sum())))
    assert floored >= 5
    with vb.SourceSet(600, 3) as s:
        for d, e in zip(data, est):
            with vb.LikelihoodContext(d) as ctx:
                s.add(ctx, e)
        S, shared = s.scores()
    _check_scores(S, shared, rows, "floored dots")
    assert S[0, 1] < floored * np.log(sr.DOT_FLOOR) * 0.5 and S[0, 2] > 0       # the veto is bounded; the true source stands


def test_a_target_fitted_above_one_half_scores_as_its_mirrored_twin():
    panel, data, plan = _cohort(M=3000)
    k = 2
    rng = np.random.default_rng(5)
    pc1, pc2 = rng.normal(0, 0.01, k), rng.normal(0, 0.01, k)
    rep1, rep2 = pc1.copy(), pc2.copy()
    rep1[:2], rep2[:2] = pc2[:2], pc1[:2]                       # as the estimator reports an alpha >= 0.5
    high = dict(alpha=0.96, pc=rep1, pc2=rep2)
    twin = dict(alpha=1.0 - 0.96, pc=pc2, pc2=pc1)
    other = dict(alpha=0.02, pc=np.zeros(k), pc2=np.zeros(k))
    with vb.SourceSet(3000, 3) as s:
        with vb.LikelihoodContext(data[0]) as ctx:
            s.add(ctx, high)
            s.add(ctx, twin)
        with vb.LikelihoodContext(data[1]) as ctx:
            s.add(ctx, other)
        S, shared = s.scores()
    assert S[0, 2] == S[1, 2] and S[2, 0] == S[2, 1] and shared[0, 2] == shared[1, 2]
    rows = [sr.sample_rows(data[0], rep1, rep2, 0.96), sr.sample_rows(data[0], pc2, pc1, 1.0 - 0.96),
            sr.sample_rows(data[1], other["pc"], other["pc2"], 0.02)]
    _check_scores(S, shared, rows, "alpha 0.96 and its twin")


def test_a_set_that_cannot_fit_says_how_much_it_needs():
    with pytest.raises(_abi.Vb2Error) as e:
        vb.SourceSet(1 << 24, 1 << 20)
    assert e.value.code == _abi.VB2_ERR_NOMEM
    assert str((1 << 44) * 24) in str(e.value)


# ---- end to end: --PileupList --FindSource ----

def _write_cohort(tmp, M=5000, depth=30, seed=71, extra_failing=False):
    from verifybamid_amd import synth
    panel, data, plan = _cohort(M=M, depth=depth, seed=seed)
    prefix = str(tmp / "panel")
    synth.write_files(data[0], prefix)                           # .UD / .mu / .bed (and sample 0's pileup)
    chrs, poss = ["1"] * M, 1000 + 10 * np.arange(M)
    piles, outs = [], []
    for i, d in enumerate(data):
        p = str(tmp / ("s%02d.pileup" % i))
        synth.write_pileup_text(p, chrs, poss, panel["ref"], d.read_off, d.bases, d.quals)
        piles.append(p)
        outs.append(str(tmp / ("s%02d" % i)))
    if extra_failing:                                            # 300 covered markers: fails the sanity check
        d = data[4]
        off = d.read_off.copy()
        off[301:] = off[300]
        p = str(tmp / "bad.pileup")
        synth.write_pileup_text(p, chrs, poss, panel["ref"], off, d.bases, d.quals)
        piles.insert(6, p)
        outs.insert(6, str(tmp / "bad"))
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        for p, o in zip(piles, outs):
            f.write("%s\t%s\n" % (p, o))
    return prefix, piles, outs, lst, plan


def _run_cli(prefix, lst, out, find, stream=True, top=None):
    env = dict(os.environ)
    if not stream:
        env["VB2_COHORT_STREAM"] = "0"
    args = [CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupList", lst, "--Output", out]
    if find:
        args.append("--FindSource")
    if top is not None:
        args += ["--SourceTop", str(top)]
    return subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def _read_sources(path):
    rows = {}
    with open(path) as f:
        assert f.readline().rstrip("\n").split("\t") == ["#SAMPLE", "FREEMIX", "RANK", "CANDIDATE", "LLR", "MARKERS"]
        for line in f:
            t = line.rstrip("\n").split("\t")
            rows.setdefault(t[0], []).append((float(t[1]), int(t[2]), t[3], t[4], int(t[5])))
    return rows


def _outputs(outs):
    return [open(o + ext, "rb").read() for o in outs for ext in (".selfSM", ".Ancestry")]


@pytest.mark.parametrize("stream", [True, False])
def test_end_to_end_find_source(tmp_path, stream, tunable):
    tunable("cohort_stream", 1 if stream else 0)               # (the in-process run below, like the command line's)
    prefix, piles, outs, lst, plan = _write_cohort(tmp_path)
    n = len(piles)
    plain = _run_cli(prefix, lst, str(tmp_path / "run"), find=False, stream=stream)
    assert plain.returncode == 0, plain.stderr[-2000:]
    files_plain = _outputs(outs)
    assert not os.path.exists(str(tmp_path / "run.Sources"))
    found = _run_cli(prefix, lst, str(tmp_path / "run"), find=True, stream=stream)
    assert found.returncode == 0, found.stderr[-2000:]
    # stdout, .selfSM and .Ancestry: byte for byte what the run without the flag wrote
    assert found.stdout == plain.stdout
    assert _outputs(outs) == files_plain
    # the matrix of vb2_cohort_run_sources on the same files
    res, src = vb.run_cohort_files(prefix, piles, num_pc=2, find_source=True,
                                   group_size=0)
    S, shared = src["score"], src["shared"]
    assert all(r["status"] == 0 for r in res)
    assert np.all(np.isnan(np.diag(S))) and not np.isnan(S[~np.eye(n, dtype=bool)]).any()
    table = _read_sources(str(tmp_path / "run.Sources"))
    assert sorted(table) == sorted(outs)
    for i, o in enumerate(outs):
        cand = table[o]
        assert [c[1] for c in cand] == [1, 2, 3]                                    # --SourceTop defaults to 3
        order = sorted((j for j in range(n) if j != i), key=lambda j: -S[i, j])[:3]
        assert [c[2] for c in cand] == [outs[j] for j in order]
        for c, j in zip(cand, order):
            assert c[3] == "%g" % S[i, j] and c[4] == shared[i, j]
            fm = res[i]["alpha"] if res[i]["alpha"] < 0.5 else 1 - res[i]["alpha"]
            assert "%g" % c[0] == "%g" % fm
    # the conditions of the feature
    true_llr = []
    for i, (srcj, alpha) in plan.items():
        row = S[i].copy()
        print("sample %d (alpha %.2f, source %s, fitted %.4f): best %d %+.1f, next %+.1f" %
              (i, alpha, srcj if srcj < n else "outside", res[i]["alpha"], np.nanargmax(row), np.nanmax(row),
               np.sort(row[~np.isnan(row)])[-2]))
        if srcj < n:
            assert np.nanargmax(row) == srcj and row[srcj] > 0
            others = np.delete(row, [i, srcj])
            assert np.all(others < 0), (i, others.max())
            true_llr.append(row[srcj])
        else:
            assert np.all(np.delete(row, i) < 0)                                    # the outsider: nobody here
    clean = [i for i in range(n) if i not in plan]
    worst_clean = max(np.nanmax(S[i]) for i in clean)
    print("smallest true-source LLR %+.1f, largest candidate of a clean sample %+.1f" % (min(true_llr), worst_clean))
    assert worst_clean < min(true_llr)


@pytest.mark.parametrize("top,rows", [(1, 1), (5, 5), (40, 11)])
def test_source_top_sets_the_candidates_listed(tmp_path, top, rows):
    """--SourceTop n: n candidates per sample, all eleven others when n is larger; the best one is the same whatever n."""
    prefix, piles, outs, lst, plan = _write_cohort(tmp_path, M=2000, depth=20)
    r = _run_cli(prefix, lst, str(tmp_path / "run"), find=True, top=top)
    assert r.returncode == 0, r.stderr[-2000:]
    table = _read_sources(str(tmp_path / "run.Sources"))
    assert sorted(table) == sorted(outs)
    for o in outs:
        assert [c[1] for c in table[o]] == list(range(1, rows + 1))
        llr = [float(c[3]) for c in table[o]]
        assert llr == sorted(llr, reverse=True) and o not in [c[2] for c in table[o]]
    for i, (srcj, _) in plan.items():
        if srcj < len(outs):
            assert table[outs[i]][0][2] == outs[srcj]
    # through the entry: top = 0 writes the header alone, the matrix is whole all the same
    res, src = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, find_source=True, source_top=0,
                                   sources_prefix=str(tmp_path / "none"))
    assert open(str(tmp_path / "none.Sources")).read().count("\n") == 1
    assert not np.isnan(src["score"][~np.eye(len(outs), dtype=bool)]).any()


def test_the_set_counts_its_samples_itself():
    d = vb.synth.make_pileup(1000, mean_depth=20, num_pc=2, alpha_true=0.05, seed=2)
    est = dict(alpha=0.03, pc=np.zeros(2), pc2=np.zeros(2))
    with vb.SourceSet(1000, 3) as s, vb.LikelihoodContext(d) as ctx:
        assert s.count == 0 and s.scores()[0].shape == (0, 0)
        s.add(ctx, est)
        s.add(ctx, est)
        assert s.count == 2
        S, shared = s.scores()
        assert S.shape == (2, 2) and S[0, 1] == S[1, 0] and shared[0, 1] > 900
        s.add(ctx, est)
        with pytest.raises(_abi.Vb2Error):
            s.add(ctx, est)                          # full
        assert s.count == 3


def test_a_sample_that_fails_its_sanity_check_is_nan_and_disturbs_nobody(tmp_path):
    prefix, piles, outs, lst, plan = _write_cohort(tmp_path, extra_failing=True)
    n = len(piles)
    res, src = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, find_source=True,
                                   sources_prefix=str(tmp_path / "run"))
    S, shared = src["score"], src["shared"]
    assert res[6]["status"] == _abi.VB2_ERR_SANITY and all(r["status"] == 0 for i, r in enumerate(res) if i != 6)
    assert np.all(np.isnan(S[6])) and np.all(np.isnan(S[:, 6])) and not shared[6].any() and not shared[:, 6].any()
    keep = [i for i in range(n) if i != 6]
    good = [p for i, p in enumerate(piles) if i != 6]
    res12, src12 = vb.run_cohort_files(prefix, good, num_pc=2, find_source=True)
    assert np.array_equal(S[np.ix_(keep, keep)], src12["score"], equal_nan=True)
    assert np.array_equal(shared[np.ix_(keep, keep)], src12["shared"])
    table = _read_sources(str(tmp_path / "run.Sources"))
    assert len(table[outs[6]]) == 1 and np.isnan(table[outs[6]][0][0]) and table[outs[6]][0][3] == "nan"
    assert all(outs[6] not in [c[2] for c in table[o]] for o in outs if o != outs[6])
