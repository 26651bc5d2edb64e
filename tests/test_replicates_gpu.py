"""Weighted-marker replicates on the MI355X (marker_sum_kernels.hip, replicates.cpp): vb2_replicates_eval against the pinned
oracle on EXPANDED inputs (tests/replicate_ref.py) in both layouts, the KSEL-compiled and the general --NumPC, a known-AF
column, every kind of weight row and of step; the bits of a point whatever the step holds; the lock-step searches against
the oracle's under three models; and --PerChromosome / --Bootstrap through the files.

Measured on an MI355X, the largest |kernel - oracle| / |oracle| over every evaluation case of this module, per layout (the
checks fail above LLK_RTOL = 1e-12); the module prints them at its end (pytest -s):

    layout 0 (run words)           1.8e-14  (the 49-point step, 255 on the deepest marker, alpha = 0.03)
    layout 1 (probability domain)  2.8e-14  (20 000 markers, k = 2, 255 on the shallowest marker, alpha = 1)

Searches (3 000 x 30, k = 2): alpha, llk1 and the evaluation counts are the oracle's under all three models, and the
all-ones replicate returns ctx.optimize()'s alpha exactly (difference 0).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interval_ref  # noqa: E402
import replicate_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
HAPMAP = os.path.join(ROOT, "tests", "golden", "hapmap", "hapmap_3.3.b37.dat")
LLK_RTOL = 1e-12                  # the project's evaluation tolerance (tests/test_gpu_parity.py)
ALPHAS = [0.0, 1e-6, 0.03, 0.5, 1.0]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for layout in sorted(_WORST):
        print("\nlayout %d: worst |kernel - oracle| / |oracle| = %.3g (%s)" % ((layout,) + _WORST[layout]))


def _close(got, want, layout, label, factor=1.0):
    rel = abs(got - want) / abs(want) if want != 0 else abs(got)
    if rel > _WORST.get(layout, (-1.0, ""))[0]:
        _WORST[layout] = (rel, label)
    assert rel <= factor * LLK_RTOL, (label, got, want, rel)


def _weight_rows(d, seed):
    """ones, zero, a contiguous third, its complement, counts 0..5, 255 on the shallowest marker, 255 on the deepest."""
    M = d.num_marker
    rng = np.random.default_rng(seed)
    depth = np.diff(d.read_off)
    third = np.zeros(M, dtype=np.int64)
    third[M // 3:M // 3 + (M + 2) // 3] = 1
    counts = rng.integers(0, 6, M)
    shallow = np.ones(M, dtype=np.int64)
    present = np.where(depth > 0, depth, depth.max() + 1)
    shallow[int(np.argmin(present))] = 255
    deep = np.ones(M, dtype=np.int64)
    deep[int(np.argmax(depth))] = 255
    return np.stack([np.ones(M, dtype=np.int64), np.zeros(M, dtype=np.int64), third, 1 - third, counts, shallow, deep])


def _points(k, n, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, (n, k)), rng.normal(0, scale, (n, k)), np.array([ALPHAS[i % len(ALPHAS)] for i in range(n)])


def _check_eval(d, ctx, rep, weights, steps, seed, label):
    """Every point of `steps` (lists of points per replicate) against the oracle on the replicate's expanded input."""
    layout = ctx.info()["layout"]
    ora = replicate_ref.ExpandedOracle(d, weights)
    for s, num_point in enumerate(steps):
        P = int(np.sum(num_point))
        pc1, pc2, alpha = _points(d.num_pc, P, seed + s)
        got = rep.eval(num_point, pc1, pc2, alpha)
        assert got.shape == (P,)
        p = 0
        for r, n in enumerate(num_point):
            for _ in range(n):
                want = ora.llk(r, pc1[p], pc2[p], alpha[p])
                where = "%s replicate %d alpha=%g" % (label, r, alpha[p])
                if not weights[r].any():
                    assert got[p] == 0.0 and want == 0.0, where
                else:
                    _close(got[p], want, layout, where)
                if np.all(weights[r] == 1):
                    _close(got[p], ctx.llk(pc1[p], pc2[p], alpha[p])[0], layout, where + " vs ctx.llk")
                p += 1


# points per replicate: 0 (the replicate sits the step out), 1, 4 and 8; every weight row is evaluated in some step
STEPS = [[8, 1, 4, 8, 4, 1, 0], [0, 4, 1, 0, 1, 8, 4], [1, 0, 0, 1, 0, 0, 1]]


@pytest.mark.parametrize("M, k, pd", [(1, 2, 1), (17, 1, 0), (17, 4, 1), (300, 4, 0), (300, 1, 1), (3000, 2, 0), (3000, 2, 1),
                                      (3000, 3, 1), (20000, 2, 1), (20000, 4, 0)])
def test_eval_matches_the_oracle_on_expanded_inputs(M, k, pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(M, mean_depth=30 if M < 20000 else 12, num_pc=k, alpha_true=0.05, seed=100 + M + k)
    weights = _weight_rows(d, M)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        with vb.Replicates(ctx, weights) as rep:
            info = rep.info()
            assert info["counted"].tolist() == [int((w[np.diff(d.read_off) > 0] > 0).sum()) for w in weights]
            _check_eval(d, ctx, rep, weights, STEPS if M < 20000 else STEPS[:2], seed=M, label="%dx%d k=%d" % (M, 30, k))


@pytest.mark.parametrize("pd", [0, 1])
def test_eval_with_known_allele_frequencies(pd, tunable):
    tunable("pd", pd)
    d = vb.synth.make_pileup(300, mean_depth=25, num_pc=2, alpha_true=0.05, seed=8)
    d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, 300), 0.0, 1.0)
    weights = _weight_rows(d, 3)
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, weights) as rep:
        assert ctx.info()["layout"] == pd
        _check_eval(d, ctx, rep, weights, STEPS[:2], seed=5, label="known AF")


def test_eval_of_a_sample_that_takes_run_words_whatever_the_switch(tunable):
    """Three markers deeper than the probability-domain bound (about 900 reads) among 300 ordinary ones, and quality-0 reads."""
    tunable("pd", 1)
    a = vb.synth.make_pileup(300, mean_depth=20, num_pc=2, alpha_true=0.05, seed=31, q_lo=0, q_hi=40)
    b = vb.synth.make_pileup(3, mean_depth=1000, num_pc=2, alpha_true=0.05, seed=32)
    d = vb.PileupData(2, np.concatenate([a.ud, b.ud]), np.concatenate([a.means, b.means]),
                      np.concatenate([a.read_off, a.read_off[-1] + b.read_off[1:]]), np.concatenate([a.bases, b.bases]),
                      np.concatenate([a.quals, b.quals]), np.concatenate([a.alt_base, b.alt_base]), None, a.avg_depth, 0.0, True)
    weights = _weight_rows(d, 9)
    assert weights[6][300:].max() == 255            # the deepest marker is one of the three
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, weights) as rep:
        assert ctx.info()["layout"] == 0
        _check_eval(d, ctx, rep, weights, STEPS[:2], seed=6, label="deep + q0")


def test_eval_with_missing_and_depth_filtered_markers():
    d = vb.synth.make_pileup(3000, mean_depth=20, num_pc=2, alpha_true=0.05, seed=21, missing_frac=0.15)
    d = vb.synth.with_sanity_stats(d)
    depth = np.diff(d.read_off)
    gone = (depth == 0) | (depth < d.avg_depth - 3 * d.sd_depth) | (depth > d.avg_depth + 3 * d.sd_depth)
    assert (depth == 0).sum() > 300 and gone.sum() > (depth == 0).sum() and not d.sanity_disabled
    weights = _weight_rows(d, 4)
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, weights) as rep:
        assert rep.info()["counted"].tolist() == [int((w[~gone] > 0).sum()) for w in weights]
        _check_eval(d, ctx, rep, weights, STEPS[:2], seed=7, label="missing + filtered")


@pytest.fixture(scope="module")
def sample_3000():
    return vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.05, seed=77)


@pytest.mark.parametrize("pd", [0, 1])
def test_a_step_of_49_points_and_the_bits_of_a_point(sample_3000, pd, tunable):
    """7 replicates x 7 points cross the launch boundary (48 points); one replicate's point gives the same bits alone, as
    the last of the 49, as the first of a launch and on a second call."""
    tunable("pd", pd)
    d = sample_3000
    weights = _weight_rows(d, 12)
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, weights) as rep:
        assert ctx.info()["layout"] == pd
        before = rep.info()
        _check_eval(d, ctx, rep, weights, [[7] * 7], seed=49, label="49 points")
        after = rep.info()
        assert after["num_step"] == before["num_step"] + 1 and after["num_launch"] == before["num_launch"] + 2
        pc1, pc2, alpha = _points(2, 49, 49)
        alpha[-1] = 0.03
        full = rep.eval([7] * 7, pc1, pc2, alpha)
        again = rep.eval([7] * 7, pc1, pc2, alpha)
        assert full.tobytes() == again.tobytes()
        alone = rep.eval([0, 0, 0, 0, 0, 0, 1], pc1[-1:], pc2[-1:], alpha[-1:])
        assert alone.tobytes() == full[-1:].tobytes()
        # the same point behind other replicates' points, and twice in one step
        mixed = rep.eval([3, 0, 8, 0, 0, 0, 2], np.concatenate([pc1[:11], pc1[-1:], pc1[-1:]]),
                         np.concatenate([pc2[:11], pc2[-1:], pc2[-1:]]), np.concatenate([alpha[:11], alpha[-1:], alpha[-1:]]))
        assert mixed[-1:].tobytes() == alone.tobytes() and mixed[-2:-1].tobytes() == alone.tobytes()
        # an alpha outside [0, 1] leaves every marker out, as in vb2_llk_eval_batch
        out = rep.eval([1, 0, 0, 0, 1, 0, 0], pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        want = ctx.llk(pc1[:2], pc2[:2], np.array([1.5, -0.25]))
        assert out.tobytes() == want.tobytes() or np.array_equal(out, want)


@pytest.mark.parametrize("pd", [0, 1])
def test_the_only_rows_of_a_partition_add_up_to_the_whole(sample_3000, pd, tunable):
    tunable("pd", pd)
    d = sample_3000
    nb = 5
    block = np.random.default_rng(3).integers(0, nb, d.num_marker)
    only = np.stack([(block == j).astype(np.uint8) for j in range(nb)])
    pc1, pc2, alpha = _points(2, nb, 8)
    alpha[:] = 0.04
    pc1[:], pc2[:] = pc1[0], pc2[0]
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, only) as rep:
        parts = rep.eval([1] * nb, pc1, pc2, alpha)
        whole = ctx.llk(pc1[0], pc2[0], 0.04)[0]
    assert abs(parts.sum() - whole) <= nb * LLK_RTOL * abs(whole), (parts.sum(), whole)


def test_argument_errors(sample_3000):
    d = sample_3000
    with vb.LikelihoodContext(d) as ctx:
        with pytest.raises(ValueError):
            vb.Replicates(ctx, np.ones((2, d.num_marker - 1)))
        with vb.Replicates(ctx, np.ones((2, d.num_marker))) as rep:
            with pytest.raises(_abi.Vb2Error):
                rep.eval([9, 0], np.zeros((9, 2)), np.zeros((9, 2)), np.full(9, 0.1))
            assert rep.eval([0, 0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)).shape == (0,)


MODELS = {"default": dict(), "within_ancestry": dict(within_ancestry=True), "fix_pc": dict(fix_pc=[0.01, -0.02])}


@pytest.fixture(scope="module")
def search_case(sample_3000):
    d = sample_3000
    M = d.num_marker
    third = np.zeros(M, dtype=np.int64)
    third[M // 3:2 * M // 3] = 1
    weights = np.stack([np.ones(M, dtype=np.int64), third, 1 - third, np.random.default_rng(2).integers(0, 4, M)])
    return d, weights, replicate_ref.ExpandedOracle(d, weights)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_searches_match_the_oracles(search_case, name):
    d, weights, ora = search_case
    model = MODELS[name]
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, weights) as rep:
        got = rep.optimize(**model)
        alone = ctx.optimize(**model)
        for r in range(4):
            want = ora.data(r).optimize(**model)
            g = got[r]
            print("%s replicate %d: alpha %.9g (oracle %.9g), -llk1 %.12g (oracle %.12g), %d evaluations (oracle %d)"
                  % (name, r, g["alpha"], want["alpha"], -g["llk1"], -want["llk1"], g["num_eval"], want["num_eval"]))
            assert g["status"] == 0 and g["converged"]
            assert abs(g["alpha"] - want["alpha"]) <= 1e-4, (name, r, g["alpha"], want["alpha"])
            assert abs(g["llk1"] - want["llk1"]) <= 1e-6 * abs(want["llk1"]), (name, r, g["llk1"], want["llk1"])
            pc1, pc2, _ = interval_ref.search_point(d, g, **model)
            npt = [0] * 4
            npt[r] = 1
            at = rep.eval(npt, pc1[None], pc2[None], [g["alpha"]])[0]
            assert abs(-at - g["llk1"]) <= LLK_RTOL * abs(g["llk1"]), (name, r, at, g["llk1"])
        print("%s all-ones replicate against ctx.optimize(): alpha differs by %.3g" % (name, abs(got[0]["alpha"] - alone["alpha"])))
        assert abs(got[0]["alpha"] - alone["alpha"]) <= 1e-4
        assert abs(got[0]["llk1"] - alone["llk1"]) <= 1e-6 * abs(alone["llk1"])


def test_a_replicate_without_counted_markers_fails_alone(sample_3000):
    d = sample_3000
    M = d.num_marker
    weights = np.stack([np.ones(M, dtype=np.uint8), np.zeros(M, dtype=np.uint8)])
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, weights) as rep:
        got = rep.optimize()
        want = ctx.optimize()
    assert got[1]["status"] == _abi.VB2_ERR_INVALID and got[0]["status"] == 0
    assert abs(got[0]["alpha"] - want["alpha"]) <= 1e-4


# ---- through the files: the hapmap panel (9 787 markers, 22 chromosomes), a planted chromosome ----
PLANTED_SEED = 5
PLANTED_CHR, PLANTED_ALPHA, BASE_ALPHA = "2", 0.15, 0.02


def planted_reads(seed):
    """(chrs, poss, refs, read_off, bases, quals): reads of depth 30 on the hapmap panel, chromosome 2's drawn at alpha = 0.15
    and all others at 0.02 (the same genotypes: the same seed draws them first)."""
    chrs, poss, refs, alts = vb.synth.read_bed_rows(HAPMAP + ".bed")
    mu = vb.synth.read_mu_column(HAPMAP + ".mu")
    lo = vb.synth.reads_on_panel(mu, refs, alts, 30.0, BASE_ALPHA, seed)
    hi = vb.synth.reads_on_panel(mu, refs, alts, 30.0, PLANTED_ALPHA, seed)
    planted = np.array([c == PLANTED_CHR for c in chrs])
    off = np.zeros(len(chrs) + 1, dtype=np.int64)
    bases, quals = [], []
    for i in range(len(chrs)):
        o, b, q = hi if planted[i] else lo
        bases.append(b[o[i]:o[i + 1]])
        quals.append(q[o[i]:o[i + 1]])
        off[i + 1] = off[i] + (o[i + 1] - o[i])
    return chrs, poss, refs, alts, off, np.concatenate(bases), np.concatenate(quals)


def planted_data(seed):
    """The same sample as a PileupData (k = 2) and its chromosomes: tests/test_replicates_cpu.py confirms with the oracle, on
    the chromosome-2 subset and its complement, that PLANTED_SEED plants what the GPU test asserts."""
    chrs, poss, refs, alts, off, bases, quals = planted_reads(seed)
    ud = np.loadtxt(HAPMAP + ".UD")[:, :2]
    mu = vb.synth.read_mu_column(HAPMAP + ".mu")
    d = vb.PileupData(2, ud, mu, off, bases, quals, alts, None, float(off[-1]) / len(chrs), 0.0, True)
    return vb.synth.with_sanity_stats(d), chrs


@pytest.fixture(scope="module")
def planted_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("planted")
    chrs, poss, refs, alts, off, bases, quals = planted_reads(PLANTED_SEED)
    pileup = vb.synth.write_pileup_text(str(tmp / "planted.pileup"), chrs, poss, refs, off, bases, quals)
    return tmp, pileup, chrs


def _cli(pileup, prefix, *flags):
    return subprocess.run([EXE, "--SVDPrefix", HAPMAP, "--Reference", "NA", "--PileupFile", pileup, "--Output", prefix,
                           "--NumPC", "2"] + list(flags), capture_output=True, text=True, timeout=120)


def _g(x):
    return "%g" % x


def test_a_planted_chromosome_through_the_files(planted_files):
    tmp, pileup, chrs = planted_files
    plain = _cli(pileup, str(tmp / "plain"))
    run = _cli(pileup, str(tmp / "chrom"), "--PerChromosome")
    assert plain.returncode == 0 and run.returncode == 0, run.stderr
    assert run.stdout == plain.stdout
    for ext in (".selfSM", ".Ancestry"):
        assert open(str(tmp / "chrom") + ext, "rb").read() == open(str(tmp / "plain") + ext, "rb").read()
    lines = open(str(tmp / "chrom") + ".Chrom").read().splitlines()
    assert lines[0].split("\t") == ["#CHROM", "MARKERS", "FREEMIX_ONLY", "FREELK1_ONLY", "FREELK0_ONLY", "FREEMIX_WITHOUT", "DELTA"]
    rows = [ln.split("\t") for ln in lines[1:-1]]
    names = list(dict.fromkeys(chrs))
    assert [r[0] for r in rows] == names and len(rows) == 22
    freemix = float(open(str(tmp / "plain") + ".selfSM").read().splitlines()[1].split("\t")[6])
    only = {r[0]: float(r[2]) for r in rows}
    without = {r[0]: float(r[5]) for r in rows}
    assert max(only, key=only.get) == PLANTED_CHR and min(without, key=without.get) == PLANTED_CHR
    assert float(rows[names.index(PLANTED_CHR)][6]) < 0
    foot = lines[-1].split("\t")
    assert foot[:2] == ["#JACKKNIFE", "FREEMIX"] and foot[3] == "SE" and foot[5] == "LO" and foot[7] == "HI"
    assert float(foot[6]) <= freemix <= float(foot[8]) and float(foot[4]) > 0
    # every row is what Replicates.optimize returns for chromosome_weights through the API
    d = vb.PileupData.from_files(HAPMAP, pileup, num_pc=2, disable_sanity=False)
    cw = vb.chromosome_weights(HAPMAP + ".bed", d.num_marker)
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, np.concatenate([cw["only"], cw["without"]])) as rep:
        whole = ctx.optimize()
        est = rep.optimize()
        counted = rep.info()["counted"]
    fm = lambda e: e["alpha"] if e["alpha"] < 0.5 else 1 - e["alpha"]
    for j, r in enumerate(rows):
        o, w = est[j], est[22 + j]
        assert r[1:] == [str(int(counted[j])), _g(fm(o)), _g(-o["llk1"]), _g(-o["llk0"]), _g(fm(w)), _g(fm(w) - fm(whole))], (j, r)
    je, jse = vb.jackknife(counted[:22], fm(whole), [fm(e) for e in est[22:]])
    assert foot[2] == _g(je) and foot[4] == _g(jse)
    # the same through run_files
    res = vb.run_files(HAPMAP, pileup, output_prefix=str(tmp / "api"), num_pc=2, per_chromosome=True)
    assert open(str(tmp / "api") + ".Chrom").read() == "\n".join(lines) + "\n"
    assert res["replicates"]["num_chrom"] == 22 and _g(res["replicates"]["jack_se"]) == foot[4]


def test_bootstrap_through_the_files(planted_files):
    tmp, pileup, chrs = planted_files
    plain = _cli(pileup, str(tmp / "plain2"))
    run = _cli(pileup, str(tmp / "boot"), "--Bootstrap", "8", "--Seed", "7")
    assert run.returncode == 0, run.stderr
    assert run.stdout == plain.stdout
    for ext in (".selfSM", ".Ancestry"):
        assert open(str(tmp / "boot") + ext, "rb").read() == open(str(tmp / "plain2") + ext, "rb").read()
    lines = open(str(tmp / "boot") + ".Boot").read().splitlines()
    assert lines[0].split("\t") == ["#REPLICATE", "FREEMIX", "FREELK1"] and len(lines) == 10
    d = vb.PileupData.from_files(HAPMAP, pileup, num_pc=2, disable_sanity=False)
    with vb.LikelihoodContext(d) as ctx, vb.Replicates(ctx, vb.bootstrap_weights(d.num_marker, 8, 7)) as rep:
        est = rep.optimize()
    fm = np.array([e["alpha"] if e["alpha"] < 0.5 else 1 - e["alpha"] for e in est])
    for q in range(8):
        assert lines[1 + q].split("\t") == [str(q + 1), _g(fm[q]), _g(-est[q]["llk1"])]
    s = np.sort(fm)
    foot = lines[-1].split("\t")
    assert foot == ["#BOOTSTRAP", "MEAN", _g(fm.mean()), "SD", _g(fm.std(ddof=1)), "P2.5", _g(s[int(np.floor(0.025 * 7 + 0.5))]),
                    "P97.5", _g(s[int(np.floor(0.975 * 7 + 0.5))])]


@pytest.mark.parametrize("flags, message", [
    (["--PerChromosome", "--PileupList", "list.txt"], "--PerChromosome cannot be combined with --PileupList"),
    (["--Bootstrap", "8", "--Devices", "0,1"], "--Bootstrap cannot be combined with more than one --Devices"),
])
def test_refusals(flags, message):
    p = _cli("none.pileup", "none", *flags)
    assert p.returncode != 0 and message in p.stderr and p.stdout == ""
