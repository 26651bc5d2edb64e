"""The cohort, streaming, shard-group and multi-start paths under every model of the reference (its six Optimize*
wrappers) and with a known-AF column -- test_gpu_parity.py pins those on the single-context path only; every other path
had only ever run the default model (Heter, everything free) on samples without known allele frequencies.

The independent reference everywhere is the C oracle (oracle_data(d).llk / .optimize); a sample's own single-context result
is a second check, never the only one.

Why the searches are held to the oracle's evaluation COUNT: on these inputs the oracle's own search gives the identical
alpha and the identical count under 1, 3 and 7 threads (three summation orders; llk1 moves by <= 3e-15 relative), for all
seven models on each of the three base samples -- so a last-bit difference between a cohort's sums and the oracle's does
not move the reference's own trajectory.  Tolerances: LLK_RTOL (1e-12) per evaluation and the north-star 1e-4 on alpha, as
test_gpu_parity.py defines them; llk1 / llk0 to 1e-9 relative and the PCs to 1e-4 as test_c2_optimize_vs_oracle holds them.

Measured on an MI355X (the tests print these, pytest -s): see the paragraph in DESIGN.md's cohort section.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from oracle.bridge import oracle_data

import test_gpu_parity as parity
from test_gpu_parity import LLK_RTOL, NORTH_STAR_ALPHA_ATOL, rel_err

pytestmark = pytest.mark.gpu

BASE_SPECS = [(3000, 25, 0.02, 61), (1200, 8, 0.15, 62), (2000, 30, 0.0, 65)]
MODEL_NAMES = ["heter", "homo", "heter-fixalpha", "homo-fixalpha", "heter-fixpc", "homo-fixpc", "known-af"]


def model_kw(name, k=3):
    """The keyword dict of a model; "known-af" is the default dict on a sample WITH a known-AF column."""
    pcs = [0.01, -0.02, 0.005, 0.0][:k]
    return {"heter": {}, "homo": dict(within_ancestry=True), "heter-fixalpha": dict(fix_alpha=0.07),
            "homo-fixalpha": dict(within_ancestry=True, fix_alpha=0.07), "heter-fixpc": dict(fix_pc=pcs),
            "homo-fixpc": dict(within_ancestry=True, fix_pc=pcs), "known-af": {}}[name]


def known_af_twin(d, seed):
    """The same arrays plus a known-AF column (uniform, clipped: nothing like mu / 2 -- a sample that read the panel instead
    of the column, or the column at another marker's offset, is far off)."""
    rng = np.random.default_rng(seed)
    return vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base,
                         np.clip(rng.uniform(0, 1, d.num_marker), 0.01, 0.99), d.avg_depth, d.sd_depth, True, {})


@functools.lru_cache(maxsize=None)
def sample(k, i, kaf=False):
    """Base sample i (0..2; "empty": no reads at all) at --NumPC k, or its known-AF twin."""
    if i == "empty":
        return vb.synth.make_pileup(50, 10, k, seed=66, missing_frac=1.0)
    M, depth, alpha, seed = BASE_SPECS[i]
    d = vb.synth.make_pileup(M, depth, k, alpha_true=alpha, seed=seed)
    return known_af_twin(d, 1000 + seed) if kaf else d


@functools.lru_cache(maxsize=None)
def oracle(k, i, kaf=False):
    return oracle_data(sample(k, i, kaf))


@functools.lru_cache(maxsize=None)
def oracle_search(k, i, name):
    """The oracle's search of base sample i under a model -- computed once, shared by the tests, never changed."""
    return oracle(k, i, name == "known-af").optimize(**model_kw(name, k))


def oracle_llks(od, pc1, pc2, al):
    return np.array([od.llk(pc1[j], pc2[j], al[j]) for j in range(len(al))])


def assert_search_is_the_oracles(est, ref, tag):
    print("%s: alpha %.9f (oracle %.9f), llk1 rel %.1e, num_eval %d (oracle %d)"
          % (tag, est["alpha"], ref["alpha"], abs(est["llk1"] - ref["llk1"]) / abs(ref["llk1"]), est["num_eval"], ref["num_eval"]))
    assert abs(est["alpha"] - ref["alpha"]) <= NORTH_STAR_ALPHA_ATOL, tag
    assert abs(est["llk1"] - ref["llk1"]) <= 1e-9 * abs(ref["llk1"]), tag
    assert abs(est["llk0"] - ref["llk0"]) <= 1e-9 * abs(ref["llk0"]), tag
    assert np.allclose(est["pc"], ref["pc"], rtol=0, atol=1e-4) and np.allclose(est["pc2"], ref["pc2"], rtol=0, atol=1e-4), tag
    assert est["num_eval"] == ref["num_eval"], tag
    assert est["converged"] == 1 and ref["converged"], tag


def assert_search_is_the_samples_own(est, one, tag):
    assert abs(est["alpha"] - one["alpha"]) <= 1e-6, tag
    assert abs(est["llk1"] - one["llk1"]) <= 1e-9 * max(1.0, abs(one["llk1"])), tag


def _w16_switch():
    lib = _abi.lib()
    lib.vb2_debug_set_cohort_w16.argtypes = [ctypes.c_int]
    lib.vb2_debug_set_cohort_w16.restype = None
    return lib.vb2_debug_set_cohort_w16


# ------------------------------------------------------------------ (a) the known-AF column in every cohort kernel shape

STEP_SHAPES = ([1] * 5, [2] * 5, [4] * 5, [8] * 5, [1, 4, 0, 2, 3], [5, 8, 0, 7, 6])
# slot -> (base sample, known-AF twin?)
COMPOSITIONS = {"all-known-af": [(0, True), (1, True), (2, True), (0, True), (1, True)],
                "known-af-at-1-and-3": [(0, False), (1, True), ("empty", False), (2, True), (1, False)],
                "known-af-first-and-last": [(0, True), (1, False), (2, False), (0, False), (2, True)],
                # the mixed batch without its known-AF samples: at --NumPC 2 / 4 the other side of Batch::launch_step's choice
                # between the kernels compiled for that k and the general ones (one known-AF sample flips the whole launch)
                "plain": [(0, False), ("empty", False), (1, False)]}


@pytest.mark.parametrize("pd", [0, 1])
@pytest.mark.parametrize("k", [3, 2, 4])
def test_known_af_column_in_every_cohort_kernel_shape(k, pd, tunable):
    """Batches of five contexts -- all with a known-AF column; mixed with the column at slots 1 and 3 and a sample without
    reads between them; mixed with the column first and last; and the mixed batch without its known-AF samples -- in the four
    wave shapes (1, 2, 4, 8 points) and two ragged steps, on 32-bit and on short lists, in both layouts.  Every value is the
    oracle's to LLK_RTOL; a repeated call and the other list width give the same bits; and a known-AF sample's values are the
    same bits whatever PCs it is handed, because it must not read them."""
    tunable("pd", pd)
    set_w16 = _w16_switch()
    keys = sorted({key for comp in COMPOSITIONS.values() for key in comp}, key=str)
    ctxs = {key: vb.LikelihoodContext(sample(k, *key)) for key in keys}
    worst = 0.0
    try:
        for key, c in ctxs.items():
            if key[0] != "empty":
                assert c.info()["layout"] == pd, key
        for name, comp in COMPOSITIONS.items():
            S = len(comp)
            rng = np.random.default_rng(200 + 10 * k + S)
            pc1, pc2 = rng.normal(0, 0.03, (S, 8, k)), rng.normal(0, 0.03, (S, 8, k))
            al = rng.uniform(0, 0.5, (S, 8))
            other1, other2 = pc1.copy(), pc2.copy()              # other PCs for the known-AF samples, the same for the rest
            for s, (_, kaf) in enumerate(comp):
                if kaf:
                    other1[s], other2[s] = rng.normal(0, 0.5, (8, k)), rng.normal(0, 0.5, (8, k))
            want = np.array([oracle_llks(oracle(k, *comp[s]), pc1[s], pc2[s], al[s]) for s in range(S)])
            shapes = [sh if S == 5 else [sh[0], sh[2], sh[4]] for sh in STEP_SHAPES]
            got = {}
            for w16 in (0, 1):
                set_w16(w16)
                with vb.CohortBatch([ctxs[key] for key in comp]) as batch:
                    for i, sh in enumerate(shapes):
                        npt = np.array(sh, dtype=np.int32)
                        got[w16, i] = batch.eval(npt, pc1, pc2, al)
                        assert np.array_equal(got[w16, i], batch.eval(npt, pc1, pc2, al)), (name, w16, sh)
                        assert np.array_equal(got[w16, i], batch.eval(npt, other1, other2, al)), (name, w16, sh)
            for i, sh in enumerate(shapes):
                assert np.array_equal(got[0, i], got[1, i]), (name, sh)
                for s, n in enumerate(sh):
                    if n == 0:
                        continue
                    if comp[s][0] == "empty":
                        assert np.all(got[1, i][s, :n] == 0) and np.all(want[s, :n] == 0)
                        continue
                    err = rel_err(got[1, i][s, :n], want[s, :n])
                    worst = max(worst, err)
                    assert err <= LLK_RTOL, (name, sh, s, err)
    finally:
        set_w16(1)
        for c in ctxs.values():
            c.close()
    print("k = %d, pd = %d: worst relative LLK error against the oracle %.2e" % (k, pd, worst))


# ------------------------------------------------------------------ (b) the static deal with a known-AF column

@pytest.mark.parametrize("tiles", [1290, 1279], ids=["static-deal", "queue"])
def test_static_deal_and_queue_of_a_cohort_with_a_known_af_column(tiles):
    """The smallest shape that takes the static deal (test_cohort_at_the_queue_vs_static_deal_boundary: 32 slots, samples of
    16 x 1290 markers at depth 3, --NumPC 2: the pipelined item loop) and, eleven tiles below, the work queue -- three distinct
    contexts reused across the slots, one of them with a known-AF column, so the launch is mixed.  Steps of 1, 2 and 4 points:
    slots 0, 1, 2 and 31 against the oracle, every slot against its context's own evaluation."""
    k, S, M = 2, 32, 16 * tiles
    datas = [vb.synth.make_pileup(M, 3, k, alpha_true=0.05, seed=500 + i) for i in range(3)]
    datas[1] = known_af_twin(datas[1], 1501)
    ods = [oracle_data(d) for d in datas]
    rng = np.random.default_rng(13)
    pc1, pc2, al = rng.normal(0, 0.03, (S, 8, k)), rng.normal(0, 0.03, (S, 8, k)), rng.uniform(0, 0.5, (S, 8))
    ctxs = [vb.LikelihoodContext(d) for d in datas]
    worst = 0.0
    try:
        want = {s: oracle_llks(ods[s % 3], pc1[s, :4], pc2[s, :4], al[s, :4]) for s in (0, 1, 2, 31)}
        own = [ctxs[s % 3].llk(pc1[s, :4], pc2[s, :4], al[s, :4]) for s in range(S)]
        with vb.CohortBatch([ctxs[s % 3] for s in range(S)]) as batch:
            for n in (1, 2, 4):
                npt = np.full(S, n, dtype=np.int32)
                got = batch.eval(npt, pc1, pc2, al)
                assert np.array_equal(got, batch.eval(npt, pc1, pc2, al))
                for s in range(S):
                    assert rel_err(got[s, :n], own[s][:n]) <= LLK_RTOL, (n, s)
                for s, w in want.items():
                    err = rel_err(got[s, :n], w[:n])
                    worst = max(worst, err)
                    assert err <= LLK_RTOL, (n, s, err)
    finally:
        for c in ctxs:
            c.close()
    print("%d tiles: worst relative LLK error against the oracle %.2e" % (tiles, worst))


# ------------------------------------------------------------------ (c) NaN parameters through vb2_batch_eval

@pytest.mark.parametrize("n", [2, 4, 8])
def test_nan_parameters_in_a_cohort_step_follow_the_reference(n):
    """vb2_batch_eval takes a caller's points, so the rule of context.h (params_hold_nan) holds there as it does for a single
    context: a NaN alpha, or a NaN PC of a sample that reads its PCs, leaves every marker out -- LLK 0; a known-AF sample never
    reads its PCs, so NaN PCs with a valid alpha give the oracle's value.  Every other point of the step is the same bits as
    in the step with finite values in those three places (and a caller's NaN does not send the step round again as "a
    workgroup never reported")."""
    k = 3
    comp = [(0, False), (1, True), ("empty", False), (2, False), (0, True)]
    rng = np.random.default_rng(31)
    S = len(comp)
    pc1, pc2, al = rng.normal(0, 0.03, (S, 8, k)), rng.normal(0, 0.03, (S, 8, k)), rng.uniform(0, 0.5, (S, 8))
    nan = float("nan")
    bad1, bad2, bad_al = pc1.copy(), pc2.copy(), al.copy()
    bad_al[0, 1] = nan                       # NaN alpha at a point of a plain sample
    bad2[3, 0, 1] = nan                      # a NaN PC at a point of another plain sample
    bad1[4, 1, :], bad2[4, 1, 0] = nan, nan  # NaN PCs with a valid alpha at a point of a known-AF sample
    ctxs = {key: vb.LikelihoodContext(sample(k, *key)) for key in set(comp)}
    try:
        with vb.CohortBatch([ctxs[key] for key in comp]) as batch:
            npt = np.full(S, n, dtype=np.int32)
            l0 = batch_launches(batch)
            fine = batch.eval(npt, pc1, pc2, al)
            l1 = batch_launches(batch)
            got = batch.eval(npt, bad1, bad2, bad_al)
            assert batch_launches(batch) - l1 == l1 - l0 >= 1           # (no step went round again)
    finally:
        for c in ctxs.values():
            c.close()
    assert got[0, 1] == 0.0 and got[3, 0] == 0.0
    want = oracle(k, 0, True).llk(bad1[4, 1], bad2[4, 1], al[4, 1])
    assert np.isfinite(want) and rel_err([got[4, 1]], [want]) <= LLK_RTOL
    same = np.ones((S, 8), dtype=bool)
    same[:, n:] = False
    same[0, 1] = same[3, 0] = False
    assert np.array_equal(got[same], fine[same])
    assert got[4, 1] == fine[4, 1]                      # (the known-AF sample did not read the NaNs)
    assert rel_err(fine[0, :n], oracle_llks(oracle(k, 0), pc1[0, :n], pc2[0, :n], al[0, :n])) <= LLK_RTOL


def batch_launches(batch):
    lib = _abi.lib()
    lib.vb2_debug_batch_launches.argtypes = [ctypes.c_void_p]
    lib.vb2_debug_batch_launches.restype = ctypes.c_longlong
    return int(lib.vb2_debug_batch_launches(batch._h))


# ------------------------------------------------------------------ (d) lock-step search under each model

def _open_contexts(keys, k=3):
    return {key: vb.LikelihoodContext(sample(k, *key)) for key in set(keys)}


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_lockstep_search_under_each_model(name):
    """batch.optimize(**kw) over the three base samples (their known-AF twins for "known-af") plus a sample without reads:
    every sample's estimate is the oracle's under the same model -- alpha, both likelihoods, the PCs, the evaluation count --
    and its own single-context search's.  Simplexes of 2k+1 (Heter), k+1 (Homo, HeterFixedPC), 2k and k (--FixAlpha) and one
    parameter (HomoFixedPC, known AF)."""
    k, kaf, kw = 3, name == "known-af", model_kw(name)
    comp = [(0, kaf), (1, kaf), ("empty", False), (2, kaf)]
    ctxs = _open_contexts(comp)
    try:
        with vb.CohortBatch([ctxs[key] for key in comp]) as batch:
            ests = batch.optimize(**kw)
        for s, key in enumerate(comp):
            one = ctxs[key].optimize(**kw)
            if key[0] == "empty":
                for f in ("alpha", "llk1", "llk0", "num_eval", "converged"):
                    assert ests[s][f] == one[f], f
                assert np.array_equal(ests[s]["pc"], one["pc"]) and np.array_equal(ests[s]["pc2"], one["pc2"])
                continue
            assert_search_is_the_oracles(ests[s], oracle_search(k, key[0], name), (name, s))
            assert_search_is_the_samples_own(ests[s], one, (name, s))
    finally:
        for c in ctxs.values():
            c.close()


# ------------------------------------------------------------------ (e), (f) one model per sample

def per_sample_assignment(n, seed):
    """n (model, base sample) pairs: the seven models in turn, a model's copies on different base samples; shuffled with a
    fixed seed chosen so that no two neighbours share a model (neighbours differ in dimension) -- a model read from a wrong
    index is then a wrong model."""
    a = [(MODEL_NAMES[i % 7], (i % 7 + i // 7) % 3) for i in range(n)]
    a = [a[i] for i in np.random.default_rng(seed).permutation(n)]
    assert all(a[i][0] != a[i + 1][0] for i in range(n - 1))
    assert 2 * sum(m == a[0][0] for m, _ in a) < n                  # sample 0's model is not the majority's
    return a


def _search_with_a_model_per_sample(assign, tunable, knobs):
    k = 3
    comp = [(base, name == "known-af") for name, base in assign]
    ctxs = _open_contexts(comp)
    models = [model_kw(name) for name, _ in assign]
    try:
        for knob in knobs:
            tunable("cohort_regroup", knob)
            with vb.CohortBatch([ctxs[key] for key in comp]) as batch:
                ests = batch.optimize(models=models)
                regroups = parity._batch_regroups(batch)
                with pytest.raises(_abi.Vb2Error) as e:
                    batch.optimize(models=models[:3])
                assert e.value.code == _abi.VB2_ERR_INVALID and "pass 1 model or one per sample" in str(e.value)
            assert (regroups >= 1) if knob else (regroups == 0), (knob, regroups)
            for s, (name, base) in enumerate(assign):
                assert_search_is_the_oracles(ests[s], oracle_search(k, base, name), (knob, s, name, base))
    finally:
        for c in ctxs.values():
            c.close()


def test_one_model_per_sample(tunable):
    """vb2_batch_optimize_llk with num_model == num_sample: fourteen samples, each of the seven models twice on different base
    samples (known-AF models on known-AF contexts), neighbours of different dimension.  Every sample is the oracle's under
    ITS model, with the unfinished samples regrouped (the one-parameter searches end after a few dozen evaluations: slots are
    handed over at the first steps) and in the fixed batch; a list of three models is refused by the library."""
    _search_with_a_model_per_sample(per_sample_assignment(14, 1), tunable, (1, 0))


def test_one_model_per_sample_in_two_lanes(tunable):
    """Twenty samples: a cohort of 16 and more is searched as two half-cohorts taking turns, so lane 1 finds its samples'
    models and contexts at base[1] + i."""
    assign = per_sample_assignment(20, 10)
    assert assign[10][0] != assign[0][0]                              # (lane 1's first sample is not lane 0's first model)
    _search_with_a_model_per_sample(assign, tunable, (1,))


# ------------------------------------------------------------------ (g) the file flow

FILE_CASES = {"within": dict(within_ancestry=True), "fixalpha": dict(fix_alpha=0.07),
              "within-fixpc": dict(within_ancestry=True, fix_pc=[0.01, -0.02, 0.005]), "fixpc": dict(fix_pc=[0.01, -0.02, 0.005]),
              "known-af": dict()}


@pytest.fixture(scope="module")
def cohort_files(tmp_path_factory):
    """One synthetic panel, six pileups of 2 500 markers on it (as test_cohort_run_equals_per_sample_runs builds them) and a
    known-AF file."""
    tmp = tmp_path_factory.mktemp("model_paths")
    k, M = 3, 2500
    base = vb.synth.with_sanity_stats(vb.synth.make_pileup(M, 14, k, alpha_true=0.03, seed=50))
    pre = vb.synth.write_files(base, str(tmp / "panel"))
    piles = []
    for s in range(6):
        d = vb.synth.make_pileup(M, 10 + 2 * s, k, alpha_true=0.02 * (s + 1), seed=60 + s)
        d = vb.PileupData(k, base.ud, base.means, d.read_off, d.bases, d.quals, base.alt_base, None, d.avg_depth, d.sd_depth,
                          True, dict(base.meta))
        piles.append(vb.synth.write_files(d, str(tmp / ("s%d" % s))) + ".pileup")
    af = vb.synth.write_known_af(pre, str(tmp / "panel.af"), seed=3)
    return dict(k=k, pre=pre, piles=piles, af=af, tmp=tmp)


@pytest.mark.parametrize("case", list(FILE_CASES))
def test_cohort_run_under_each_model_equals_per_sample_runs(cohort_files, case, tunable):
    """--PileupList with --WithinAncestry, --FixAlpha, --FixPC (with and without --WithinAncestry) and --KnownAF: six samples
    through four slots (slots are handed over), streamed and group-at-a-time -- every sample's .selfSM and .Ancestry are byte
    for byte what vb2_run writes for it alone under the same arguments, and its alpha is the oracle's search on the Python
    restatement of the readers."""
    f, kw = cohort_files, dict(FILE_CASES[case])
    k, tmp = f["k"], f["tmp"]
    if case == "known-af":
        kw["known_af_path"] = f["af"]
    singles = []
    for s, pile in enumerate(f["piles"]):
        out = str(tmp / ("%s_single%d" % (case, s)))
        singles.append((vb.run_files(f["pre"], pile, out, num_pc=k, **kw), out))
    for stream in (1, 0):
        tunable("cohort_stream", stream)
        outs = [str(tmp / ("%s_cohort%d_%d" % (case, stream, s))) for s in range(6)]
        res = vb.run_cohort_files(f["pre"], f["piles"], outs, num_pc=k, group_size=4, **kw)
        assert [r["status"] for r in res] == [0] * 6
        for s in range(6):
            for ext in (".selfSM", ".Ancestry"):
                assert open(outs[s] + ext, "rb").read() == open(singles[s][1] + ext, "rb").read(), (case, stream, s, ext)
            ref = _oracle_file_search(f, s, case)
            assert abs(res[s]["alpha"] - ref["alpha"]) <= 1e-4, (case, stream, s, res[s]["alpha"], ref["alpha"])
            assert abs(singles[s][0]["alpha"] - ref["alpha"]) <= 1e-4


_file_refs = {}


def _oracle_file_search(f, s, case):
    """The oracle's search on the Python restatement of the readers (refio.load_flat) of the same files; once per sample."""
    from oracle import binding, refio
    key = (f["piles"][s], case)
    if key not in _file_refs:
        af = f["af"] if case == "known-af" else None
        flat, _, _ = refio.load_flat(f["pre"], f["piles"][s], f["k"], sanity_disabled=False, known_af_path=af)
        assert bool(flat.af_known) == (case == "known-af")
        _file_refs[key] = binding.OracleData(flat).optimize(**FILE_CASES[case])
    return _file_refs[key]


def test_cli_pileup_list_with_known_af(cohort_files):
    """The command line takes the same path: --PileupList with --KnownAF exits 0, prints the reference's summary block under
    "Estimation from OptimizeHomoFixedPC:" once per sample, and writes the first sample's .selfSM row as the API's run does."""
    f = cohort_files
    tmp = f["tmp"]
    lst = str(tmp / "cli_list.txt")
    outs = [str(tmp / ("cli%d" % s)) for s in range(6)]
    with open(lst, "w") as fh:
        for p, o in zip(f["piles"], outs):
            fh.write("%s\t%s\n" % (p, o))
    exe = os.path.join(parity.ROOT, "verifybamid_amd", "bin", "VerifyBamID")
    p = subprocess.run([exe, "--SVDPrefix", f["pre"], "--Reference", "x.fa", "--NumPC", str(f["k"]), "--PileupList", lst,
                        "--KnownAF", f["af"], "--Output", str(tmp / "cli")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.count("Estimation from OptimizeHomoFixedPC:") == 6
    api_out = str(tmp / "cli_api0")
    r = vb.run_files(f["pre"], f["piles"][0], api_out, num_pc=f["k"], known_af_path=f["af"])
    row = open(outs[0] + ".selfSM").read().splitlines()[1]
    assert row == open(api_out + ".selfSM").read().splitlines()[1]
    assert row.split("\t")[6] == parity.cxx_default(r["alpha"] if r["alpha"] < 0.5 else 1 - r["alpha"])
    assert ("FREEMIX(Alpha):%s" % row.split("\t")[6]) in p.stdout


# ------------------------------------------------------------------ (h) shard groups

@pytest.mark.parametrize("kaf", [False, True], ids=["plain", "known-af"])
def test_shard_group_under_each_model(kaf):
    """Three virtual shards on one device: the known-AF column is sliced per marker range like the panel's rows, the NaN rule
    has the known-AF exemption, the search runs under the caller's model -- 9 points and the searches against the oracle."""
    k = 3
    d, od = sample(k, 0, kaf), oracle(k, 0, kaf)
    rng = np.random.default_rng(23)
    B = 9
    pc1, pc2, al = rng.normal(0, 0.03, (B, k)), rng.normal(0, 0.03, (B, k)), rng.uniform(0, 0.5, B)
    with vb.ShardGroup(d, devices=[0, 0, 0]) as g:
        assert g.info()["num_shard"] == 3
        err = rel_err(g.llk(pc1, pc2, al), oracle_llks(od, pc1, pc2, al))
        print("shard group (known AF: %s): worst relative LLK error %.2e" % (kaf, err))
        assert err <= LLK_RTOL
        if kaf:
            nan = float("nan")
            n1, n2 = np.full((2, k), nan), np.array([[nan, 0.0, nan], [0.01, nan, 0.0]])
            got = g.llk(n1, n2, np.array([0.07, nan]))
            want = od.llk(n1[0], n2[0], 0.07)
            assert np.isfinite(want) and rel_err(got[:1], [want]) <= LLK_RTOL and got[1] == 0.0
        for name in (["known-af"] if kaf else ["heter", "homo-fixpc", "heter-fixalpha"]):
            assert_search_is_the_oracles(g.optimize(**model_kw(name)), oracle_search(k, 0, name), ("shards", name))


def test_shard_group_rank_mode_with_a_known_af_column():
    """Two ranks of the process-per-GPU form on the known-AF sample (tests/stub_rccl/run_case.py, the in-process stand-in for
    the collective library): each rank slices its own range of the column; both receive the oracle's sums and the oracle's
    search."""
    r = parity._stub_case("ranks", "known-af", 2)
    assert not any(r["errors"]), r["errors"]
    assert r["all_ranks_equal"] and r["equals_host_sum"]
    ref = oracle_search(3, 0, "known-af")
    for q, rk in enumerate(r["ranks"]):
        assert rk["info"] == {"num_shard": 1, "nranks": 2, "rank": q, "uses_rccl": True, "rccl_stub": True, "partial_sums": False}
        assert rk["rel_vs_fixture"] <= LLK_RTOL
        assert abs(float.fromhex(rk["est"]["alpha_hex"]) - ref["alpha"]) <= NORTH_STAR_ALPHA_ATOL
        assert abs(float.fromhex(rk["est"]["llk1_hex"]) - ref["llk1"]) <= 1e-9 * abs(ref["llk1"])
        assert rk["est"]["num_eval"] == ref["num_eval"]
    assert float.fromhex(r["want_alpha_hex"]) == ref["alpha"] and r["want_num_eval"] == ref["num_eval"]


# ------------------------------------------------------------------ (i) multi-start

@pytest.mark.parametrize("name", ["homo", "heter-fixalpha", "known-af"])
def test_multi_start_search_under_each_model(name):
    """vb2_ctx_optimize_llk_ex with six starts: run 0 IS the plain search under the same model (same bits, same count), and
    the oracle agrees with the winner's likelihood at the reported point."""
    k, kaf, kw = 3, name == "known-af", model_kw(name)
    od = oracle(k, 0, kaf)
    with vb.LikelihoodContext(sample(k, 0, kaf)) as ctx:
        plain = ctx.optimize(**kw)
        best, every = ctx.optimize_ex(num_start=6, seed=7, **kw)
    assert len(every) == 6
    for key in ("alpha", "llk1", "llk0", "num_eval"):
        assert every[0][key] == plain[key], key
    assert best["llk1"] == min(e["llk1"] for e in every) <= plain["llk1"]
    pc2 = best["pc"] if name == "homo" else best["pc2"]           # (within ancestry: one set of PCs for both samples)
    want = od.llk(best["pc"], pc2, best["alpha"])
    assert abs(-best["llk1"] - want) <= LLK_RTOL * abs(want)
    assert_search_is_the_oracles(plain, oracle_search(k, 0, name), ("single context", name))
