"""The searches that end at the reference's cycle limit (cycleMax = 50 000) on every driver of the device: plain launches,
the host optimiser through the resident kernel, the simplex that lives in the kernel (status 2 of resident_kernel.inc, its
result block and device_minimizer's hand-back in estimator.cpp), the cohort's lock-step search, multi-start, weighted
replicates, conditioned refits, a shard group, the interval and the command line behind them.

The cases are two of test_search_exits_cpu.py's (LIMIT_CASES; samples of 64 markers at depth 6):

    heter-k31   k = 31, --Epsilon 1e-12                     63 parameters, the widest simplex the running resident kernel keeps
                                                            state for (llk_kernels.h: kDeviceSimplexMaxDim; a context takes the
                                                            device simplex when 2k + 1 <= 63); two phases, the second hits the
                                                            limit; 66 058 evaluations
    homo-k60    k = 60, --WithinAncestry --Epsilon 1e-14    one phase, 61 parameters, 50 003 evaluations; 2k + 1 = 121 is too
                                                            wide for the device simplex (vb2_debug_resident_nmax reads 0): the
                                                            host optimiser takes the search, which the test asserts instead

Both meet the condition test_model_paths_gpu.py states -- the oracle's search gives the identical num_eval, converged and
alpha under 1, 3 and 7 threads -- and are held to the oracle's own numbers.  No other case is: searched with the oracle over
k = 6 .. 31, epsilon 1e-12 .. 1e-16 (and 120 other seeds at k = 30, 31), a one-phase or --FixAlpha search on these samples
either converges or ends at the limit under one summation order and converges under another (the CPU file's "homo",
"heter-fixalpha" and "heter-first-phase", all at --Epsilon 1e-16, where the search ends only when the best and the worst
vertex are the SAME double).  Measured on an MI355X, those three converge on the device's sums (the k = 16 Homo search after
9 042 evaluations), so they are no limit cases there.  A conditioned refit is a lock-step gang over an evaluator and not
bound by the device simplex's width: the k = 31 sample's (32 parameters) converges after 22 903 evaluations, a k = 36
sample's ends at the limit under every summation order (test_conditioned_refit_at_the_cycle_limit has its own case).

Seconds per search, measured on an MI355X (the tests print them, pytest -s): heter-k31 1.03 with plain launches, 1.51 with
the host optimiser through the resident kernel, 1.45 on the device simplex (its wait is 20 s); homo-k60 1.05, 1.82, 1.83
(the last two are the host optimiser through the resident kernel); the interval at the non-converged estimate 0.18; the
conditioned refit 1.22 (k = 40, 48, 52 at 1e-16 there: converged after 43 119 / at the limit / at the limit).
"""
import ctypes as C
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from oracle import binding
from oracle.bridge import oracle_data

import test_gpu_parity as parity
from test_gpu_parity import LLK_RTOL, NORTH_STAR_ALPHA_ATOL, rel_err
from test_abi_and_host import _capture_stderr
from test_search_exits_cpu import LIMIT_CASES, WARNING, limit_oracle, limit_sample, oracle_limit_search

pytestmark = pytest.mark.gpu

GPU_CASES = ["heter-k31", "homo-k60"]
MAIN = "heter-k31"                      # the case of drivers 4 to 8
TRACE = 1 << 17
EST_KEYS = ("alpha", "llk1", "llk0", "num_eval", "converged")


def _lib():
    lib = _abi.lib()
    lib.vb2_debug_resident_evals.restype = C.c_longlong
    lib.vb2_debug_resident_evals.argtypes = [C.c_void_p]
    lib.vb2_debug_device_minimizes.restype = C.c_longlong
    lib.vb2_debug_device_minimizes.argtypes = [C.c_void_p]
    lib.vb2_debug_set_resident.argtypes = [C.c_void_p, C.c_int]
    lib.vb2_debug_set_device_simplex.argtypes = [C.c_void_p, C.c_int]
    lib.vb2_debug_resident_nmax.restype = C.c_int
    lib.vb2_debug_resident_nmax.argtypes = [C.c_void_p]
    return lib


def assert_same_bits(got, want, tag, trace=True):
    for key in EST_KEYS:
        assert got[key] == want[key], (tag, key, got[key], want[key])
    assert np.array_equal(got["pc"], want["pc"]) and np.array_equal(got["pc2"], want["pc2"]), tag
    if trace:
        assert got["trace_count"] == want["trace_count"] == want["num_eval"], tag
        for key in ("llk", "alpha", "pc1", "pc2"):
            assert np.array_equal(got["trace"][key], want["trace"][key]), (tag, key)


@functools.lru_cache(maxsize=None)
def plain_search(name):
    """Driver 1 on a context of its own: one launch per step, full trace -- computed once, shared, never changed."""
    k, kw = LIMIT_CASES[name][:2]
    lib = _lib()
    with vb.LikelihoodContext(limit_sample(k)) as ctx:
        lib.vb2_debug_set_resident(ctx._h, 0)
        n0 = lib.vb2_debug_resident_evals(ctx._h)
        t0 = time.perf_counter()
        est = ctx.optimize(trace_capacity=TRACE, **kw)
        est["seconds"] = time.perf_counter() - t0
        assert lib.vb2_debug_resident_evals(ctx._h) == n0 and lib.vb2_debug_device_minimizes(ctx._h) == 0
    return est


@pytest.mark.parametrize("name", GPU_CASES)
def test_three_single_context_drivers_at_the_cycle_limit(name):
    """Drivers 1 to 3 on one context: plain launches, the host optimiser through the resident kernel, the device simplex.
    alpha, llk1, llk0, num_eval, converged (0), both PC sets and the full trace are the same bits (the contract of
    test_device_simplex_equals_host_optimiser); each driver is shown to have run (no resident evaluation / resident
    evaluations and no device Minimize / one device Minimize per phase -- none for "homo-k60", too wide for it).  With a
    trace of 64 rows, shorter than the search, trace_count is still the full count and the rows are the first 64 of the
    long trace.  The reference's compiled AmoebaMinimizer over this context's values (oracle/_ref, where built) makes the
    same evaluations and hits its own limit; the oracle's search is held as assert_search_is_the_oracles holds it, with
    converged == 0 on both sides.
    A status 2 that fell through to another iteration (resident_kernel.inc:764-766) makes the device simplex of
    "heter-k31" run on: another num_eval, another trace -- this test fails.  A device Minimize that handed back its last
    point at the limit instead of the start (estimator.cpp:205) is invisible in these two cases (the phase that hits the
    limit is the last): on the device it needs a first phase at the limit on a context that takes the
    device simplex.  The resident kernel keeps simplex state only when 2k + 1 <= 63 (state_nmax is derived from the widest
    model of the context, not from the search asked for), so the 61 parameters of "homo-k60" are refused although they
    would fit, and with k <= 31 no Homo phase reaches the limit whatever the summation order (module docstring);
    test_search_exits_cpu.py pins that line through its host-only hook
    (test_device_minimize_at_the_limit_hands_back_the_start_point) and shows the restart itself on the host optimiser
    ("heter-first-phase")."""
    parity._needs_resident_mode()
    k, kw = LIMIT_CASES[name][:2]
    phases = 1 if kw.get("within_ancestry") else 2
    lib = _lib()
    plain = plain_search(name)
    assert not plain["converged"] and plain["trace_count"] == plain["num_eval"] < TRACE
    with vb.LikelihoodContext(limit_sample(k)) as ctx:
        secs = {"plain": plain["seconds"]}
        for driver in ("resident-host", "device-simplex"):
            lib.vb2_debug_set_resident(ctx._h, 1)
            lib.vb2_debug_set_device_simplex(ctx._h, 1 if driver == "device-simplex" else 0)
            n_res, n_min = lib.vb2_debug_resident_evals(ctx._h), lib.vb2_debug_device_minimizes(ctx._h)
            t0 = time.perf_counter()
            est = ctx.optimize(trace_capacity=TRACE, **kw)
            secs[driver] = time.perf_counter() - t0
            # the widest simplex the resident kernel of that search kept state for, read from the context (0: none)
            on_device = driver == "device-simplex" and lib.vb2_debug_resident_nmax(ctx._h) >= 2 * k + 1
            assert on_device == (driver == "device-simplex" and name == MAIN), (name, driver, lib.vb2_debug_resident_nmax(ctx._h))
            if not on_device:
                assert lib.vb2_debug_device_minimizes(ctx._h) == n_min
                assert lib.vb2_debug_resident_evals(ctx._h) > n_res + 10000
            else:
                assert lib.vb2_debug_device_minimizes(ctx._h) == n_min + phases        # (no fall-back to the host)
            assert_same_bits(est, plain, (name, driver))
            assert est["num_launch_point"] == plain["num_launch_point"], (name, driver)
            if name != MAIN:
                continue                                  # (the host optimiser's short trace: pinned with "heter-k31")
            n_min = lib.vb2_debug_device_minimizes(ctx._h)
            short = ctx.optimize(trace_capacity=64, **kw)
            assert_same_bits(short, plain, (name, driver, "short trace"), trace=False)
            assert short["trace_count"] == plain["trace_count"] and len(short["trace"]["llk"]) == 64
            for key in ("llk", "alpha", "pc1", "pc2"):
                assert np.array_equal(short["trace"][key], plain["trace"][key][:64]), (name, driver, key)
            if on_device:
                assert lib.vb2_debug_device_minimizes(ctx._h) == n_min + phases
        print("%s: %d evaluations, seconds %s" % (name, plain["num_eval"], {d: round(s, 2) for d, s in secs.items()}))
        assert secs["device-simplex"] < 10.0          # (well under device_minimize's 20-second wait)
        if binding.ref_lib() is not None:
            ref = binding.reference_optimiser_on_gpu(_abi.lib(), ctx._h, k, trace_capacity=TRACE, **kw)
            for key in ("alpha", "llk1", "num_eval"):
                assert ref[key] == plain[key], (name, "reference on the device's values", key)
            assert ref["trace_count"] == plain["trace_count"]
            for key in ("llk", "alpha", "pc1", "pc2"):
                assert np.array_equal(ref["trace"][key], plain["trace"][key]), (name, "reference", key)
    want = oracle_limit_search(name)
    assert not want["converged"] and not plain["converged"]
    assert abs(plain["alpha"] - want["alpha"]) <= NORTH_STAR_ALPHA_ATOL
    assert abs(plain["llk1"] - want["llk1"]) <= 1e-9 * abs(want["llk1"])
    assert abs(plain["llk0"] - want["llk0"]) <= 1e-9 * abs(want["llk0"])
    assert plain["num_eval"] == want["num_eval"]


def test_cohort_search_with_one_sample_at_the_cycle_limit(tunable):
    """Driver 4, vb2_batch_optimize_llk with the unfinished samples regrouped: the "heter-k31" sample between two samples
    that converge (--WithinAncestry at the default --Epsilon) and a sample without reads, one model per sample.  The long
    sample's estimate is its plain run's, bit for bit, converged == 0; the others are their own single-context runs (the
    same evaluation count; alpha and the likelihoods as assert_search_is_the_samples_own holds them), converged == 1: they
    are not held to the long sample's flag.  Measured on an MI355X: 1.25 s, 2 regroups."""
    k, kw = LIMIT_CASES[MAIN][:2]
    plain = plain_search(MAIN)
    datas = [vb.synth.make_pileup(64, 6, k, alpha_true=0.1, seed=301), limit_sample(k),
             vb.synth.make_pileup(64, 6, k, seed=66, missing_frac=1.0), vb.synth.make_pileup(64, 6, k, alpha_true=0.1, seed=302)]
    models = [dict(within_ancestry=True), kw, dict(within_ancestry=True), dict(within_ancestry=True)]
    tunable("cohort_regroup", 1)
    ctxs = [vb.LikelihoodContext(d) for d in datas]
    try:
        with vb.CohortBatch(ctxs) as batch:
            t0 = time.perf_counter()
            ests = batch.optimize(models=models)
            print("cohort of four with one sample at the limit: %.2f s, %d regroups"
                  % (time.perf_counter() - t0, parity._batch_regroups(batch)))
        assert_same_bits(ests[1], plain, "batch slot of the long sample", trace=False)
        assert not ests[1]["converged"]
        for s in (0, 2, 3):
            one = ctxs[s].optimize(**models[s])
            assert one["converged"] and ests[s]["converged"], s
            assert ests[s]["num_eval"] == one["num_eval"] < 30000, s
            if s == 2:                                    # (no reads: nothing to sum, the same bits)
                for key in EST_KEYS:
                    assert ests[s][key] == one[key], (s, key)
                continue
            # (a cohort step sums in another order than a single context's launch: assert_search_is_the_samples_own's bounds)
            assert abs(ests[s]["alpha"] - one["alpha"]) <= 1e-6, s
            assert abs(ests[s]["llk1"] - one["llk1"]) <= 1e-9 * max(1.0, abs(one["llk1"])), s
            assert abs(ests[s]["llk0"] - one["llk0"]) <= 1e-9 * max(1.0, abs(one["llk0"])), s
        assert ests[2]["alpha"] == 0.5 and ests[2]["llk1"] == 0
    finally:
        for c in ctxs:
            c.close()


def test_lockstep_drivers_on_one_context_at_the_cycle_limit():
    """Drivers 5 and 6 on the "heter-k31" case:
    optimize_ex(num_start=3) -- start 0 IS the plain run, same bits, converged == 0 (the jittered starts are other
    searches: their flags are printed, not pinned);
    vb2_replicates_optimize_llk with an all-ones replicate and one with every fourth marker counted twice -- status 0 for
    both and converged == 0 for the all-ones one, which is the plain run to the tolerances of test_replicates_gpu.py
    (1e-4 on alpha, 1e-6 relative on llk1): a refit that hit the limit is reported, not dropped.
    Measured on an MI355X: multi-start 1.65 s (all three starts at the limit), replicates 1.81 s (66 058 and 68 089
    evaluations, both at the limit)."""
    k, kw = LIMIT_CASES[MAIN][:2]
    plain = plain_search(MAIN)
    d = limit_sample(k)
    with vb.LikelihoodContext(d) as ctx:
        t0 = time.perf_counter()
        best, every = ctx.optimize_ex(num_start=3, seed=7, **kw)
        t_ms = time.perf_counter() - t0
        for key in EST_KEYS:
            assert every[0][key] == plain[key], key
        assert np.array_equal(every[0]["pc"], plain["pc"]) and not every[0]["converged"]
        assert best["llk1"] == min(e["llk1"] for e in every) <= plain["llk1"]
        print("multi-start: %.2f s, converged %s" % (t_ms, [e["converged"] for e in every]))

        w = np.ones((2, d.num_marker), dtype=np.uint8)
        w[1, ::4] = 2
        with vb.Replicates(ctx, w) as rep:
            t0 = time.perf_counter()
            got = rep.optimize(**kw)
            print("replicates: %.2f s, converged %s, num_eval %s"
                  % (time.perf_counter() - t0, [g["converged"] for g in got], [g["num_eval"] for g in got]))
        assert [g["status"] for g in got] == [0, 0]
        assert not got[0]["converged"]
        assert abs(got[0]["alpha"] - plain["alpha"]) <= 1e-4
        assert abs(got[0]["llk1"] - plain["llk1"]) <= 1e-6 * abs(plain["llk1"])


def test_shard_group_at_the_cycle_limit():
    """Driver 8, ShardGroup(d, devices=[0, 0]) on the "heter-k31" case: two virtual shards, sums met on the host --
    converged == 0, and the estimate is the sample's own plain run as assert_search_is_the_samples_own holds it (1e-6 on
    alpha, 1e-9 relative on llk1).  Measured on an MI355X: 1.19 s, 66 058 evaluations."""
    k, kw = LIMIT_CASES[MAIN][:2]
    plain = plain_search(MAIN)
    with vb.ShardGroup(limit_sample(k), devices=[0, 0]) as g:
        assert g.info()["num_shard"] == 2
        t0 = time.perf_counter()
        est = g.optimize(**kw)
        print("shard group: %.2f s, %d evaluations" % (time.perf_counter() - t0, est["num_eval"]))
    assert not est["converged"]
    assert abs(est["alpha"] - plain["alpha"]) <= 1e-6
    assert abs(est["llk1"] - plain["llk1"]) <= 1e-9 * max(1.0, abs(plain["llk1"]))


def test_context_after_a_search_at_the_cycle_limit():
    """After the device simplex ended with status 2 on a context: vb2_ctx_interval on the non-converged estimate returns and
    prints its NOTICE; plain evaluations on the context are the oracle's; a search at the default --Epsilon on the same
    context converges and equals a fresh context's, bit for bit."""
    parity._needs_resident_mode()
    k, kw = LIMIT_CASES[MAIN][:2]
    d, od = limit_sample(k), limit_oracle(k)
    lib = _lib()
    with vb.LikelihoodContext(d) as fresh:
        want = fresh.optimize(within_ancestry=True, trace_capacity=TRACE)
    assert want["converged"]
    with vb.LikelihoodContext(d) as ctx:
        n0 = lib.vb2_debug_device_minimizes(ctx._h)
        est = ctx.optimize(**kw)
        assert lib.vb2_debug_device_minimizes(ctx._h) == n0 + 2 and not est["converged"]

        def interval():
            m, keep = vb.api._model(known_af=False, **kw)
            m.notices = 1
            ci = _abi.Interval()
            rc = lib.vb2_ctx_interval(ctx._h, C.byref(m), C.byref(vb.api._estimate_struct(est, k)), C.byref(ci))
            return rc, ci
        t0 = time.perf_counter()
        (rc, ci), err = _capture_stderr(interval)
        print("interval at the non-converged estimate: %.2f s, rc %d, [%g, %g]" % (time.perf_counter() - t0, rc, ci.lo, ci.hi))
        assert rc == 0, _abi.lib().vb2_last_error()
        assert "the search did not converge: the interval is computed at its best point all the same" in err
        assert ci.freemix == min(est["alpha"], 1 - est["alpha"])
        assert (np.isnan(ci.lo) or 0 <= ci.lo <= ci.freemix) and (np.isnan(ci.hi) or ci.freemix <= ci.hi <= 0.5)
        rng = np.random.default_rng(5)
        pc1, pc2, al = rng.normal(0, 0.03, (5, k)), rng.normal(0, 0.03, (5, k)), rng.uniform(0, 0.5, 5)
        ref = np.array([od.llk(pc1[i], pc2[i], al[i]) for i in range(5)])
        assert rel_err(ctx.llk(pc1, pc2, al), ref) <= LLK_RTOL
        n0 = lib.vb2_debug_device_minimizes(ctx._h)
        again = ctx.optimize(within_ancestry=True, trace_capacity=TRACE)
        assert lib.vb2_debug_device_minimizes(ctx._h) == n0 + 1
        assert_same_bits(again, want, "default search after the limit")
        assert again["converged"]


def test_file_flow_at_the_cycle_limit(tmp_path):
    """bin/VerifyBamID on a written panel and pileup of the "heter-k31" case (--NumPC 31 --Epsilon 1e-12): exit status 0,
    stderr holds the warning's bytes once, .selfSM and .Ancestry hold what vb2_ctx_optimize_llk gives on the same files.
    Measured on an MI355X: 1.82 s for the command."""
    k, kw = LIMIT_CASES[MAIN][:2]
    pre = vb.synth.write_files(limit_sample(k), str(tmp_path / "s"))
    d = vb.PileupData.from_files(pre, pre + ".pileup", k, disable_sanity=True)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize(**kw)
    assert not est["converged"]
    out = str(tmp_path / "out")
    exe = os.path.join(parity.ROOT, "verifybamid_amd", "bin", "VerifyBamID")
    t0 = time.perf_counter()
    p = subprocess.run([exe, "--SVDPrefix", pre, "--PileupFile", pre + ".pileup", "--Reference", "x.fa", "--NumPC", str(k),
                        "--Epsilon", "1e-12", "--DisableSanityCheck", "--Output", out], capture_output=True, timeout=120)
    print("command line: %.2f s" % (time.perf_counter() - t0))
    stderr = p.stderr.decode("latin-1")
    assert p.returncode == 0, stderr[-3000:]
    assert stderr.count(WARNING) == 1 == stderr.count("Couldn't converge"), stderr[-3000:]
    row = open(out + ".selfSM").read().splitlines()[1].split("\t")
    assert row[6] == parity.cxx_default(est["alpha"] if est["alpha"] < 0.5 else 1 - est["alpha"])
    assert open(out + ".Ancestry").read() == parity.ancestry_text(est["pc"], est["pc2"])


def test_conditioned_refit_at_the_cycle_limit():
    """Driver 7, vb2_conditioned_optimize_llk with one hypothesis (all-zero triples: the Hardy-Weinberg prior, so the
    likelihood is the plain one with the contaminant's PCs held).  The refit is a lock-step gang over an evaluator, not
    bound by the device simplex's width: make_pileup(64, 6, 36, alpha_true=0.1, seed=43) with pc1_fixed =
    default_rng(3).normal(0, 0.03, 36) at --Epsilon 1e-16 (37 free parameters).  The same driver over the oracle's
    likelihood (conditioned_with_evaluator) ends at the limit with num_eval 50 003, status 0, converged 0 under 1, 3 and 7
    oracle threads, with alpha 0.103713 / 0.107096 / 0.103777 and llk1 127.484839 / 127.481157 / 127.484800: after 50 000
    cycles in 37 dimensions the simplex has not settled, and the summation order moves alpha by 3.4e-3 and llk1 by 2.9e-5
    relative.  Pinned here: status == 0 and converged == 0 -- a refit that hit the limit is reported, not dropped --, the
    count, the reported likelihood is the oracle's at the reported point (1e-9), and alpha and llk1 within three times the
    reference's own spread (1e-2, 1e-4 relative) of the one-thread refit; the existing 1e-4 / 1e-6 of
    test_conditioned_gpu.py are for converged refits and tighter than the reference agrees with itself here.
    Measured on an MI355X: 1.22 s, 50 003 evaluations, alpha 0.106295, llk1 127.483205."""
    k = 36
    d = vb.synth.make_pileup(64, 6, k, alpha_true=0.1, seed=43)
    fixed = np.random.default_rng(3).normal(0, 0.03, k)
    ref = dict(alpha=0.10371276199092389, llk1=127.48483895420574, num_eval=50003)     # (the one-thread refit above)
    with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, np.zeros((1, d.num_marker, 3), dtype=np.float32)) as cond:
        t0 = time.perf_counter()
        (g,) = cond.optimize(fixed, epsilon=1e-16)
        print("conditioned refit: %.2f s, status %d, converged %s, num_eval %d, alpha %.6f, llk1 %.6f"
              % (time.perf_counter() - t0, g["status"], g["converged"], g["num_eval"], g["alpha"], g["llk1"]))
    assert g["status"] == 0 and not g["converged"]
    assert g["num_eval"] == ref["num_eval"]
    want = oracle_data(d).llk(fixed, g["pc2"], g["alpha"])
    assert abs(-g["llk1"] - want) <= 1e-9 * abs(want)
    assert abs(g["alpha"] - ref["alpha"]) <= 1e-2
    assert abs(g["llk1"] - ref["llk1"]) <= 1e-4 * abs(ref["llk1"])
