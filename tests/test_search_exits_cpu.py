"""The searches where they do NOT end by convergence, on the host (no GPU needed): the reference's cycle limit
(cycleMax = 50 000, MathGenMin.cpp:380-383: Minimize returns DBL_MAX and leaves `point` untouched), the exits at the head
of the first iterations, degenerate samples, the --Epsilon convention and the bytes of the non-convergence warning.

The limit is reached by the inputs, not by a knob: samples of 64 markers at depth 6 with many PCs and an --Epsilon the
simplex cannot meet within 50 000 cycles (LIMIT_CASES; the oracle's evaluation counts on this sample are in the table).
The device simplex takes contexts of 2k + 1 <= 63 parameters, so the cases have k <= 31 but for the widest (k = 60);
below k = 16 the one-phase (Homo) search converges under every positive epsilon on these samples (searched downwards with
the oracle: k = 13, 14, 15 converge at 1e-16, the tightest tolerance a relative difference of doubles can miss).
The three cases at --Epsilon 1e-16 end only when two vertices have the same double: the oracle's count there moves with
its thread count (its summation order), which does not matter here -- the evaluator IS the oracle with one thread -- but
keeps them out of test_search_exits_gpu.py, which takes "heter-k31" and "homo-k60" (identical under 1, 3 and 7 threads).

What is under test is the library's optimiser (amoeba.cpp + estimator.cpp) over the ORACLE's likelihood as evaluator: the
oracle's own search (and the reference's compiled AmoebaMinimizer where oracle/_ref is built) is the reference, bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from oracle import binding
from oracle.bridge import oracle_data

from test_abi_and_host import _capture_stderr

# statgen's warning() (Error.cpp:42-53) around MathGenMin.cpp:381
WARNING = "\n\aWARNING - \nAmoeba.Minimize - Couldn't converge in 50000 cycles\n"

# name -> (k, model, Minimize calls that hit the limit, the oracle's num_eval, speculation levels run here)
LIMIT_CASES = {
    # one phase (OptimizeHomo, 17 parameters)
    "homo": (16, dict(within_ancestry=True, epsilon=1e-16), 1, 50012, (1, 2, 4)),
    # two phases, the SECOND hits the limit (OptimizeHomoFixedAlpha converges after 4 344 evaluations;
    # OptimizeHeterFixedAlpha, 20 parameters, is one of the two wrappers that report success regardless: always_ok)
    "heter-fixalpha": (10, dict(fix_alpha=0.05, epsilon=1e-16), 1, 54358, (1, 2, 4)),
    # two phases, the FIRST hits the limit ("homo" is that phase) and the second starts again from the start point
    "heter-first-phase": (16, dict(epsilon=1e-16), 2, 100016, (1, 2, 4)),
    # the default model at the widest simplex the device takes (63 parameters); the second phase hits the limit
    # (one level here, like the widest case: the cost is the Python callback, 9 s a run)
    "heter-k31": (31, dict(epsilon=1e-12), 1, 66058, (2,)),
    # the widest case (61 parameters): one point at a time only
    "homo-k60": (60, dict(within_ancestry=True, epsilon=1e-14), 1, 50003, (1,)),
}


@functools.lru_cache(maxsize=None)
def limit_sample(k):
    return vb.synth.make_pileup(64, 6, k, alpha_true=0.1, seed=7 + k)


@functools.lru_cache(maxsize=None)
def limit_oracle(k):
    return oracle_data(limit_sample(k))


@functools.lru_cache(maxsize=None)
def oracle_limit_search(name, minimizer="oracle"):
    """The oracle's search of a limit case with its full trace -- computed once, shared, never changed."""
    k, kw = LIMIT_CASES[name][:2]
    return limit_oracle(k).optimize(trace_capacity=1 << 17, minimizer=minimizer, **kw)


def host_search(od, k, notices=0, trace_capacity=0, **kw):
    """vb2_optimize_llk over the oracle's likelihood, with vb2_model.notices as asked (one thread: the oracle's own sums)."""
    def cb(_user, n, p1, p2, a, out):
        pc1, pc2, al = np.ctypeslib.as_array(p1, (n, k)), np.ctypeslib.as_array(p2, (n, k)), np.ctypeslib.as_array(a, (n,))
        for i in range(n):
            out[i] = od.llk(pc1[i], pc2[i], al[i])
        return 0
    fn = _abi.EVAL_FN(cb)
    m, keep = vb.api._model(**kw)
    m.notices = notices
    est = _abi.Estimate()
    tb = vb.api._TraceBuf(trace_capacity, k) if trace_capacity else None
    _abi.check(_abi.lib().vb2_optimize_llk(fn, None, k, C.byref(m), C.byref(est), C.byref(tb.c) if tb else None),
               "vb2_optimize_llk")
    del keep
    out = vb.api._estimate_dict(est, k)
    if tb:
        out["trace"], out["trace_count"] = tb.result()
    return out


def assert_same_search(got, want, tag, launch_points=False):
    for key in ("alpha", "llk1", "llk0", "num_eval"):
        assert got[key] == want[key], (tag, key, got[key], want[key])
    assert bool(got["converged"]) == bool(want["converged"]), tag
    assert np.array_equal(got["pc"], want["pc"]) and np.array_equal(got["pc2"], want["pc2"]), tag
    if "trace" in want and "trace" in got:
        assert got["trace_count"] == want["trace_count"], tag
        for key in ("alpha", "pc1", "pc2", "llk"):
            assert np.array_equal(got["trace"][key], want["trace"][key]), (tag, key)


@pytest.mark.parametrize("name,level", [(n, lv) for n, c in LIMIT_CASES.items() for lv in c[4]])
def test_host_optimiser_at_the_cycle_limit(name, level, tunable):
    """amoeba.cpp:103 and the speculation that looks a round ahead, estimator.cpp's run_minimizer / Search / OptimizeLLK at a
    search that ends at cycleMax: the full trace, num_eval, alpha, llk1, llk0, both PC sets and converged == 0 are the
    oracle's, bit for bit, at every speculation level (1, 2, 4 points per round), and the reference's compiled
    AmoebaMinimizer's where oracle/_ref is built.  A phase that hit the limit leaves its start point in place: in
    "heter-first-phase" the second phase's first vertex is the start point again, which the trace pins; in
    "heter-fixalpha" the wrapper reports success regardless.  The warning is printed once per Minimize that hit the limit,
    in the reference's bytes, between that phase's "Starting phase" and "Finished phase" lines."""
    k, kw, num_warn, num_eval, _ = LIMIT_CASES[name]
    want = oracle_limit_search(name)
    assert want["num_eval"] == num_eval and not want["converged"]          # (the table above is the oracle's)
    tunable("speculate", level)
    got, err = _capture_stderr(lambda: host_search(limit_oracle(k), k, notices=1, trace_capacity=1 << 17, **kw))
    assert got["trace_count"] == got["num_eval"] < 1 << 17
    assert_same_search(got, want, (name, level))
    assert not got["converged"]
    if binding.ref_lib() is not None:
        assert_same_search(got, oracle_limit_search(name, "reference"), (name, level, "reference"))
    if level == 1:
        assert got["num_launch_point"] == got["num_eval"]
    elif level == 2:
        assert got["num_eval"] < got["num_launch_point"] <= 2 * got["num_eval"]
    else:
        assert got["num_launch_point"] > got["num_eval"]
    assert err.count(WARNING) == num_warn == err.count("WARNING"), err[-400:]
    lines = err.split("\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith("Amoeba.Minimize - ")]
    for i in at:
        before = [ln for ln in lines[:i] if ln.startswith("NOTICE -   ")][-1]
        assert before.startswith("NOTICE -   Starting phase: Optimize"), before       # (inside a search phase)
    if name == "heter-first-phase":
        # The Heter phase starts from the start point, not from where Homo stopped.  A phase's first dim + 1 evaluations
        # are its start simplex, whose vertices differ from the start point in one coordinate each: the coordinate-wise
        # median of those rows is the start point.
        n1 = oracle_limit_search("homo")["num_eval"] - 2          # ("homo" without Initialize's and the null model's call)
        tr = got["trace"]
        homo, heter = slice(1, 1 + k + 2), slice(1 + n1, 1 + n1 + 2 * k + 2)
        start = np.median(tr["pc1"][homo], axis=0)
        assert np.array_equal(np.median(tr["pc1"][heter], axis=0), start)
        assert np.array_equal(np.median(tr["pc2"][heter], axis=0), start)
        # (alpha went through Logit and InvLogit once more, as in the reference: a few units in the last place of 0.03)
        assert abs(np.median(tr["alpha"][heter]) - np.median(tr["alpha"][homo])) <= 1e-16 * 4
        assert not np.array_equal(got["pc"], start)               # (the Homo phase did move: its best point is elsewhere)


def test_nothing_is_printed_without_notices(tunable):
    """vb2_model.notices = 0: a search that hits the limit prints nothing at all (and is the same search)."""
    k, kw = LIMIT_CASES["homo"][:2]
    got, err = _capture_stderr(lambda: host_search(limit_oracle(k), k, notices=0, **kw))
    assert err == ""
    want = oracle_limit_search("homo")
    assert got["num_eval"] == want["num_eval"] and got["alpha"] == want["alpha"] and not got["converged"]


def test_lockstep_fibers_with_a_run_at_the_cycle_limit():
    """lockstep.h, as test_lockstep_fibers_give_each_run_its_own_search drives it: three OptimizeLLK searches of the "homo"
    case from jittered starts as fibers of one thread.  Run 0 is the plain search and hits the limit; among the three there
    are runs that hit it and runs that converge (run 0: 50 012 evaluations, at the limit; runs 1 and 2 converge after 12 544
    and 9 743), and runs 0 and 1 -- one of each kind -- return in a gang of two what they return among the three: their own
    flag, their own evaluation count.  The short runs are not held to the long run's."""
    k, kw = LIMIT_CASES["homo"][:2]
    od = limit_oracle(k)

    def cb(_user, n, p1, p2, a, out):
        pc1, pc2, al = np.ctypeslib.as_array(p1, (n, k)), np.ctypeslib.as_array(p2, (n, k)), np.ctypeslib.as_array(a, (n,))
        for i in range(n):
            out[i] = od.llk(pc1[i], pc2[i], al[i])
        return 0
    fn = _abi.EVAL_FN(cb)
    L = _abi.lib()
    L.vb2_debug_lockstep_optimize.restype = C.c_int
    L.vb2_debug_lockstep_optimize.argtypes = [_abi.EVAL_FN, C.c_void_p, C.c_int32, C.POINTER(_abi.Model), C.c_int32,
                                              C.c_int32, C.POINTER(_abi.Estimate), C.POINTER(C.c_int64)]
    m, _keep = vb.api._model(**kw)
    runs = 3
    ests = (_abi.Estimate * runs)()
    assert L.vb2_debug_lockstep_optimize(fn, None, k, C.byref(m), runs, 4, ests, None) == 0
    plain = oracle_limit_search("homo")
    for key in ("alpha", "llk1", "llk0", "num_eval"):
        assert getattr(ests[0], key) == plain[key], key
    assert ests[0].converged == 0
    assert np.array_equal(np.array(ests[0].pc[:k]), plain["pc"])
    flags = [e.converged for e in ests]
    print("lock-step runs: converged %s, num_eval %s" % (flags, [e.num_eval for e in ests]))
    assert flags[0] == 0 and flags[1] == 1, flags         # (run 1 converges next to the long run 0: compared alone below)
    alone = (_abi.Estimate * 2)()
    assert L.vb2_debug_lockstep_optimize(fn, None, k, C.byref(m), 2, 4, alone, None) == 0
    for i in (0, 1):
        for key in ("alpha", "llk1", "llk0", "num_eval", "converged"):
            assert getattr(alone[i], key) == getattr(ests[i], key), (i, key)


# ------------------------------------------------------------------ exits at the head of the first iterations

def _early_sample():
    return vb.synth.make_pileup(48, 8, 2, alpha_true=0.1, seed=9)


@pytest.mark.parametrize("level", [1, 2, 4])
@pytest.mark.parametrize("epsilon,num_eval", [(1.0, None), (3.0, 12)])
def test_search_that_ends_in_its_first_iterations(epsilon, num_eval, level, tunable):
    """--Epsilon 1 ends each phase after a few iterations; --Epsilon 3 is more than the relative difference of two values
    can be (rtol <= 2), so each phase ends at the head of its first iteration: Initialize's call, the k + 2 = 4 vertices of
    Homo, the 2k + 2 = 6 of Heter and the null model's call -- 12 evaluations.  The library's search is the oracle's."""
    d = _early_sample()
    od = oracle_data(d)
    want = od.optimize(trace_capacity=256, epsilon=epsilon)
    assert want["converged"] and (num_eval is None or want["num_eval"] == num_eval)
    tunable("speculate", level)
    got = host_search(od, 2, trace_capacity=256, epsilon=epsilon)
    assert_same_search(got, want, (epsilon, level))
    assert got["converged"]


def test_sample_without_reads():
    """No marker has a read: every likelihood is 0, the first simplex is flat and the search ends at once with
    alpha == 0.5, llk1 == 0 after the 12 evaluations above."""
    d = vb.synth.make_pileup(50, 10, 2, seed=66, missing_frac=1.0)
    assert d.num_read == 0
    od = oracle_data(d)
    want = od.optimize(trace_capacity=64)
    assert want["alpha"] == 0.5 and want["llk1"] == 0 and want["num_eval"] == 12 and want["converged"]
    assert_same_search(host_search(od, 2, trace_capacity=64), want, "no reads")


@pytest.mark.parametrize("markers,seed,num_eval", [(1, 41, 173), (2, 42, 245), (3, 43, 274)])
@pytest.mark.parametrize("level", [1, 4])
def test_samples_of_one_two_and_three_markers(markers, seed, num_eval, level, tunable):
    """With fewer markers than parameters the objective is flat in most directions: ties between vertices and shrinks
    (MathGenMin.cpp:395-419) are common.  The library's search is the oracle's, evaluation by evaluation."""
    d = vb.synth.make_pileup(markers, 10, 2, alpha_true=0.2, seed=seed)
    od = oracle_data(d)
    want = od.optimize(trace_capacity=1024)
    assert want["num_eval"] == num_eval and want["converged"]
    tunable("speculate", level)
    assert_same_search(host_search(od, 2, trace_capacity=1024), want, (markers, level))


# ------------------------------------------------------------------ the --Epsilon convention

@pytest.mark.parametrize("epsilon", [0.0, -1.0, float("nan")], ids=["zero", "negative", "nan"])
def test_epsilon_that_is_not_positive_means_the_default(epsilon):
    """include/vb2_abi.h, vb2_model.epsilon: a zero-initialised struct (and -1, and NaN) runs with the default 1e-8 -- the
    same search exactly.  (The reference would take such a value literally and run to the cycle limit; a test of the limit
    written with epsilon=0 would test nothing.)"""
    od = oracle_data(_early_sample())
    kw = dict(within_ancestry=True)
    default = host_search(od, 2, trace_capacity=1024, **kw)
    assert default["converged"] and default["num_eval"] < 1024
    assert_same_search(default, od.optimize(trace_capacity=1024, **kw), "default")
    assert_same_search(host_search(od, 2, trace_capacity=1024, epsilon=epsilon, **kw), default, epsilon)


# ------------------------------------------------------------------ what a device Minimize hands back

def test_device_minimize_at_the_limit_hands_back_the_start_point():
    """estimator.cpp, minimize_handback: after a Minimize that ran on the device the host's minimiser object holds the
    minimum the kernel found (status 1) or, at the cycle limit (status 2), the START -- the reference leaves `point` untouched
    there, and the phase after it starts from that point.  On the device this shows only when a FIRST phase hits the limit on
    a context that takes the device simplex, which no input of these shapes reaches whatever the summation order
    (test_search_exits_gpu.py), so the hand-back is pinned here through its host-only hook: handing back the kernel's last
    point at status 2 fails this test."""
    L = _abi.lib()
    L.vb2_debug_minimize_handback.restype = None
    L.vb2_debug_minimize_handback.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    dim = 17
    point, start = np.arange(1.0, dim + 1), np.full(dim, 0.01)
    for status, want in ((1, point), (2, start)):
        out = np.full(dim, np.nan)
        L.vb2_debug_minimize_handback(status, dim, point.ctypes.data, start.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, want), status
