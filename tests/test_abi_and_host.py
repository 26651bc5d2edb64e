"""CPU tests of the product's host side (no GPU needed):

* libvb2.so loads and exports every symbol include/vb2_abi.h declares;
* without a device, compute entry points fail LOUDLY (no CPU fallback);
* the C++ optimiser (amoeba.cpp + estimator.cpp, speculative batching included)
  reproduces the oracle's evaluation trace bit for bit when fed the same objective
  (the oracle's LLK as the vb2_eval_fn callback -- the checker drives, the product's
  optimiser is what is under test);
* the C++ readers/flattening (hostio.cpp) agree with the Python restatement of the
  reference's readers (oracle/refio.py) on the golden files and on quirky inputs.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from oracle import binding, refio
from oracle.bridge import flat_from_input, oracle_data

HAPMAP = "hapmap/hapmap_3.3.b37.dat"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "vb2_abi.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(vb2_[a-z0-9_]+)\s*\(", header))
    declared -= {"vb2_eval_fn"}
    assert declared == set(_abi.SYMBOLS), declared ^ set(_abi.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.vb2_abi_version() == 7


def test_header_is_plain_c_and_struct_layouts_match_the_binding(tmp_path):
    """include/vb2_abi.h must compile as C99 (it is the FFI boundary: extern "C", PODs, no C++), and
    the ctypes structs of the Python binding must have the sizes the C compiler gives them."""
    import subprocess
    src = tmp_path / "abi_check.c"
    names = ["vb2_input", "vb2_options", "vb2_info", "vb2_model", "vb2_estimate", "vb2_trace",
             "vb2_run_args", "vb2_run_result", "vb2_cohort_args", "vb2_shard_info", "vb2_search_opts",
             "vb2_mpileup_opts"]
    src.write_text('#include <stdio.h>\n#include "vb2_abi.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   "  return 0;\n}\n")
    exe = tmp_path / "abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    sizes = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                         check=True).stdout.splitlines())
    binding = dict(vb2_input=_abi.Input, vb2_options=_abi.Options, vb2_info=_abi.Info, vb2_model=_abi.Model,
                   vb2_estimate=_abi.Estimate, vb2_trace=_abi.Trace, vb2_run_args=_abi.RunArgs,
                   vb2_run_result=_abi.RunResult, vb2_cohort_args=_abi.CohortArgs, vb2_shard_info=_abi.ShardInfo,
                   vb2_search_opts=_abi.SearchOpts, vb2_mpileup_opts=_abi.MpileupOpts)
    for n, cls in binding.items():
        assert int(sizes[n]) == C.sizeof(cls), (n, sizes[n], C.sizeof(cls))


def test_cmake_build_gives_the_same_library(tmp_path):
    """CMakeLists.txt (HIP language, gfx950, -ffp-contract=off; htslib an optional component) builds
    libvb2.so + VerifyBamID like the hand Makefile does: same ABI version, every declared symbol."""
    import shutil
    import subprocess
    if shutil.which("cmake") is None or not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("cmake / ROCm clang not available")
    b = str(tmp_path / "b")
    subprocess.run(["cmake", "-S", ROOT, "-B", b, "-DCMAKE_HIP_COMPILER=/opt/rocm/lib/llvm/bin/clang++",
                    "-DCMAKE_PREFIX_PATH=/opt/rocm"], check=True, capture_output=True, timeout=600)
    subprocess.run(["cmake", "--build", b, "-j8"], check=True, capture_output=True, timeout=1200)
    L = C.CDLL(os.path.join(b, "libvb2.so"))
    assert L.vb2_abi_version() == _abi.lib().vb2_abi_version()
    for name in _abi.SYMBOLS:
        assert hasattr(L, name), name
    assert os.access(os.path.join(b, "VerifyBamID"), os.X_OK)


def test_bam_input_without_htslib_fails_loudly(tmp_path):
    """--BamFile goes through htslib (bam_flatten.cpp, an optional CMake component).  This image has
    no htslib: the request must fail with an explanation, not fall back to anything."""
    pre = str(tmp_path / "q")
    _tiny_panel(pre)
    args, keep = vb.api._run_args(pre, None, 2, True, None, None)
    args.bam_path = b"/nonexistent/sample.bam"
    args.reference_path = b"/nonexistent/ref.fa"
    h = C.c_void_p()
    rc = _abi.lib().vb2_flat_load(C.byref(args), C.byref(h))
    assert rc == _abi.VB2_ERR_IO
    assert b"htslib" in _abi.lib().vb2_last_error()


def test_cli_knows_the_references_pileup_options(tmp_path):
    """The reference's seven "Pileup Options" (main.cpp:176-187: --min-BQ --min-MQ --adjust-MQ --max-depth
    --no-orphans --incl-flags --excl-flags) are flags of the command line: a drop-in --BamFile command line
    fails with the htslib explanation (this build has no BAM reader), never with "unknown option ... ignored";
    a repeated one is the reference's "specified more than once" error."""
    import subprocess
    exe = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
    pre = str(tmp_path / "q")
    _tiny_panel(pre)
    cmd = [exe, "--SVDPrefix", pre, "--BamFile", "/nonexistent/sample.bam", "--Reference", "/nonexistent/ref.fa",
           "--min-BQ", "20", "--min-MQ", "10", "--adjust-MQ", "50", "--max-depth", "500", "--no-orphans",
           "--incl-flags", "16", "--excl-flags", "1796", "--Output", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "htslib" in r.stderr, r.stderr
    assert "unknown option" not in r.stderr, r.stderr
    r2 = subprocess.run(cmd + ["--min-BQ", "3"], capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and "specified more than once" in r2.stderr, r2.stderr


def test_no_device_fails_loudly():
    lib = _abi.lib()
    if lib.vb2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    d = vb.synth.make_pileup(64, 10, 2, seed=3)
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.LikelihoodContext(d)
    assert ei.value.code == _abi.VB2_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.vb2_last_error() or b"gfx950" in lib.vb2_last_error()


def test_rank_group_without_an_id_is_an_argument_error_before_any_device_work():
    """vb2_shard_group_create_rank(nranks > 1, id128 = NULL) used to build a group that returned
    PARTIAL sums without saying so; since ABI 5 it is VB2_ERR_INVALID (checked before the device is touched:
    testable here), and partial sums are an explicit request (VB2_SHARD_PARTIAL_SUMS)."""
    lib = _abi.lib()
    d = vb.synth.make_pileup(64, 10, 2, seed=3)
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.ShardGroup(d, device=0, rank=1, nranks=2, unique_id=None)
    assert ei.value.code == _abi.VB2_ERR_INVALID
    assert b"VB2_SHARD_PARTIAL_SUMS" in lib.vb2_last_error()
    # the stand-in for librccl is test infrastructure: it exports what shard.cpp binds, plus its marker
    import ctypes
    stub = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stub_rccl", "librccl_stub.so")
    L = ctypes.CDLL(stub)
    for sym in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommInitAll", "ncclCommDestroy", "ncclAllReduce",
                "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString", "vb2_rccl_stub_marker"):
        assert hasattr(L, sym), sym


def _oracle_evaluator(od):
    return lambda p1, p2, a: [od.llk(p1[i], p2[i], a[i]) for i in range(len(a))]


@pytest.mark.parametrize("pileup", ["expected/result.Pileup", "test.LongRead.pileup"])
@pytest.mark.parametrize("kw", [{}, {"within_ancestry": True}, {"fix_alpha": 0.1},
                                {"fix_pc": [0.034756, 0.0193]},
                                {"within_ancestry": True, "fix_pc": [0.034756, 0.0193]},
                                {"within_ancestry": True, "fix_alpha": 0.25}])
def test_cpp_optimiser_trace_equals_oracle(golden_dir, pileup, kw):
    flat, _, _ = refio.load_flat(os.path.join(golden_dir, HAPMAP), os.path.join(golden_dir, pileup), 2)
    od = binding.OracleData(flat)
    got = vb.optimize_with_evaluator(_oracle_evaluator(od), 2, trace_capacity=4096, **kw)
    want = od.optimize(trace_capacity=4096, **kw)
    assert got["num_eval"] == want["num_eval"] == got["trace_count"]
    assert got["num_launch_point"] >= got["num_eval"]          # speculation evaluates extra points
    for key in ("alpha", "pc1", "pc2", "llk"):
        assert np.array_equal(got["trace"][key], want["trace"][key]), key
    for key in ("alpha", "llk1", "llk0"):
        assert got[key] == want[key], key
    assert np.array_equal(got["pc"], want["pc"]) and np.array_equal(got["pc2"], want["pc2"])


@pytest.mark.parametrize("level", [1, 2, 4])
@pytest.mark.parametrize("kw", [{}, {"within_ancestry": True}, {"fix_alpha": 0.1},
                                {"within_ancestry": True, "fix_pc": [0.034756, 0.0193]}])
def test_speculation_level_does_not_change_the_trajectory(golden_dir, level, kw, tunable):
    """amoeba.h: 4 = {R, E, C_A, C_R} per iteration, 2 = {R, C_R}, 1 = one point at a time.  The
    committed evaluations (the trace) are the reference's in every case; only the number of points
    launched differs."""
    flat, _, _ = refio.load_flat(os.path.join(golden_dir, HAPMAP), os.path.join(golden_dir, "test.LongRead.pileup"), 2)
    od = binding.OracleData(flat)
    want = od.optimize(trace_capacity=4096, **kw)
    tunable("speculate", level)
    got = vb.optimize_with_evaluator(_oracle_evaluator(od), 2, trace_capacity=4096, **kw)
    assert got["num_eval"] == want["num_eval"]
    for key in ("alpha", "pc1", "pc2", "llk"):
        assert np.array_equal(got["trace"][key], want["trace"][key]), key
    assert got["alpha"] == want["alpha"] and got["llk1"] == want["llk1"]
    if level == 1:
        assert got["num_launch_point"] == got["num_eval"]
    elif level == 2:
        assert got["num_eval"] < got["num_launch_point"] <= 2 * got["num_eval"]
    else:
        assert got["num_launch_point"] > got["num_eval"]


def line_search_cases(golden_dir):
    """(function, lo, hi, tol): plain test functions that take every branch of the bracket, and the real objective (the
    LLK of the bundled input as a function of logit(alpha)).  The C library's functions (math), like the oracle's: the
    abscissae do not depend on which vector code numpy picks on a machine."""
    import math
    flat, _, _ = refio.load_flat(os.path.join(golden_dir, HAPMAP), os.path.join(golden_dir, "expected/result.Pileup"), 2)
    od = binding.OracleData(flat)
    pc = [0.01, 0.01]

    def neg_llk(x):
        return -od.llk(pc, pc, 1.0 / (1.0 + math.exp(-x)), num_thread=1)

    return [
        (lambda x: (x - 2.0) ** 2 + 1.0, 0.0, 1.0, 1e-8),                  # downhill to the right
        (lambda x: (x + 30.0) ** 2, 0.0, 1.0, 1e-10),                      # far: magnification limit
        (lambda x: abs(x - 0.3) ** 1.5 + 0.1 * x, 5.0, 4.0, 1e-9),         # swapped ends, non-smooth
        (lambda x: math.cosh(0.7 * x) + 0.05 * x ** 4 - x, -3.0, -2.9, 1e-12),
        (lambda x: -math.exp(-(x - 1.0) ** 2 / 50.0), -40.0, -39.0, 1e-8),  # nearly flat start
        (lambda x: float(math.floor(abs(x) * 3)), 2.2, 2.9, 1e-8),         # plateaus: the tie rules
        (neg_llk, math.log(0.03 / 0.97), math.log(0.03 / 0.97) + 1.0, 1e-8),
    ]


def test_line_search_equals_the_references_scalar_minimizer(golden_dir):
    """csrc/line_search.cpp (bracket + Brent; the optimiser of the one-parameter models, SURVEY.md
    8f row 4) against the reference's own ScalarMinimizer (MathGold.cpp:27-195): the same abscissae
    evaluated in the same order, the same result, bit for bit.  Against the reference's runs stored in
    golden/reference_runs.json (sha256 of the abscissae), and against oracle/_ref live where it is built."""
    import ctypes as C
    import hashlib
    import json
    L = _abi.lib()
    FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_double)
    CM = C.CFUNCTYPE(None, C.c_void_p, C.c_double, C.c_double)
    L.vb2_debug_line_search.restype = C.c_int
    L.vb2_debug_line_search.argtypes = [FN, CM, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int,
                                        C.POINTER(C.c_double)]
    digest = lambda xs: hashlib.sha256(np.array(xs, dtype=np.float64).tobytes()).hexdigest()   # noqa: E731
    cases = line_search_cases(golden_dir)
    stored = json.load(open(os.path.join(golden_dir, "reference_runs.json")))["line_search"]
    assert len(stored) == len(cases)
    for (fn, lo, hi, tol), rec in zip(cases, stored):
        refs = [(rec["num_eval"], rec["x_sha256"], {key: float.fromhex(v) for key, v in rec["want"].items()})]
        if binding.ref_lib() is not None:
            ref_x = []
            want = binding.reference_scalar_minimize(lambda x: (ref_x.append(x), fn(x))[1], lo, hi, tol)
            refs.append((len(ref_x), digest(ref_x), want))
        for speculate in (0, 1):
            got_x, launched = [], []
            out = (C.c_double * 5)()
            f_cb = FN(lambda _u, x: (launched.append(x), float(fn(x)))[1])
            c_cb = CM(lambda _u, x, y: got_x.append(x))
            rc = L.vb2_debug_line_search(f_cb, c_cb, None, lo, hi, tol, speculate, out)
            assert rc == 0
            for n, x_sha, want in refs:
                assert len(got_x) == n and digest(got_x) == x_sha, (speculate, len(got_x), n)
                assert dict(zip(("min", "fmin", "a", "b", "c"), list(out))) == want
                assert len(launched) == n + (1 if speculate else 0)   # the unused candidate for c


def _capture_stderr(fn):
    """fn() with file descriptor 2 redirected to a temporary file (C stdio of the libraries included)."""
    import ctypes
    import tempfile
    libc = ctypes.CDLL(None)
    with tempfile.TemporaryFile(mode="w+b") as tf:
        saved = os.dup(2)
        libc.fflush(None)
        os.dup2(tf.fileno(), 2)
        try:
            res = fn()
        finally:
            libc.fflush(None)
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        return res, tf.read().decode("latin-1")


@pytest.mark.parametrize("kw", [{}, {"within_ancestry": True}, {"fix_alpha": 0.1}])
def test_verbose_notices_are_the_references_per_evaluation_lines(golden_dir, kw):
    """--Verbose (VERDICT r3 missing #4): FullLLKFunc::Evaluate ends every call with
    notice("ContaminatingSamplePC1:%f\t...\tFREEMIX(Alpha):%f\tllk:%f") of the best-so-far state
    (ContaminationEstimator.h:435-440; notice() = "NOTICE - " + text + newline on stderr, statgen/Error.cpp:70-79).
    The library's estimator (here over the oracle as evaluator: no GPU) prints the same stream as the oracle's
    restatement of that statement, line for line: one line per evaluation of the searches, in the reference's format."""
    import re
    flat, _, _ = refio.load_flat(os.path.join(golden_dir, HAPMAP), os.path.join(golden_dir, "expected/result.Pileup"), 2)
    od = binding.OracleData(flat)
    want, err_o = _capture_stderr(lambda: od.optimize(verbose=True, **kw))
    got, err_p = _capture_stderr(lambda: vb.optimize_with_evaluator(_oracle_evaluator(od), 2, verbose=True, **kw))
    pat = re.compile(r"^NOTICE - ContaminatingSamplePC1:-?\d+\.\d{6}\tContaminatingSamplePC2:-?\d+\.\d{6}\t"
                     r"IntendedSamplePC1:-?\d+\.\d{6}\tIntendedSamplePC2:-?\d+\.\d{6}\tFREEMIX\(Alpha\):-?\d+\.\d{6}\tllk:-?\d+\.\d{6}$")
    lines_o = [ln for ln in err_o.split("\n") if ln.startswith("NOTICE - Contaminating")]
    lines_p = [ln for ln in err_p.split("\n") if ln.startswith("NOTICE - Contaminating")]
    assert lines_o and all(pat.match(ln) for ln in lines_o)
    assert lines_p == lines_o
    # one line per evaluation made THROUGH Evaluate: all but Initialize's and CalculateLLK0's two direct calls
    assert len(lines_p) == got["num_eval"] - 2 and got["num_eval"] == want["num_eval"]


LOCKSTEP_MODELS = [("heter", {}), ("homo", dict(within_ancestry=True)), ("heter-fixalpha", dict(fix_alpha=0.07)),
                   ("homo-fixalpha", dict(within_ancestry=True, fix_alpha=0.07)), ("heter-fixpc", dict(fix_pc=[0.01, -0.02])),
                   ("homo-fixpc", dict(within_ancestry=True, fix_pc=[0.01, -0.02]))]


@pytest.mark.parametrize("speculate", [4, 2])
@pytest.mark.parametrize("kw", [m for _, m in LOCKSTEP_MODELS], ids=[n for n, _ in LOCKSTEP_MODELS])
def test_lockstep_fibers_give_each_run_its_own_search(golden_dir, speculate, kw):
    """lockstep.h -- what cohorts and multi-start searches run on: several OptimizeLLK searches as
    fibers of one thread, every step's requests answered by ONE evaluator call.  Here without a
    device: the oracle evaluates, run 0 must equal the plain search (evaluation count, alpha, LLKs
    bit for bit), the jittered runs must equal themselves done alone, and the steps must indeed
    carry several runs' points each.  Under each of the six models: simplexes of 2k+1 = 5 (Heter), k+1 = 3 (Homo,
    HeterFixedPC), 2k = 4 and k = 2 (--FixAlpha) and ONE parameter (HomoFixedPC); run 0 is held to the oracle's own
    search under the same model, PCs included."""
    import ctypes as C
    flat, _, _ = refio.load_flat(os.path.join(golden_dir, HAPMAP), os.path.join(golden_dir, "expected/result.Pileup"), 2)
    od = binding.OracleData(flat)
    k, runs = 2, 5
    sizes = []

    def cb(_user, n, p1, p2, a, out):
        pc1 = np.ctypeslib.as_array(p1, (n, k)); pc2 = np.ctypeslib.as_array(p2, (n, k)); al = np.ctypeslib.as_array(a, (n,))
        sizes.append(n)
        for i in range(n):
            out[i] = od.llk(pc1[i], pc2[i], al[i], num_thread=1)
        return 0
    fn = _abi.EVAL_FN(cb)
    L = _abi.lib()
    L.vb2_debug_lockstep_optimize.restype = C.c_int
    L.vb2_debug_lockstep_optimize.argtypes = [_abi.EVAL_FN, C.c_void_p, C.c_int32, C.POINTER(_abi.Model), C.c_int32,
                                              C.c_int32, C.POINTER(_abi.Estimate), C.POINTER(C.c_int64)]
    m, _keep_fix_pc = vb.api._model(**kw)
    if not kw:
        m = _abi.Model(1, 0, 0, 0, 0.0, None, 1e-8, 0, 0)
    ests = (_abi.Estimate * runs)()
    steps = C.c_int64(0)
    assert L.vb2_debug_lockstep_optimize(fn, None, k, C.byref(m), runs, speculate, ests, C.byref(steps)) == 0
    together = list(sizes)
    assert steps.value == len(together) and max(together) > speculate        # steps carry several runs
    plain = od.optimize(**kw)
    assert ests[0].alpha == plain["alpha"] and ests[0].llk1 == plain["llk1"] and ests[0].llk0 == plain["llk0"]
    assert ests[0].num_eval == plain["num_eval"]
    assert all(e.converged for e in ests)
    assert np.array_equal(np.array(ests[0].pc[:k]), plain["pc"]) and np.array_equal(np.array(ests[0].pc2[:k]), plain["pc2"])
    # each run alone (a gang of i + 1 runs whose last member is run i) gives the same answer
    for i in (1, 4):
        alone = (_abi.Estimate * (i + 1))()
        assert L.vb2_debug_lockstep_optimize(fn, None, k, C.byref(m), i + 1, speculate, alone, None) == 0
        for key in ("alpha", "llk1", "llk0", "num_eval"):
            assert getattr(alone[i], key) == getattr(ests[i], key), (i, key)
    # the starts do differ (alpha is not searched under --FixAlpha: the likelihoods then)
    assert len({e.llk1 if "fix_alpha" in kw and "fix_pc" not in kw else e.alpha for e in ests}) > 1


def test_cpp_optimiser_other_dimensions():
    """k = 1 (the reference's hard-coded index-1 swap must not run) and k = 4."""
    for k, seed in ((1, 11), (4, 12)):
        d = vb.synth.make_pileup(300, 12, k, alpha_true=0.6 if k == 1 else 0.1, seed=seed)
        od = oracle_data(d)
        got = vb.optimize_with_evaluator(_oracle_evaluator(od), k, trace_capacity=20000)
        want = od.optimize(trace_capacity=20000)
        assert got["num_eval"] == want["num_eval"]
        assert np.array_equal(got["trace"]["llk"], want["trace"]["llk"])
        assert got["alpha"] == want["alpha"] and np.array_equal(got["pc"], want["pc"])


def test_evaluator_error_propagates():
    def bad(p1, p2, a):
        raise ValueError("boom")
    with pytest.raises(ValueError):
        vb.optimize_with_evaluator(bad, 2)


@pytest.mark.parametrize("pileup", ["expected/result.Pileup", "test.LongRead.pileup"])
def test_readers_match_reference_restatement(golden_dir, pileup):
    prefix = os.path.join(golden_dir, HAPMAP)
    d = vb.PileupData.from_files(prefix, os.path.join(golden_dir, pileup), 2, disable_sanity=True)
    flat, panel, viewer = refio.load_flat(prefix, os.path.join(golden_dir, pileup), 2)
    mine = flat_from_input(d)
    assert d.num_marker == flat.num_marker == 9787
    assert d.avg_depth == flat.avg_depth
    assert d.meta["num_bases"] == viewer.num_bases
    assert np.array_equal(mine.base_info_index >= 0, flat.base_info_index >= 0)
    assert np.array_equal(d.ud, flat.ud) and np.array_equal(d.means, flat.means)
    present = flat.base_info_index >= 0
    assert np.array_equal(d.alt_base[present], flat.alt_base[present])
    # same reads per marker, in the same order
    for i in np.nonzero(present)[0]:
        s = flat.base_info_index[i]
        a = flat.bases[flat.site_off[s]:flat.site_off[s + 1]]
        b = d.bases[d.read_off[i]:d.read_off[i + 1]]
        assert np.array_equal(a, b)
        a = flat.quals[flat.site_off[s]:flat.site_off[s + 1]]
        b = d.quals[d.read_off[i]:d.read_off[i + 1]]
        assert np.array_equal(a, b)


def test_reader_quirks(tmp_path):
    """First-char alleles, dropped unterminated last panel line, duplicate pileup line,
    indels / ^ / * / $ handling, sites outside the panel, sanity statistics."""
    pre = str(tmp_path / "p")
    with open(pre + ".bed", "w") as f:
        f.write("1\t99\t100\tA\tC,G\n1\t199\t200\tG\tT\n2\t9\t10\tC\tA\n2\t19\t20\tT\tG")   # no final \n
    with open(pre + ".UD", "w") as f:
        f.write("0.5 -0.25 9\n-1.5\t2.0\t9\n0.125 0.0 9\n")
    with open(pre + ".mu", "w") as f:
        f.write("1:100_A/C_rs1 0.4\n1:200_G/T_rs2 1.2\n2:10_C/A_rs3 0.9\n")
    with open(pre + ".pileup", "w") as f:
        f.write("1\t100\tA\t6\t.,c^].+2AGC$*\tIJK!LM\n"      # ^] skipped, +2AG skipped, * eats a qual
                "1\t150\tT\t2\t..\tII\n"                      # not in the panel
                "2\t10\tC\t3\taA-1gN\tABC\n"
                "1\t100\tA\t2\tcc\tII\n")                     # duplicate line: counted, not stored
    d = vb.PileupData.from_files(pre, pre + ".pileup", 2, disable_sanity=True)
    flat, panel, viewer = refio.load_flat(pre, pre + ".pileup", 2)
    assert d.num_marker == 3                                  # 4th bed line has no newline
    assert chr(d.alt_base[0]) == "C"                          # "C,G" -> 'C'
    got = [bytes(d.bases[d.read_off[i]:d.read_off[i + 1]]).decode() for i in range(3)]
    assert got == [".,c.C", "", "aAN"]
    quals = [bytes(d.quals[d.read_off[i]:d.read_off[i + 1]]).decode() for i in range(3)]
    assert quals == ["IJK!L", "", "ABC"]
    assert viewer.num_bases == d.meta["num_bases"] == 5 + 3 + 2
    assert d.avg_depth == flat.avg_depth == 10 / 3            # 3 counted lines (duplicate included)
    mine = flat_from_input(d)
    od_a, od_b = binding.OracleData(mine), binding.OracleData(flat)
    assert od_a.llk([0.1, 0.2], [0.0, 0.1], 0.07) == od_b.llk([0.1, 0.2], [0.0, 0.1], 0.07)

    # sanity statistics (IsSanityCheckOK) -- too few markers, so the check itself fails
    d2 = vb.PileupData.from_files(pre, pre + ".pileup", 2, disable_sanity=False)
    flat2, _, v2 = refio.load_flat(pre, pre + ".pileup", 2, sanity_disabled=False)
    assert d2.meta["sanity_ok"] is False
    assert d2.sd_depth == flat2.sd_depth and not d2.sanity_disabled


def _load_arrays(pre, k, **kw):
    d = vb.PileupData.from_files(pre, pre + ".pileup", k, **kw)
    return dict(M=d.num_marker, ud=d.ud.tobytes(), mu=d.means.tobytes(), off=d.read_off.tobytes(),
                bases=d.bases.tobytes(), quals=d.quals.tobytes(), alt=d.alt_base.tobytes(),
                avg=np.float64(d.avg_depth).tobytes(), sd=np.float64(d.sd_depth).tobytes(),
                nb=d.meta["num_bases"])


def test_fast_scanner_equals_stringstream_statements(tmp_path, tunable):
    """The readers parse plainly formatted lines with a hand-written scanner and everything else
    with the original `stringstream >> field` statements.  Differential test on deliberately
    odd files (CRLF, blank and short lines, signs, exponents, junk after numbers, hex, nan,
    huge values, multi-character alleles, tabs/spaces mixes): VB2_SLOW_PARSE=1 sends every
    line through the stringstream statements; the two must agree byte for byte."""
    rng = np.random.default_rng(77)
    nums = ["0.5", "-0.25", "+1.5", "1e-3", "2.5E+2", ".5", "5.", "1e5x", "0x10", "nan", "inf", "1e999",
            "1e-320", "-0", "12abc", "", "3,4", "1.2.3", "+", "-.e5", "00012.5000", "7e", "1e+", "９"]
    ints = ["100", "+200", "-5", "0300", "12x", "4294967296", "99999999999", "", "1.5", "0x1F", "7", "8"]
    alle = ["A", "C", "G", "T", "AC", "A,G", "a", "N", "", ".", "<DEL>"]
    seps = ["\t", " ", "  ", "\t ", " \t\t"]
    eols = ["\n", "\r\n", "\n", "\n"]

    def sep():
        return str(rng.choice(seps))

    for trial in range(int(os.environ.get("VB2_FUZZ_TRIALS", "25"))):
        pre = str(tmp_path / ("f%d" % trial))
        M = int(rng.integers(1, 40))
        odd = trial >= 5                       # the first files are clean apart from spacing/CRLF
        rows_bed, rows_ud, rows_mu, rows_pl = [], [], [], []
        for i in range(M):
            pos = 100 + 10 * i
            e = str(rng.choice(eols))
            pick = lambda pool, plain: str(rng.choice(pool)) if odd and rng.random() < 0.25 else plain
            rows_bed.append("1" + sep() + pick(ints, str(pos - 1)) + sep() + pick(ints, str(pos)) + sep() +
                            pick(alle, "A") + sep() + pick(alle, "C") + e)
            rows_ud.append(sep().join(pick(nums, "%r" % float(rng.normal())) for _ in range(3)) + e)
            rows_mu.append("m%d" % i + sep() + pick(nums, "%r" % float(rng.uniform(0.1, 1.9))) + e)
            depth = int(rng.integers(0, 8))
            seq = "".join(rng.choice(list(".,ACGTacgtN*$^+-1#"), size=depth)) if depth else "*"
            qual = "".join(chr(int(x)) for x in rng.integers(33, 100, size=max(depth, 1)))
            fields = ["1", pick(ints, str(pos)), "A", pick(ints, str(depth)), seq, qual]
            if odd and rng.random() < 0.15:
                fields = fields[:int(rng.integers(0, 6))]          # short / blank line
            rows_pl.append(sep().join(fields) + e)
        if odd and rng.random() < 0.5:
            rows_pl[-1] = rows_pl[-1].rstrip("\r\n")              # unterminated last pileup line counts
        if odd and rng.random() < 0.5:
            rows_bed[-1] = rows_bed[-1].rstrip("\r\n")            # ... but not the last panel line
        for ext, rows in ((".bed", rows_bed), (".UD", rows_ud), (".mu", rows_mu), (".pileup", rows_pl)):
            with open(pre + ext, "w", newline="") as f:
                f.write("".join(rows))
        out = []
        for slow in (0, 1):
            tunable("slow_parse", slow)
            try:
                out.append(_load_arrays(pre, 2, disable_sanity=True))
            except Exception as exc:             # both paths must fail alike, too
                out.append(("error", str(exc)))
        assert out[0] == out[1], trial


def test_avx2_pileup_scanner_equals_the_scalar_one(tmp_path, tunable):
    """read_pileup classifies the bases column 32 characters at a time (AVX2) and copies runs of kept
    characters with their qualities as blocks.  Differential test against the scalar scanner
    (tunable scalar_parse) and the stringstream statements (tunable slow_parse): long columns (runs that
    cross block boundaries), read-start / read-end marks, indels with one- and two-digit lengths, '*' / '#'
    placeholders, fewer qualities than bases, a last line without a newline, lines outside the panel."""
    rng = np.random.default_rng(4242)
    n_ok = 0
    for trial in range(int(os.environ.get("VB2_FUZZ_TRIALS", "24"))):
        pre = str(tmp_path / ("g%d" % trial))
        M = int(rng.integers(5, 60))
        with open(pre + ".bed", "w") as f:
            for i in range(M):
                f.write("1\t%d\t%d\tA\tC\n" % (99 + 10 * i, 100 + 10 * i))
        with open(pre + ".UD", "w") as f:
            for i in range(M):
                f.write("%r\t%r\n" % (float(rng.normal()), float(rng.normal())))
        with open(pre + ".mu", "w") as f:
            for i in range(M):
                f.write("m%d\t%r\n" % (i, float(rng.uniform(0.1, 1.9))))
        lines = []
        for i in range(M + 3):
            pos = 100 + 10 * i if i < M else 55 + i                 # the last three: not in the panel
            depth = int(rng.choice([0, 1, 7, 31, 32, 33, 63, 64, 65, 100, int(rng.integers(0, 130))]))
            seq, nread = [], 0
            while nread < depth:
                r = rng.random()
                if r < 0.80:
                    seq.append(str(rng.choice(list(".,ACGTNacgtn")))); nread += 1
                elif r < 0.84:
                    seq.append("^" + chr(int(rng.integers(33, 127))))
                elif r < 0.88:
                    seq.append("$")
                elif r < 0.92:
                    seq.append(str(rng.choice(["*", "#"]))); nread += 1
                else:
                    L = int(rng.choice([1, 2, 9, 10, 12]))
                    seq.append(str(rng.choice(["+", "-"])) + str(L) + "".join(rng.choice(list("ACGTNacgt"), size=L)))
            seq = "".join(seq) or "*"
            nq = max(1, nread - (int(rng.integers(0, 4)) if rng.random() < 0.2 else 0))
            qual = "".join(chr(int(x)) for x in rng.integers(33, 127, size=nq))
            lines.append("1\t%d\tA\t%d\t%s\t%s\n" % (pos, depth, seq, qual))
        # From the fourth trial on, lines the SIMD path must hand to the fallback statements are mixed in (ADVICE r3:
        # the bookkeeping of the base / quality pools across SIMD lines and fallback lines, and a duplicated
        # position recorded while the pools are inflated, were not pinned): CRLF ends, blanks instead of tabs,
        # a seventh field, short and empty lines, a position seen before.
        if trial >= 3:
            mixed = []
            for ln in lines:
                r = rng.random()
                body = ln.rstrip("\n")
                if r < 0.12:
                    mixed.append(body + "\r\n")
                elif r < 0.24:
                    mixed.append(body.replace("\t", " ") + "\n")
                elif r < 0.32:
                    mixed.append(body + "\textra\n")
                elif r < 0.38:
                    mixed.append("\t".join(body.split("\t")[:3]) + "\n")
                elif r < 0.42:
                    mixed.append("\n")
                    mixed.append(ln)
                elif r < 0.52 and mixed:
                    mixed.append(ln)
                    mixed.append(str(rng.choice(mixed[:-1])))           # a position seen before (SIMD or fallback form)
                else:
                    mixed.append(ln)
            lines = mixed
        if trial % 2:
            lines[-1] = lines[-1].rstrip("\n")
        with open(pre + ".pileup", "w", newline="") as f:
            f.write("".join(lines))
        out = []
        for var in (None, "scalar_parse", "slow_parse"):
            if var:
                tunable(var, 1)
            try:
                out.append(_load_arrays(pre, 2, disable_sanity=True))
            except Exception as exc:             # the three paths must fail alike, too
                out.append(("error", str(exc)))
            if var:
                tunable(var, 0)
        assert out[0] == out[1] == out[2], trial
        if trial < 3:
            assert out[0]["nb"] > 0
        n_ok += 0 if isinstance(out[0], tuple) else 1
    assert n_ok >= 8          # (mixed files are not all parse errors: the fallback transitions are exercised on successes)


def _flatten_digest(d):
    import ctypes
    L = _abi.lib()
    L.vb2_debug_flatten_digest.argtypes = [ctypes.POINTER(_abi.Input), ctypes.POINTER(ctypes.c_ulonglong)]
    L.vb2_debug_flatten_digest.restype = ctypes.c_int
    inp = d.as_input()
    out = ctypes.c_ulonglong(0)
    _abi.check(L.vb2_debug_flatten_digest(ctypes.byref(inp), ctypes.byref(out)), "vb2_debug_flatten_digest")
    return out.value


def test_flatten_is_the_same_bytes_whatever_the_thread_count():
    """The host half of vb2_ctx_create (classification, run-length coding, marker sort, per-marker constants) gives the same
    run words, tile records, constants and dictionary with one thread and with several (vb2_debug_flatten_digest: no device):
    the bench shape in small, a wide quality alphabet (codes beyond the first 64), deep and ragged markers (depth 0 .. 200),
    missing markers with the depth filter on, odd base characters, a known-AF input."""
    import json
    import subprocess
    import sys
    code = r"""
import sys, json
sys.path.insert(0, %r)
import numpy as np
import verifybamid_amd as vb
sys.path.insert(0, %r)
from test_abi_and_host import _flatten_digest
out = []
out.append(_flatten_digest(vb.synth.make_pileup(3000, 30, 4, seed=5)))
out.append(_flatten_digest(vb.synth.make_pileup(3000, 30, 2, seed=6, q_lo=2, q_hi=93)))
out.append(_flatten_digest(vb.synth.with_sanity_stats(vb.synth.make_pileup(2000, 33, 3, seed=7, missing_frac=0.2))))
out.append(_flatten_digest(vb.synth.make_pileup(1500, 64, 2, seed=8, q_lo=0, q_hi=60)))
rng = np.random.default_rng(9)
M = 600
depth = rng.choice([0, 1, 2, 31, 32, 33, 63, 64, 65, 100, 200], size=M)
off = np.zeros(M + 1, dtype=np.int64); np.cumsum(depth, out=off[1:])
R = int(off[-1])
bases = rng.choice(np.frombuffer(b".,ACGTacgtNn*", dtype=np.uint8), size=R)
quals = rng.integers(30, 130, size=R).astype(np.uint8)
alt = rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), size=M)
dd = vb.PileupData(2, rng.normal(size=(M, 2)), rng.uniform(0.1, 1.9, size=M), off, bases, quals, alt, None, 30.0, 0.0, True, {})
out.append(_flatten_digest(dd))
kaf = np.clip(rng.uniform(0, 1, size=M), 0.01, 0.99)
out.append(_flatten_digest(vb.PileupData(2, dd.ud, dd.means, off, bases, quals, alt, kaf, 30.0, 0.0, True, {})))
print(json.dumps(out))
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    # ... in the default layout, in the run-word layout (VB2_PD=0: its multi-threaded pack and schedule_tile pass) and in the
    # probability domain without the pair windows
    for layout in ({}, {"VB2_PD": "0"}, {"VB2_PD_PAIRS": "0"}):
        res = []
        for env_extra in ({"VB2_FLATTEN_THREADS": "1"}, {"VB2_FLATTEN_THREADS": "3"}, {"VB2_FLATTEN_THREADS": "8"}):
            p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **layout, **env_extra), capture_output=True,
                               text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            res.append(json.loads(p.stdout.strip().splitlines()[-1]))
        assert res[0] == res[1] == res[2], layout
        assert len(set(res[0])) == len(res[0]), layout     # (six different inputs, six different digests)


def test_run_scheduling_only_reorders_the_runs_of_a_marker():
    """Wide quality alphabets: a tile's runs are placed by schedule_tile (tile_sched.h) instead of in dictionary order.  The
    flatten's digest with the run words taken as a per-marker multiset (tunable digest_multiset) is the same with the
    scheduling on and off -- every run of every marker is still there, once, next to the same padding -- while the plain digest
    differs (the order did change); a narrow alphabet is left alone either way.  (Run-word layout only: VB2_PD=0 keeps the
    samples out of the probability-domain layout, which has one step order.)"""
    import json
    import subprocess
    import sys
    code = r"""
import sys, json
sys.path.insert(0, %r)
import numpy as np
import verifybamid_amd as vb
sys.path.insert(0, %r)
from test_abi_and_host import _flatten_digest
print(json.dumps([_flatten_digest(vb.synth.make_pileup(3000, 30, 2, seed=6, q_lo=2, q_hi=93)),
                  _flatten_digest(vb.synth.make_pileup(2000, 30, 4, seed=12, q_lo=2, q_hi=60)),
                  _flatten_digest(vb.synth.make_pileup(1500, 80, 2, seed=13, q_lo=5, q_hi=70)),
                  _flatten_digest(vb.synth.make_pileup(3000, 30, 4, seed=5))]))
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for sched in ("0", "1"):
        for mode in ("bytes", "multiset"):
            env = dict(os.environ, VB2_RUN_SCHED=sched, VB2_DIGEST_MULTISET="1" if mode == "multiset" else "0", VB2_PD="0")
            if sched == "1":
                del env["VB2_RUN_SCHED"]                   # (the default: scheduled above 48 codes)
            p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            res[sched, mode] = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["0", "multiset"] == res["1", "multiset"]
    for i in range(3):
        assert res["0", "bytes"][i] != res["1", "bytes"][i], i     # wide alphabets: the order changed
    assert res["0", "bytes"][3] == res["1", "bytes"][3]            # 42 codes: plain order either way


def _tiny_panel(pre):
    open(pre + ".bed", "w").write("1\t0\t1\tA\tC\n1\t9\t10\tG\tT\n")
    open(pre + ".UD", "w").write("0.5 0.25\n-0.5 0.125\n")
    open(pre + ".mu", "w").write("1:1_A/C 0.5\n1:10_G/T 1.0\n")


@pytest.mark.parametrize("seq", ["..+99999999999A", ".+A.", "-"])
def test_indel_marker_without_valid_length_is_an_error_not_a_crash(tmp_path, seq):
    """The reference's std::stoi throws on these (SimplePileupViewer.cpp:722) and the run dies;
    the library must report an error code -- with its helper threads joined, not std::terminate."""
    pre = str(tmp_path / "q")
    _tiny_panel(pre)
    open(pre + ".pileup", "w").write("1\t1\tA\t2\t%s\tII\n" % seq)
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.PileupData.from_files(pre, pre + ".pileup", 2, disable_sanity=True)
    assert "indel" in str(ei.value)
    # the process (and the library's error state) is still usable
    open(pre + ".pileup", "w").write("1\t1\tA\t2\t.+1AC\tII\n")
    d = vb.PileupData.from_files(pre, pre + ".pileup", 2, disable_sanity=True)
    assert bytes(d.bases).decode() == ".C"


def test_stale_fields_after_a_line_outside_the_panel_are_the_parsed_ones(tmp_path):
    """ReadPileup assigns the parsed strings back to seq/qual before the .bed lookup
    (SimplePileupViewer.cpp:785-786), so a following SHORT line inherits the parsed bases."""
    pre = str(tmp_path / "q")
    _tiny_panel(pre)
    # line 1 is outside the panel (fields persist, parsed: "." / "I"); line 2 has only chr pos
    open(pre + ".pileup", "w").write("1\t5\tA\t3\t.$*^]\tIJ\n1\t10\n")
    d = vb.PileupData.from_files(pre, pre + ".pileup", 2, disable_sanity=True)
    got = bytes(d.bases[d.read_off[1]:d.read_off[2]]).decode()
    assert got == "." and bytes(d.quals[d.read_off[1]:d.read_off[2]]).decode() == "I"


def test_gzipped_panel_files_are_inflated_like_the_reference_inputfile(tmp_path, golden_dir):
    """statgen's InputFile opens gzip'd .UD/.mu/.bed transparently (InputFile.cpp ifopen)."""
    import gzip
    import shutil
    pre = str(tmp_path / "gz")
    for ext in (".UD", ".mu", ".bed"):
        with open(os.path.join(golden_dir, HAPMAP + ext), "rb") as fi, gzip.open(pre + ext, "wb") as fo:
            shutil.copyfileobj(fi, fo)
    pile = os.path.join(golden_dir, "expected/result.Pileup")
    a = vb.PileupData.from_files(pre, pile, 2, disable_sanity=True)
    b = vb.PileupData.from_files(os.path.join(golden_dir, HAPMAP), pile, 2, disable_sanity=True)
    assert a.num_marker == b.num_marker == 9787
    assert a.ud.tobytes() == b.ud.tobytes() and a.means.tobytes() == b.means.tobytes()
    assert a.alt_base.tobytes() == b.alt_base.tobytes() and a.read_off.tobytes() == b.read_off.tobytes()


def test_big_ud_file_parsed_by_several_threads_equals_numpy(tmp_path):
    """A .UD of more than 1 MiB is cut at line ends and parsed by several threads (hostio.cpp:
    read_ud): same values, same order as a plain parse, 17-digit (strtod path) and short values
    mixed, and a bad row still reports the reference's message."""
    M, k = 40000, 4
    base = vb.synth.with_sanity_stats(vb.synth.make_pileup(M, 3, k, seed=12))
    pre = vb.synth.write_files(base, str(tmp_path / "panel"))
    assert os.path.getsize(pre + ".UD") > (1 << 20)
    d = vb.PileupData.from_files(pre, pre + ".pileup", k, disable_sanity=True)
    want = np.loadtxt(pre + ".UD")[:, :k]
    assert np.array_equal(d.ud, want)
    lines = open(pre + ".UD").read().splitlines()
    lines[31234] = lines[31234].split()[0]                     # one column where four are needed
    open(pre + ".UD", "w").write("\n".join(lines) + "\n")
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.PileupData.from_files(pre, pre + ".pileup", k, disable_sanity=True)
    assert "Expected:4 vs Observed:1" in str(ei.value)


def test_ud_with_too_few_columns(tmp_path):
    pre = str(tmp_path / "q")
    open(pre + ".bed", "w").write("1\t0\t1\tA\tC\n")
    open(pre + ".UD", "w").write("0.5\n")
    open(pre + ".mu", "w").write("1:1_A/C 0.5\n")
    open(pre + ".pileup", "w").write("1\t1\tA\t1\t.\tI\n")
    with pytest.raises(_abi.Vb2Error) as ei:
        vb.PileupData.from_files(pre, pre + ".pileup", 2)
    assert "NumPC" in str(ei.value)


def test_shard_range_is_the_read_balanced_partition():
    """vb2_shard_range: contiguous, complete, balanced on reads -- and well defined at the edges
    (more shards than markers, markers without reads)."""
    d = vb.synth.make_pileup(997, 17, 2, seed=8, missing_frac=0.3)
    for world in (1, 2, 5, 8, 64):
        cuts = [d.shard_range(r, world) for r in range(world)]
        assert cuts[0][0] == 0 and cuts[-1][1] == d.num_marker
        assert all(cuts[r][1] == cuts[r + 1][0] for r in range(world - 1))
        reads = [int(d.read_off[hi] - d.read_off[lo]) for lo, hi in cuts]
        assert sum(reads) == d.num_read
        assert max(reads) - min(reads) <= 2 * 40
    tiny = vb.synth.make_pileup(3, 10, 2, seed=9)
    cuts = [tiny.shard_range(r, 8) for r in range(8)]
    assert cuts[0][0] == 0 and cuts[-1][1] == 3 and all(lo <= hi for lo, hi in cuts)
    assert sum(hi - lo for lo, hi in cuts) == 3


def test_shard_partition_covers_all_reads():
    d = vb.synth.make_pileup(1000, 20, 3, seed=5, missing_frac=0.1)
    for world in (2, 3, 8):
        shards = [d.shard(r, world) for r in range(world)]
        assert sum(s.num_marker for s in shards) == d.num_marker
        assert sum(s.num_read for s in shards) == d.num_read
        reads = [s.num_read for s in shards]
        assert max(reads) - min(reads) <= 2 * 60              # balanced on reads
        cat = np.concatenate([s.bases for s in shards])
        assert np.array_equal(cat, d.bases)


def test_run_scheduling_leaves_almost_no_bank_conflicts(tmp_path):
    """tile_sched.h's claim, on a simulated sample (tools/ubench/sched_sim.cpp: the same header, host only): with 118 codes the
    16 table rows a step reads fall into distinct LDS bank groups in all but a fraction of a percent of the steps -- the padding
    row included -- where plain dictionary order needs 1.9 passes per step; 72 codes likewise."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sched_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "verifybamid_amd", "csrc"), "-o", exe,
                           os.path.join(root, "tools", "ubench", "sched_sim.cpp")])
    for q_lo, q_hi, plain_min in ((2, 60, 1.7), (10, 45, 1.25)):
        out = subprocess.run([exe, str(q_lo), str(q_hi), "20000"], capture_output=True, text=True, timeout=120).stdout
        m = re.search(r"plain ([0-9.]+), scheduled ([0-9.]+) \(ignoring the padding row: ([0-9.]+)\)", out)
        assert m, out
        plain, sched, nopad = (float(x) for x in m.groups())
        assert plain > plain_min and sched < 1.02 and nopad <= sched, out


def test_reads_without_their_arrays_are_an_argument_error_before_any_device_work():
    """vb2_ctx_create with read offsets that announce reads but no bases / quals / alt_base arrays: VB2_ERR_INVALID from the
    argument check (the device flatten uploads those arrays as they are; a NULL must not reach a memcpy)."""
    import ctypes
    lib = _abi.lib()
    d = vb.synth.make_pileup(64, 10, 2, seed=3)
    inp = d.as_input()
    for field in ("bases", "quals", "alt_base"):
        saved = getattr(inp, field)
        setattr(inp, field, None)
        h = ctypes.c_void_p()
        lib.vb2_ctx_create.restype = ctypes.c_int
        rc = lib.vb2_ctx_create(ctypes.byref(inp), None, ctypes.byref(h))
        assert rc == _abi.VB2_ERR_INVALID and not h.value, (field, rc)
        assert b"bases / quals / alt_base" in lib.vb2_last_error()
        setattr(inp, field, saved)
