"""Weighted-marker replicates without a GPU: the additions to the ABI, the host-only helpers against restatements of
their definitions (the delete-m_j jackknife, the bootstrap generator, the chromosome blocks of the hapmap .bed), the lock-step
driver (vb2_replicates_lockstep) over the oracle on expanded inputs, the command line's refusals, and the new kernels'
resources from the code-object notes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replicate_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
HAPMAP = os.path.join(ROOT, "tests", "golden", "hapmap", "hapmap_3.3.b37.dat")
NEW_SYMBOLS = ["vb2_replicates_create", "vb2_replicates_destroy", "vb2_replicates_eval", "vb2_replicates_optimize_llk",
               "vb2_replicates_lockstep", "vb2_chromosome_weights", "vb2_bootstrap_weights", "vb2_jackknife",
               "vb2_run_replicates"]


def test_new_symbols_and_the_abi_is_still_7():
    lib = _abi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _abi.SYMBOLS
    assert lib.vb2_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "vb2_abi.h")).read()
    assert re.search(r"#define VB2_ABI_VERSION 7\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name


@pytest.mark.parametrize("m, tw", [
    ([100] * 6, [0.031, 0.029, 0.033, 0.030, 0.0305, 0.028]),                 # equal blocks
    ([870, 720, 610, 40, 330], [0.021, 0.035, 0.030, 0.0301, 0.027]),         # unequal blocks
    ([500, 0, 300, 200], [0.05, 0.9, 0.04, 0.06]),                            # a block without markers is skipped
    ([700, 300], [0.02, 0.04]),                                               # g = 2
])
def test_jackknife_agrees_with_the_formulas(m, tw):
    theta = 0.03
    est, se = vb.jackknife(m, theta, tw)
    want_est, want_se = replicate_ref.jackknife_numpy(m, theta, tw)
    assert abs(est - want_est) <= 1e-14 * max(1.0, abs(want_est)), (est, want_est)
    assert abs(se - want_se) <= 1e-12 * max(1e-3, want_se), (se, want_se)


def test_jackknife_of_equal_estimates_has_no_error_and_one_block_is_refused():
    est, se = vb.jackknife([400, 100, 250], 0.07, [0.07, 0.07, 0.07])
    assert se == 0.0 and est == 0.07
    # equal estimates that differ from the whole-sample one: tau_j - estimate = (h_j - g)(theta_hat - theta), 0 for equal blocks
    est, se = vb.jackknife([100, 100, 100, 100], 0.05, [0.07, 0.07, 0.07, 0.07])
    assert se == 0.0 and abs(est - (4 * 0.05 - 3 * 0.07)) <= 1e-16
    est, se = vb.jackknife([100] * 6, 0.05, [0.07] * 6)
    assert se <= 1e-16
    with pytest.raises(_abi.Vb2Error):
        vb.jackknife([400, 0], 0.07, [0.07, 0.07])


def test_bootstrap_weights_agree_with_the_generator():
    M, R, seed = 700, 3, 7
    w = vb.bootstrap_weights(M, R, seed)
    assert w.shape == (R, M) and w.dtype == np.uint8
    for r in range(R):
        want = np.bincount(replicate_ref.splitmix_draws(seed, r, M), minlength=M)
        assert want.max() < 255
        assert np.array_equal(w[r], want)
        assert int(w[r].sum()) == M
    assert w.tobytes() == vb.bootstrap_weights(M, R, seed).tobytes()
    assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[1], w[2])
    assert not np.array_equal(w, vb.bootstrap_weights(M, R, seed + 1))


def test_chromosome_weights_of_the_hapmap_bed(tmp_path):
    chrs, poss, _, _ = vb.synth.read_bed_rows(HAPMAP + ".bed")
    M = len(chrs)
    cw = vb.chromosome_weights(HAPMAP + ".bed")
    names = list(dict.fromkeys(chrs))
    assert cw["names"] == names and len(names) == 22
    distinct = {}
    for c, p in zip(chrs, poss):
        distinct.setdefault(c, set()).add(int(p))
    assert cw["block_size"].tolist() == [len(distinct[c]) for c in names]
    assert cw["only"].shape == (22, M) and cw["without"].shape == (22, M)
    assert np.all(cw["only"] + cw["without"] == 1)
    assert np.all(cw["only"].sum(axis=0) == 1)
    assert cw["block_of"].tolist() == [names.index(c) for c in chrs]
    # a position listed twice is one marker of its block
    rows = open(HAPMAP + ".bed").read().splitlines()[:50]
    twice = tmp_path / "twice.bed"
    twice.write_text("\n".join(rows + [rows[3]]) + "\n")
    cw2 = vb.chromosome_weights(str(twice))
    assert int(cw2["block_size"].sum()) == 50 and cw2["only"].shape[1] == 51
    assert np.all(cw2["only"] + cw2["without"] == 1)
    # fewer rows than markers: refused
    with pytest.raises(_abi.Vb2Error):
        vb.chromosome_weights(str(twice), num_marker=60)


@pytest.fixture(scope="module")
def lockstep_case():
    k, M = 2, 300
    d = vb.synth.make_pileup(M, mean_depth=20, num_pc=k, alpha_true=0.06, seed=11)
    rng = np.random.default_rng(5)
    half = np.zeros(M, dtype=np.int64)
    half[rng.permutation(M)[:M // 2]] = 1
    weights = np.stack([np.ones(M, dtype=np.int64), half, rng.integers(0, 4, M), np.zeros(M, dtype=np.int64)])
    return d, weights, replicate_ref.ExpandedOracle(d, weights)


@pytest.mark.parametrize("model", [dict(), dict(within_ancestry=True), dict(fix_pc=[0.01, -0.02])])
def test_lockstep_driver_returns_the_oracles_searches(lockstep_case, model):
    d, weights, ora = lockstep_case
    calls = []

    def evaluate(num_point, pc1, pc2, alpha):
        calls.append(tuple(int(x) for x in num_point))
        return ora.evaluate(num_point, pc1, pc2, alpha)

    got = vb.replicates_with_evaluator(evaluate, 4, d.num_pc, **model)
    assert got[3]["status"] == _abi.VB2_ERR_INVALID
    for r in range(3):
        want = ora.data(r).optimize(**model)
        assert got[r]["status"] == 0
        assert got[r]["alpha"] == want["alpha"], (r, got[r]["alpha"], want["alpha"])
        assert got[r]["llk1"] == want["llk1"]
        assert got[r]["num_eval"] == want["num_eval"]
        assert np.array_equal(got[r]["pc"], want["pc"]) and np.array_equal(got[r]["pc2"], want["pc2"])
    # one call per step, every live replicate in it; the empty replicate leaves after its first evaluation
    assert all(len(c) == 4 and max(c) <= _abi.VB2_BATCH_SLOTS for c in calls)
    assert calls[0][3] > 0 and all(c[3] == 0 for c in calls[1:])
    assert any(sum(1 for n in c if n > 0) >= 3 for c in calls)


def test_an_evaluator_error_ends_every_search(lockstep_case):
    d, weights, ora = lockstep_case
    seen = []

    def evaluate(num_point, pc1, pc2, alpha):
        seen.append(1)
        if len(seen) == 3:
            raise RuntimeError("evaluator gave up")
        return ora.evaluate(num_point, pc1, pc2, alpha)

    with pytest.raises(RuntimeError, match="evaluator gave up"):
        vb.replicates_with_evaluator(evaluate, 4, d.num_pc)


@pytest.mark.parametrize("flags, message", [
    (["--PerChromosome", "--PileupList", "list.txt"], "--PerChromosome cannot be combined with --PileupList"),
    (["--Bootstrap", "8", "--PileupList", "list.txt"], "--Bootstrap cannot be combined with --PileupList"),
    (["--PerChromosome", "--Devices", "0,1"], "--PerChromosome cannot be combined with more than one --Devices"),
    (["--Bootstrap", "8", "--Devices", "0,1"], "--Bootstrap cannot be combined with more than one --Devices"),
    (["--Bootstrap", "0"], "--Bootstrap takes 1 to 1000 replicates"),
    (["--Bootstrap", "1001"], "--Bootstrap takes 1 to 1000 replicates"),
])
def test_command_line_refusals(flags, message):
    p = subprocess.run([EXE, "--SVDPrefix", HAPMAP, "--Reference", "NA", "--PileupFile", "none.pileup"] + flags,
                       capture_output=True, text=True)
    assert p.returncode != 0
    assert message in p.stderr, p.stderr
    assert p.stdout == ""


def test_the_planted_chromosome_stands_out_for_the_oracle():
    """The sample of the GPU suite's planted-region test, on the CPU: the oracle on the chromosome-2 subset and on its
    complement (expanded inputs) brackets the genome-wide estimate as the .Chrom assertions need it to."""
    import test_replicates_gpu as gpu_tests
    from oracle.bridge import oracle_data
    d, chrs = gpu_tests.planted_data(gpu_tests.PLANTED_SEED)
    on_two = np.array([c == gpu_tests.PLANTED_CHR for c in chrs]).astype(np.int64)
    assert on_two.sum() == 870 and d.num_marker == 9787 and len(set(chrs)) == 22
    whole = oracle_data(d).optimize()["alpha"]
    only = oracle_data(replicate_ref.expand(d, on_two)).optimize()["alpha"]
    without = oracle_data(replicate_ref.expand(d, 1 - on_two)).optimize()["alpha"]
    print("oracle: whole %.6f, chromosome 2 only %.6f, without it %.6f" % (whole, only, without))
    assert abs(only - gpu_tests.PLANTED_ALPHA) < 0.03 and abs(without - gpu_tests.BASE_ALPHA) < 0.005
    assert without < whole - 0.005 < only


def test_weighted_kernels_use_no_scratch():
    """Note-only, like tests/test_kernel_resources_cpu.py: the six weight-term instantiations of llk_sum_marker_kernel
    (marker_sum_kernels.hip), the reduction and the permutation of libvb2.so live in one code object, use no scratch memory
    and fit 128 VGPRs."""
    import test_kernel_resources_cpu as res
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = res.all_kernel_notes(res.LIB)
    mine = {k: v for k, v in notes.items()
            if re.search(r"llk_sum_marker_kernel<[^>]*WeightTerm|llk_sum_reduce_kernel|weights_permute_kernel", k[1])}
    short = lambda name: re.search(r"(\w+_kernel(<[^>]*>)?)\(", name).group(1)
    for k, v in sorted(mine.items()):
        print("%4d VGPRs %5d B scratch  %s  [%s]" % (v["vgpr_count"], v["private_segment_fixed_size"], short(k[1]), k[0]))
    marker = {short(k[1]) for k in mine if "llk_sum_marker_kernel<" in k[1]}
    assert len(marker) == 6, marker                      # PD x KSEL 0, 2, 4
    assert len(mine) == 8 and len({k[0] for k in mine}) == 1, sorted(mine)
    over = {short(k[1]): v for k, v in mine.items() if v["private_segment_fixed_size"] != 0 or v["vgpr_count"] > 128}
    assert not over, over
