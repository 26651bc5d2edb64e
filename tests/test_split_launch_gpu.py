"""The split launch (eval_body, SPLIT: sets of two or three workgroups share their tiles and split the point groups) where
tests/test_gpu_parity.py leaves off: every compile-time variant of the kernel, sparse samples, batch sizes around the point
where it takes over, many launches queued back to back on one stream between launches of other kinds, and parameters at the
edges of the double range inside one batch.  The split launch's tables are built from records and alphas that each thread
requests itself, and its sums are added up by one workgroup per share of the point groups, each behind a ticket of its own:
none of that may move a bit."""
import os

import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

pytestmark = pytest.mark.gpu

LLK_RTOL = 1e-12


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _known_af(d):
    return vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                         d.avg_depth, d.sd_depth, True, {})


# (markers, --NumPC, lowest and highest quality, known allele frequencies): 42 / 72 / 118 codes; KSEL 4, 2 and 0 (three
# PCs, and a known-AF context); 100 000 markers down to samples with fewer micro-tiles than the grid has virtual blocks
SHAPES = [(100000, 4, 20, 40, False), (100000, 4, 2, 60, False), (12500, 4, 20, 40, False), (3000, 2, 2, 93, False),
          (100000, 2, 10, 45, False), (30000, 2, 20, 40, False), (30000, 4, 10, 45, True), (30000, 2, 2, 60, True),
          (30000, 3, 20, 40, False), (1500, 4, 20, 40, False), (600, 2, 10, 45, False), (100, 4, 20, 40, False)]
# below, at and above the size where the split launch takes over (16 or 24 points, by the dictionary), last groups that are
# not full, four to six groups (sets of two and of three workgroups), and more than one call's 48
SIZES = (9, 16, 17, 23, 24, 25, 26, 31, 32, 33, 39, 40, 41, 47, 48, 49, 57, 73, 96, 97)


@pytest.mark.parametrize("shape", SHAPES)
def test_split_launch_equals_passes_and_plain_launches_for_every_kernel_variant(shape, tunable):
    M, k, q_lo, q_hi, kaf = shape
    d = vb.synth.make_pileup(M, 30, k, alpha_true=0.04, seed=331, q_lo=q_lo, q_hi=q_hi)
    if kaf:
        d = _known_af(d)
    rng = np.random.default_rng(318)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        for B in SIZES:
            pc1, pc2, al = rng.normal(0, 0.03, (B, k)), rng.normal(0, 0.03, (B, k)), rng.uniform(0, 0.4, B)
            tunable("split", 1)
            got = ctx.llk(pc1, pc2, al)
            assert np.all(np.isfinite(got)) and np.all(got < 0), B
            assert np.array_equal(got, ctx.llk(pc1, pc2, al)), B
            tunable("split", 0)
            assert np.array_equal(ctx.llk(pc1, pc2, al), got), B
            tunable("split", 1)
            plain = np.concatenate([ctx.llk(pc1[i:i + 8], pc2[i:i + 8], al[i:i + 8]) for i in range(0, B, 8)])
            assert np.array_equal(plain, got), B
    if M <= 30000:
        od = oracle_data(d)
        idx = [0, 7, 8, 40, B - 1]
        ref = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=os.cpu_count() or 1) for i in idx])
        assert rel_err(got[idx], ref) <= LLK_RTOL


@pytest.mark.parametrize("M", [100000, 12500])
def test_split_launches_queued_back_to_back_between_launches_of_other_kinds(M):
    """300 launches of 48 points through the device-pointer call on one stream, nothing synchronised in between, each with its
    own points and its own output row; every few of them a 4-point launch and a 16-point launch on the same context (the tagged
    hand-off: the same partial sums' buffer).  The arrival tickets must be back at zero and the partial sums reusable whenever
    the next launch starts: every row is the row its points give in a call that is synchronised on its own."""
    import torch
    k, N, B = 4, 300, 48
    d = vb.synth.make_pileup(M, 30, k, alpha_true=0.05, seed=2)
    rng = np.random.default_rng(300)
    stride = 2 * k + 1

    def points(n, b):
        p = np.concatenate([rng.normal(0, 0.03, (n, b, 2 * k)), rng.uniform(0, 0.5, (n, b, 1))], axis=2)
        assert p.shape == (n, b, stride)
        return p

    big, small, mid = points(N, B), points(N // 3 + 1, 4), points(N // 7 + 1, 16)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with vb.LikelihoodContext(d, device=0, stream=stream.cuda_stream) as ctx:
            assert ctx.info()["layout"] == 1
            dev = [torch.tensor(a, device="cuda") for a in (big, small, mid)]
            out = [torch.full(a.shape[:2], float("nan"), dtype=torch.float64, device="cuda") for a in (big, small, mid)]
            stream.synchronize()
            n4 = n16 = 0
            for i in range(N):
                ctx.llk_device(dev[0][i].data_ptr(), out[0][i].data_ptr(), B, stream.cuda_stream)
                if i % 3 == 1:
                    ctx.llk_device(dev[1][n4].data_ptr(), out[1][n4].data_ptr(), 4, stream.cuda_stream)
                    n4 += 1
                if i % 7 == 3:
                    ctx.llk_device(dev[2][n16].data_ptr(), out[2][n16].data_ptr(), 16, stream.cuda_stream)
                    n16 += 1
            stream.synchronize()
            got = [o.cpu().numpy() for o in out]
            assert n4 >= 90 and n16 >= 40
            for a, g, n in ((big, got[0], N), (small, got[1], n4), (mid, got[2], n16)):
                for i in range(n):
                    want = ctx.llk(a[i][:, :k], a[i][:, k:2 * k], a[i][:, 2 * k])        # (a call that waits for its own result)
                    assert np.array_equal(g[i], want), (a.shape[1], i)
    od = oracle_data(d)
    ref = np.array([od.llk(big[-1][j][:k], big[-1][j][k:2 * k], big[-1][j][2 * k], num_thread=os.cpu_count() or 1) for j in (0, 47)])
    assert rel_err(got[0][-1][[0, 47]], ref) <= LLK_RTOL


def test_alphas_at_the_edges_of_the_double_range_inside_one_split_launch(tunable):
    """alpha = 0, 1, the smallest double and NaN as members of ONE 48-point batch of a probability-domain context (qualities from 0:
    table entries exactly 0, subnormal, alpha * const), by the rule of tests/test_gpu_parity.py::
    test_parameters_at_the_edges_of_the_double_range_follow_the_reference: the oracle's value to LLK_RTOL where it is finite,
    and exactly 0 for a NaN alpha (every marker fails `markerLK > 0` and is left out).  The split launch's table is built from
    alphas that arrive in registers straight from global memory: the same values either way (tunable split)."""
    k = 2
    d = vb.synth.make_pileup(20000, 25, k, alpha_true=0.05, seed=77, q_lo=0, q_hi=45)
    od = oracle_data(d)
    rng = np.random.default_rng(5324)
    B = 48
    pc1, pc2, al = rng.normal(0, 0.03, (B, k)), rng.normal(0, 0.03, (B, k)), rng.uniform(0, 0.4, B)
    nan = float("nan")
    edge = {0: 0.0, 7: 1.0, 8: 5e-324, 15: nan, 16: 1.0, 23: 0.0, 24: nan, 31: 5e-324, 40: 1e-310, 46: 1.0 - 2.0 ** -53, 47: nan}
    for i, a in edge.items():
        al[i] = a
    want = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=os.cpu_count() or 1) for i in range(B)])
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        got = ctx.llk(pc1, pc2, al)
        tunable("split", 0)
        passes = ctx.llk(pc1, pc2, al)
        tunable("split", 1)
        plain = np.concatenate([ctx.llk(pc1[i:i + 8], pc2[i:i + 8], al[i:i + 8]) for i in range(0, B, 8)])
    isnan = np.isnan(al)
    print("edge alphas:", {i: (al[i], got[i], want[i]) for i in edge})
    assert np.all(want[isnan] == 0.0) and np.all(got[isnan] == 0.0)
    assert np.all(np.isfinite(want[~isnan]))
    assert rel_err(got[~isnan], want[~isnan]) <= LLK_RTOL
    assert np.array_equal(got, passes) and np.array_equal(got, plain)
