"""The split launches' tile butterfly as a reduce-scatter (eval_body, EPI_SCATTER: behind the exchange over marker bit 3 the even
16-lane rows go on with point 0 of a lane's two points and the odd rows with point 1 of the lane sixteen below; the lanes of
marker 0 and the lanes sixteen above them store) against code that change does not touch: launches of ONE point (MODE 4: one
point per lane -- no second point to scatter, the exchange over marker bit 3 a __shfl) and plain launches of eight points (the
old butterfly, ds_bpermute).  A tile's product has its own slot and the slots are multiplied in the same order whatever the
wave shape, so every point agrees bit for bit.  Which kernel ran is read from the library's count of split launches
(vb2_debug_split_launches), never inferred.

Shapes, all seeded synth.make_pileup: 800 markers at depth 30 (the six-way case of tests/test_split_six_gpu.py: a grid of 12, a
FULL last tile) and 801 / 808 / 809 markers -- the last tile then has live lanes in one even-row lane (marker 0), in exactly the
even rows (markers 0..7), and in one odd-row lane besides (marker 8); 41 points (a group padded with replicas of the last
point), 40, 24 and 17 points (fewer ways: WAYS below says which each takes here); --NumPC 2 and known allele frequencies (the
KSEL 2 and 0 instantiations); depth 200 (a tile's exponent sum in the thousands, negative: a dropped or doubled exponent dword
cannot hide); and points with alpha = 0, a NaN coordinate and a NaN alpha, through the device entry, which hands out what the
kernel computed (the select `lk > 0 ? lk : 1.0` now sits in the branch of the tiny values)."""
import ctypes
import functools

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

pytestmark = pytest.mark.gpu

POINTS = 48


def ways_counts():
    lib = _abi.lib()
    lib.vb2_debug_split_launches.argtypes = [ctypes.c_int]
    lib.vb2_debug_split_launches.restype = ctypes.c_longlong
    return {w: int(lib.vb2_debug_split_launches(w)) for w in (2, 3, 6)}


def ways_taken(before):
    now = ways_counts()
    return {w: now[w] - before[w] for w in now if now[w] != before[w]}


# name -> (markers, depth, --NumPC, known allele frequencies)
SHAPES = {
    "m800": (800, 30, 4, False),
    "m801": (801, 30, 4, False),
    "m808": (808, 30, 4, False),
    "m809": (809, 30, 4, False),
    "numpc2": (800, 30, 2, False),
    "knownaf": (800, 30, 4, True),
    "depth200": (800, 200, 4, False),
}
# points of a launch -> the ways the launch takes on these contexts (a grid of 12; a workgroup's LDS holds two groups' tables: five
# groups go three ways, three groups in pairs -- two groups and one)
WAYS = {48: 6, 41: 6, 40: 3, 24: 2, 17: 2}


@functools.lru_cache(maxsize=None)
def sample(name):
    """(pileup, points): made once per shape and shared, never written to"""
    M, depth, k, kaf = SHAPES[name]
    d = vb.synth.make_pileup(M, depth, k, alpha_true=0.04, seed=613, q_lo=20, q_hi=40)
    if kaf:
        d = vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                          d.avg_depth, d.sd_depth, True, {})
    rng = np.random.default_rng(67)
    pts = rng.normal(0, 0.03, (POINTS, k)), rng.normal(0, 0.03, (POINTS, k)), rng.uniform(0, 0.4, POINTS)
    for a in pts:
        a.setflags(write=False)
    return d, pts


def one_by_one(ctx, p1, p2, a):
    return np.concatenate([ctx.llk(p1[i:i + 1], p2[i:i + 1], a[i:i + 1]) for i in range(len(a))])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_shape(name, sizes, tunable):
    d, (pc1, pc2, al) = sample(name)
    M = SHAPES[name][0]
    with vb.LikelihoodContext(d) as ctx:
        info = ctx.info()
        assert info["layout"] == 1 and info["num_active_marker"] == M, info       # (the last tile's live lanes are M % 16, as the shape says)
        tunable("split", 1)
        c = ways_counts()
        single = one_by_one(ctx, pc1, pc2, al)
        plain = np.concatenate([ctx.llk(pc1[i:i + 8], pc2[i:i + 8], al[i:i + 8]) for i in range(0, POINTS, 8)])
        assert ways_taken(c) == {}                                                 # neither reference is a split launch
        assert np.all(np.isfinite(single)) and np.all(single < 0)
        for B in sizes:
            c = ways_counts()
            got = ctx.llk(pc1[:B], pc2[:B], al[:B])
            took = ways_taken(c)
            print("%s, %d points: took %s; %d points differ from single-point launches, %d from plain launches of eight"
                  % (name, B, took, int(np.sum(bits(got) != bits(single[:B]))), int(np.sum(bits(got) != bits(plain[:B])))))
            assert took == {WAYS[B]: 1}, (B, took)
            assert np.array_equal(bits(got), bits(single[:B])), B
            assert np.array_equal(bits(got), bits(plain[:B])), B
    return single


def test_full_last_tile_and_fewer_points(tunable):
    check_shape("m800", (48, 41, 40, 24, 17), tunable)


@pytest.mark.parametrize("name", ["m801", "m808", "m809"])
def test_partly_filled_last_tile(name, tunable):
    check_shape(name, (48, 41), tunable)


@pytest.mark.parametrize("name", ["numpc2", "knownaf"])
def test_other_kernel_selections(name, tunable):
    check_shape(name, (48, 40, 17), tunable)


def test_exponent_sums_in_the_thousands(tunable):
    """depth 200: the LLK of a point over the 50 tiles is 50 x (a tile's mean exponent sum) x ln 2 -- the sums are below -1000"""
    single = check_shape("depth200", (48, 17), tunable)
    print("mean exponent sum of a tile: %.0f .. %.0f" % (single.min() / 50 / np.log(2.0), single.max() / 50 / np.log(2.0)))
    assert single.max() < -1000.0 * 50 * np.log(2.0), single.max()      # (this input does what the case is for)


def test_alpha_zero_and_nan_parameters_through_the_device_entry(tunable):
    """ctx.llk_device hands out the kernel's own value (the host entry answers a NaN point with 0 by rule); the points' values
    from launches of 48, 41 and 17 points and from launches of one"""
    import torch
    d, (pc1, pc2, al) = sample("m809")
    rows = np.concatenate([pc1, pc2, al[:, None]], axis=1)
    rows[3, -1] = 0.0                    # alpha = 0
    rows[12, 1] = float("nan")           # a NaN coordinate of the first component: every allele frequency of the point
    rows[16, -1] = 0.0                   # (the last point of a 17-point launch: the one its padded group replicates)
    rows[9, -1] = float("nan")           # a NaN alpha: every table entry, so every marker's likelihood is NaN -- the factor 1
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with vb.LikelihoodContext(d, device=0, stream=stream.cuda_stream) as ctx:
            assert ctx.info()["layout"] == 1
            tunable("split", 1)
            dev = torch.tensor(rows, device="cuda")
            single = torch.full((POINTS,), 7.0, dtype=torch.float64, device="cuda")
            stream.synchronize()
            c = ways_counts()
            for i in range(POINTS):
                ctx.llk_device(dev[i:i + 1].data_ptr(), single[i:i + 1].data_ptr(), 1, stream.cuda_stream)
            stream.synchronize()
            assert ways_taken(c) == {}
            want = single.cpu().numpy()
            for B in (48, 41, 17):
                out = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
                stream.synchronize()
                c = ways_counts()
                ctx.llk_device(dev.data_ptr(), out.data_ptr(), B, stream.cuda_stream)
                stream.synchronize()
                got = out.cpu().numpy()
                print("%d points: took %s; alpha 0 -> %r, NaN coordinate -> %r, NaN alpha -> %r (single-point launches: %r, %r, %r)"
                      % (B, ways_taken(c), got[3], got[12], got[9], want[3], want[12], want[9]))
                assert ways_taken(c) == {WAYS[B]: 1}, B
                assert np.array_equal(bits(got), bits(want[:B])), B
            assert np.isfinite(want[3]) and want[3] < 0
            assert want[9] == 0.0            # (the reference's rule, context.h: no marker has a likelihood above 0 -- the sum over none)
