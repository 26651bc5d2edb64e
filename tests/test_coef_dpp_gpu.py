"""The six-way split launch with the projection's coefficients resident in the lanes of the DPP rows (eval_body, COEF_DPP:
llk_eval_split6_kernel<4> and <2> take a coefficient from lane j of the reader's 16-lane row -- v_fmac_f64_dpp under row_newbcast:j,
twice per FMA under complementary bank masks -- where the epilogue read it from LDS per item) against code that change does not
touch: launches of ONE point and plain launches of eight points, which read their coefficients from LDS.  Each FMA has the factors
and the addend it had, in the old order: every point agrees bit for bit.  The split launches go through the device entry
(vb2_llk_eval_batch_device), which hands out what the kernel computed; which kernel ran is read from the library's count of split
launches (vb2_debug_split_launches), so no case passes by not taking the path.

Samples, all seeded synth.make_pileup at depth 30 (a dictionary of 156 rows and a grid of 12: six ways):
  * 800 and 808 markers: a full last tile, and one whose live lanes are exactly the even 16-lane rows' (markers 0..7);
  * 801 and 809 markers: a partly filled last tile with ONE live lane, and with one odd-row lane besides -- the dead lanes are
    switched off in the branch on `live`, and a DPP read from a lane that is switched off leaves the reader with its old value: the
    projection stands in front of that branch, and these are the samples that say so;
  * --NumPC 4 and 2 (the two new paths, every sample), --NumPC 6 and known allele frequencies (KSEL 0: the old text, 800 and 809).
Launches of 48 points (six ways), 41 (six ways: the sixth group holds one valid point and seven copies of it, so the resident
registers of that workgroup hold the copies' coefficients) and 40 (three ways: the old path).
Points with ONE coordinate different from zero, each of the 2 k in every slot and at either of a lane's two points, at --NumPC 4: a
wrong lane index or the two register pairs swapped changes such a sum grossly, where a random point could hide it behind rounding.
A NaN alpha, a NaN coordinate and alpha = 0 through the same entry."""
import ctypes
import functools

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

pytestmark = pytest.mark.gpu

POINTS = 48
SIZES = (48, 41, 40)
# points of a launch -> the ways the launch takes on these contexts (a grid of 12; a workgroup's LDS holds two groups' tables: five
# groups go three ways)
WAYS = {48: 6, 41: 6, 40: 3}

# name -> (markers, --NumPC, known allele frequencies)
SHAPES = {
    "m800": (800, 4, False), "m801": (801, 4, False), "m808": (808, 4, False), "m809": (809, 4, False),
    "m800_numpc2": (800, 2, False), "m801_numpc2": (801, 2, False), "m808_numpc2": (808, 2, False), "m809_numpc2": (809, 2, False),
    "m800_numpc6": (800, 6, False), "m809_numpc6": (809, 6, False),
    "m800_knownaf": (800, 4, True), "m809_knownaf": (809, 4, True),
}


def ways_counts():
    lib = _abi.lib()
    lib.vb2_debug_split_launches.argtypes = [ctypes.c_int]
    lib.vb2_debug_split_launches.restype = ctypes.c_longlong
    return {w: int(lib.vb2_debug_split_launches(w)) for w in (2, 3, 6)}


def ways_taken(before):
    now = ways_counts()
    return {w: now[w] - before[w] for w in now if now[w] != before[w]}


@functools.lru_cache(maxsize=None)
def sample(name):
    """(pileup, parameter rows [48][2 k + 1]): made once per shape and shared, never written to"""
    M, k, kaf = SHAPES[name]
    d = vb.synth.make_pileup(M, 30, k, alpha_true=0.04, seed=1515, q_lo=20, q_hi=40)
    if kaf:
        d = vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                          d.avg_depth, d.sd_depth, True, {})
    rng = np.random.default_rng(1516)
    rows = np.concatenate([rng.normal(0, 0.03, (POINTS, k)), rng.normal(0, 0.03, (POINTS, k)), rng.uniform(0, 0.4, (POINTS, 1))], axis=1)
    rows.setflags(write=False)
    return d, rows


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class DeviceEntry:
    """A context on a stream of its own and launches through ctx.llk_device (vb2_llk_eval_batch_device)"""

    def __init__(self, d, tunable):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()
        self.d = d
        self.tunable = tunable

    def __enter__(self):
        self.guard = self.torch.cuda.stream(self.stream)
        self.guard.__enter__()
        self.ctx = vb.LikelihoodContext(self.d, device=0, stream=self.stream.cuda_stream)
        self.ctx.__enter__()
        self.tunable("split", 1)
        return self

    def __exit__(self, *exc):
        self.stream.synchronize()
        self.ctx.__exit__(*exc)
        self.guard.__exit__(*exc)

    def launches(self, rows, size):
        """the rows in launches of `size` points each (the last one shorter) -> (values, the split launches it took)"""
        torch = self.torch
        dev = torch.tensor(np.ascontiguousarray(rows), device="cuda")
        out = torch.full((len(rows),), 7.0, dtype=torch.float64, device="cuda")
        self.stream.synchronize()
        c = ways_counts()
        for i in range(0, len(rows), size):
            n = min(size, len(rows) - i)
            self.ctx.llk_device(dev[i:i + n].data_ptr(), out[i:i + n].data_ptr(), n, self.stream.cuda_stream)
        self.stream.synchronize()
        return out.cpu().numpy(), ways_taken(c)


def check_rows(name, rows, sizes, tunable, what):
    """launches of sizes[...] points of `rows` against launches of one point and plain launches of eight, bit for bit"""
    d, _ = sample(name)
    with DeviceEntry(d, tunable) as e:
        info = e.ctx.info()
        assert info["layout"] == 1 and info["num_active_marker"] == SHAPES[name][0], info      # (the last tile's live lanes are M % 16)
        single, took = e.launches(rows, 1)
        assert took == {}, took                                                    # neither reference is a split launch
        plain, took = e.launches(rows, 8)
        assert took == {}, took
        for B in sizes:
            got, took = e.launches(rows[:B], B)
            print("%s, %s, %d points: took %s; %d points differ from single-point launches, %d from plain launches of eight"
                  % (name, what, B, took, int(np.sum(bits(got) != bits(single[:B]))), int(np.sum(bits(got) != bits(plain[:B])))))
            assert took == {WAYS[B]: 1}, (B, took)
            assert np.array_equal(bits(got), bits(single[:B])), B
            assert np.array_equal(bits(got), bits(plain[:B])), B
    return single


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_split_launches_give_the_bits_of_single_point_and_plain_launches(name, tunable):
    _, rows = sample(name)
    single = check_rows(name, rows, SIZES, tunable, "random points")
    assert np.all(np.isfinite(single)) and np.all(single < 0)


@pytest.mark.parametrize("name", ["m800", "m809"])
def test_one_coordinate_at_a_time(name, tunable):
    """Point p of a launch sits at point p % 2 of slot (p % 8) / 2 of group p / 8.  Its one coordinate that is not zero is number
    (p % 8 + p / 8 + shift) % 8 of the 2 k = 8: over the six groups and the shifts 0 and 6 every (slot, point) position meets every
    coordinate, that is every accumulator every one of its FMAs alone -- its last one too -- from either register pair."""
    k = SHAPES[name][1]
    assert k == 4
    rng = np.random.default_rng(1517)
    seen = set()
    for shift in (0, 6):
        rows = np.zeros((POINTS, 2 * k + 1))
        for p in range(POINTS):
            c = (p % 8 + p // 8 + shift) % (2 * k)
            rows[p, c] = rng.choice([-1.0, 1.0]) * rng.uniform(0.02, 0.08)
            seen.add((p % 8, c))
        rows[:, -1] = rng.uniform(0.01, 0.4, POINTS)
        single = check_rows(name, rows, (48, 41), tunable, "one coordinate a point, shift %d" % shift)
        assert np.all(np.isfinite(single)) and np.all(single < 0)
        assert len(set(single.tolist())) == POINTS                                 # (no two points alike: a value taken from a neighbour shows)
    assert len(seen) == 8 * 2 * k


@pytest.mark.parametrize("name", ["m809", "m809_numpc2"])
def test_alpha_zero_and_nan_parameters(name, tunable):
    """the device entry hands out the kernel's own value (the host entry answers a NaN point with 0 by rule)"""
    _, rows0 = sample(name)
    rows = rows0.copy()
    rows[3, -1] = 0.0                    # alpha = 0
    rows[12, 1] = float("nan")           # a NaN coordinate of the first component: every allele frequency of the point
    rows[40, -1] = 0.0                   # (the last point of a 41-point launch: the one its padded group replicates)
    rows[9, -1] = float("nan")           # a NaN alpha: every table entry, so every marker's likelihood is NaN -- the factor 1
    single = check_rows(name, rows, SIZES, tunable, "alpha 0 and NaN")
    print("alpha 0 -> %r and %r, NaN coordinate -> %r, NaN alpha -> %r" % (single[3], single[40], single[12], single[9]))
    assert np.isfinite(single[3]) and single[3] < 0 and np.isfinite(single[40]) and single[40] < 0
    assert single[9] == 0.0              # (the reference's rule, context.h: no marker has a likelihood above 0 -- the sum over none)
