"""The split launches' item loop with its uniform address arithmetic on the scalar unit (eval_body, ADDR_SCALAR: the nine per-marker
constants through one buffer descriptor per column, the list words through a descriptor with the row in the scalar offset, the tile
record decoded and the queue drawn by scalar instructions) against code that change does not touch: launches of ONE point and plain
launches of eight points, which keep the 64-bit global addresses, the vector decode and the compiler's atomic.  No arithmetic on a
likelihood changes, a tile's product has its own slot and the slots are multiplied in the same order whatever the wave shape: every
point agrees bit for bit.  Which kernel ran is read from the library's count of split launches (vb2_debug_split_launches).

Shapes, all seeded synth.make_pileup, chosen for the addresses:
  * 800 markers at depth 30: the smallest sample that takes six ways (a grid of 12, a FULL last tile);
  * 801, 808, 809 markers: a partly filled last tile -- dead lanes, whose offset into a column is clamped to position 0;
  * --NumPC 2, 4 and 6 (KSEL 2, 4 and 0; with six components the columns 4 and 5 are loaded in the epilogue, the old way) and known
    allele frequencies (KSEL 0: no UD columns, the known-AF column the old way);
  * mean depth 0.5 (markers of one to four reads; a marker without a read is not active, so a tile without rows needs sixteen
    markers whose only reads are of a third base): tiles shorter than the three rows requested ahead, zero, odd and even counts of
    ref steps -- the three kinds of first row (the row that holds the last ref and the first alt step further down a list is
    the deep tiles' of every shape).  These
    markers follow 800 markers at depth 30 in ONE sample: the dictionary grows with the sample, and below 800 deep markers a
    workgroup's LDS holds the tables of all 48 points -- no launch is split (HISTORY.md, "The 400-marker case of the tests");
  * depth 200: long lists, the ring refilled many times from row offsets far from the tile's first row.
Launches of 48, 41, 40, 24 and 17 points each: six ways, six ways with a padded group, and fewer ways (WAYS)."""
import ctypes
import functools

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

pytestmark = pytest.mark.gpu

POINTS = 48
SIZES = (48, 41, 40, 24, 17)


def ways_counts():
    lib = _abi.lib()
    lib.vb2_debug_split_launches.argtypes = [ctypes.c_int]
    lib.vb2_debug_split_launches.restype = ctypes.c_longlong
    return {w: int(lib.vb2_debug_split_launches(w)) for w in (2, 3, 6)}


def ways_taken(before):
    now = ways_counts()
    return {w: now[w] - before[w] for w in now if now[w] != before[w]}


# name -> (markers, depth, --NumPC, known allele frequencies, every marker active); a depth below 1: that many markers at this depth
# behind 800 markers at depth 30 (a marker without a read is not active: about 80 and 95 of them are)
SHAPES = {
    "m800": (800, 30, 4, False, True),
    "m801": (801, 30, 4, False, True),
    "m808": (808, 30, 4, False, True),
    "m809": (809, 30, 4, False, True),
    "numpc2": (800, 30, 2, False, True),
    "numpc6": (809, 30, 6, False, True),
    "knownaf": (800, 30, 4, True, True),
    "knownaf809": (809, 30, 4, True, True),
    "depth05": (200, 0.5, 4, False, False),
    "depth05_numpc2": (209, 0.5, 2, False, False),
    "depth200": (800, 200, 4, False, True),
}
# points of a launch -> the ways the launch takes on these contexts of 50 to 56 tiles (a grid of 12; a workgroup's LDS holds two
# groups' tables: five groups go three ways, three groups in pairs)
WAYS = {48: 6, 41: 6, 40: 3, 24: 2, 17: 2}


@functools.lru_cache(maxsize=None)
def sample(name):
    """(pileup, points): made once per shape and shared, never written to"""
    M, depth, k, kaf, _ = SHAPES[name]
    d = vb.synth.make_pileup(M, depth, k, alpha_true=0.04, seed=1414, q_lo=20, q_hi=40)
    if depth < 1:
        a = vb.synth.make_pileup(800, 30, k, alpha_true=0.04, seed=1416, q_lo=20, q_hi=40)
        d = vb.PileupData(k, np.concatenate([a.ud, d.ud]), np.concatenate([a.means, d.means]),
                          np.concatenate([a.read_off, a.read_off[-1] + d.read_off[1:]]), np.concatenate([a.bases, d.bases]),
                          np.concatenate([a.quals, d.quals]), np.concatenate([a.alt_base, d.alt_base]), None, a.avg_depth, 0.0, True, {})
    if kaf:
        d = vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                          d.avg_depth, d.sd_depth, True, {})
    rng = np.random.default_rng(1415)
    pts = rng.normal(0, 0.03, (POINTS, k)), rng.normal(0, 0.03, (POINTS, k)), rng.uniform(0, 0.4, POINTS)
    for a in pts:
        a.setflags(write=False)
    return d, pts


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_split_launches_give_the_bits_of_single_point_and_plain_launches(name, tunable):
    d, (pc1, pc2, al) = sample(name)
    M, _, _, _, all_active = SHAPES[name]
    with vb.LikelihoodContext(d) as ctx:
        info = ctx.info()
        assert info["layout"] == 1, info
        if all_active:
            assert info["num_active_marker"] == M, info                           # (the last tile's live lanes are M % 16, as the shape says)
        tunable("split", 1)
        c = ways_counts()
        single = np.concatenate([ctx.llk(pc1[i:i + 1], pc2[i:i + 1], al[i:i + 1]) for i in range(POINTS)])
        plain = np.concatenate([ctx.llk(pc1[i:i + 8], pc2[i:i + 8], al[i:i + 8]) for i in range(0, POINTS, 8)])
        assert ways_taken(c) == {}                                                 # neither reference is a split launch
        assert np.all(np.isfinite(single)) and np.all(single < 0)
        for B in SIZES:
            c = ways_counts()
            got = ctx.llk(pc1[:B], pc2[:B], al[:B])
            took = ways_taken(c)
            print("%s (%d active markers), %d points: took %s; %d points differ from single-point launches, %d from plain launches of eight"
                  % (name, info["num_active_marker"], B, took, int(np.sum(bits(got) != bits(single[:B]))),
                     int(np.sum(bits(got) != bits(plain[:B])))))
            assert took == {WAYS[B]: 1}, (B, took)
            assert np.array_equal(bits(got), bits(single[:B])), B
            assert np.array_equal(bits(got), bits(plain[:B])), B
