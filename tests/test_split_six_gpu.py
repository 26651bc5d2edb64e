"""The split launch in sets of SIX workgroups (eval_body, SPLIT == kMaxGroups: a launch of six point groups on a grid that is a
multiple of six gives every workgroup ONE group over the tiles of six virtual blocks).  The work items, their slots, the order
in which the slots are multiplied and the word of the partial sums a virtual block's sum goes to are those of a three-way and of
a plain launch, so no bit may move: the default launch, `split` 3 (at most three ways, the behaviour before sets of six),
`split` 0 (passes) and plain launches of eight points agree byte for byte, and all of them with the oracle to LLK_RTOL.

Shapes: the smallest at which six ways can go wrong -- a grid of 12 (two sets of six, the last virtual blocks a tile pair short:
800 markers -- 400 markers, 13 tile pairs, have a grid of 7 and a dictionary of 49 rows, and their 48 points go up in one plain
launch: that sample is the case that must NOT take six ways), a grid of 24 with one virtual block a pair short, short and
empty lists (depth 3), the widest dictionary (qualities 2..60), and the three KSEL instantiations (--NumPC 4, 2, 3 and 4 with known allele frequencies).  Which ways a launch took is read from the
library's own count of split launches (vb2_debug_split_launches), never inferred."""
import ctypes
import functools

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from oracle.bridge import oracle_data

pytestmark = pytest.mark.gpu

LLK_RTOL = 1e-12          # (the bound of the existing launch tests: tests/test_split_launch_gpu.py)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def launches(ways):
    lib = _abi.lib()
    lib.vb2_debug_split_launches.argtypes = [ctypes.c_int]
    lib.vb2_debug_split_launches.restype = ctypes.c_longlong
    return int(lib.vb2_debug_split_launches(ways))


def ways_counts():
    return {w: launches(w) for w in (2, 3, 6)}


def ways_taken(before):
    """{ways: split launches since `before`}, the zero entries left out"""
    now = ways_counts()
    return {w: now[w] - before[w] for w in now if now[w] != before[w]}


# name -> (markers, depth, --NumPC, lowest and highest quality, known allele frequencies)
SHAPES = {
    "grid12": (800, 30, 4, 20, 40, False),       # 25 tile pairs, 156 rows: grid 13 -> 12; virtual block 0 owns three pairs, the others two
    "small": (400, 30, 4, 20, 40, False),        # 13 tile pairs, grid 7, a 49-row dictionary whose 48-point tables fit ONE workgroup: no split launch
    "grid24": (1500, 30, 4, 20, 40, False),
    "depth3": (1500, 3, 4, 20, 40, False),
    "wide": (1500, 30, 4, 2, 60, False),
    "numpc2": (1500, 30, 2, 20, 40, False),
    "numpc3": (1500, 30, 3, 20, 40, False),
    "knownaf": (1500, 30, 4, 20, 40, True),
}
POINTS = 48


@functools.lru_cache(maxsize=None)
def sample(name):
    """(pileup, points, the oracle's values of all 48 points): made once per shape and shared, never written to"""
    M, depth, k, q_lo, q_hi, kaf = SHAPES[name]
    d = vb.synth.make_pileup(M, depth, k, alpha_true=0.04, seed=612, q_lo=q_lo, q_hi=q_hi)
    if kaf:
        d = vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                          d.avg_depth, d.sd_depth, True, {})
    rng = np.random.default_rng(66)
    pc1, pc2, al = rng.normal(0, 0.03, (POINTS, k)), rng.normal(0, 0.03, (POINTS, k)), rng.uniform(0, 0.4, POINTS)
    od = oracle_data(d)
    want = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=1) for i in range(POINTS)])
    for a in (pc1, pc2, al, want):
        a.setflags(write=False)
    return d, (pc1, pc2, al), want


def four_ways(ctx, tunable, pc1, pc2, al, B):
    """the first B points as the default launch, with `split` 3, with `split` 0 and as plain launches of eight; and the ways the
    first two took"""
    p1, p2, a = pc1[:B], pc2[:B], al[:B]
    tunable("split", 1)
    c = ways_counts()
    default = ctx.llk(p1, p2, a)
    took_default = ways_taken(c)
    tunable("split", 3)
    c = ways_counts()
    three = ctx.llk(p1, p2, a)
    took_three = ways_taken(c)
    tunable("split", 0)
    c = ways_counts()
    passes = ctx.llk(p1, p2, a)
    assert ways_taken(c) == {}, B
    tunable("split", 1)
    plain = np.concatenate([ctx.llk(p1[i:i + 8], p2[i:i + 8], a[i:i + 8]) for i in range(0, B, 8)])
    return default, three, passes, plain, took_default, took_three


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "small"])
def test_six_ways_equal_three_ways_passes_and_plain_launches(name, tunable):
    d, (pc1, pc2, al), want = sample(name)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        for B in (48, 47, 41):
            default, three, passes, plain, took_default, took_three = four_ways(ctx, tunable, pc1, pc2, al, B)
            print("%s, %d points: default took %s, split 3 took %s, rel. error against the oracle %.3g"
                  % (name, B, took_default, took_three, rel_err(default, want[:B])))
            assert took_default == {6: 1}, (B, took_default)           # the launch under test really took six ways
            assert 6 not in took_three and sum(took_three.values()) == 1, (B, took_three)
            assert np.all(np.isfinite(default)) and np.all(default < 0), B
            assert np.array_equal(default, three), B
            assert np.array_equal(default, passes), B
            assert np.array_equal(default, plain), B
            assert rel_err(default, want[:B]) <= LLK_RTOL, B


@pytest.mark.parametrize("name", ["grid12", "grid24"])
def test_forty_points_do_not_take_six_ways(name, tunable):
    """five groups: sets of six would leave a workgroup without a group"""
    d, (pc1, pc2, al), want = sample(name)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        tunable("split", 1)
        c = ways_counts()
        assert np.array_equal(ctx.llk(pc1, pc2, al), ctx.llk(pc1, pc2, al))
        assert ways_taken(c) == {6: 2}                                # (this context does take six ways for 48 points)
        default, three, passes, plain, took_default, took_three = four_ways(ctx, tunable, pc1, pc2, al, 40)
        assert 6 not in took_default and sum(took_default.values()) == 1, took_default
        assert took_three == took_default
        assert np.array_equal(default, three) and np.array_equal(default, passes) and np.array_equal(default, plain)
        assert rel_err(default, want[:40]) <= LLK_RTOL


def test_a_grid_that_is_no_multiple_of_six_takes_no_six_ways(tunable):
    d, (pc1, pc2, al), want = sample("small")
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        for B in (48, 41):
            default, three, passes, plain, took_default, took_three = four_ways(ctx, tunable, pc1, pc2, al, B)
            assert 6 not in took_default and took_three == took_default, (took_default, took_three)
            assert np.array_equal(default, three) and np.array_equal(default, passes) and np.array_equal(default, plain)
            assert rel_err(default, want[:B]) <= LLK_RTOL


@pytest.mark.parametrize("name", ["grid12", "grid24"])
def test_both_entry_points_take_six_ways(name, tunable):
    """ctx.llk: the host waits on the flag behind the LAST share's results (the shares are counted at the seventh ticket word);
    ctx.llk_device: results in device memory, no flag"""
    import torch
    d, (pc1, pc2, al), want = sample(name)
    rows = np.concatenate([pc1, pc2, al[:, None]], axis=1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with vb.LikelihoodContext(d, device=0, stream=stream.cuda_stream) as ctx:
            assert ctx.info()["layout"] == 1
            tunable("split", 1)
            c = ways_counts()
            host = ctx.llk(pc1, pc2, al)
            assert ways_taken(c) == {6: 1}
            dev_rows = torch.tensor(rows, device="cuda")
            out = torch.full((POINTS,), float("nan"), dtype=torch.float64, device="cuda")
            stream.synchronize()
            c = ways_counts()
            ctx.llk_device(dev_rows.data_ptr(), out.data_ptr(), POINTS, stream.cuda_stream)
            stream.synchronize()
            assert ways_taken(c) == {6: 1}
            assert np.array_equal(out.cpu().numpy(), host)
            assert rel_err(host, want) <= LLK_RTOL


def test_launch_kinds_queued_back_to_back_leave_the_seven_ticket_words_at_zero(tunable):
    """One context, one stream, nothing synchronised in between: six ways, three ways, a 16-point launch (the tagged hand-off), a
    4-point launch, six ways again -- each with its own points and output.  Every result is the result of the same launch made
    alone: a ticket word that one kind left above zero would make the next launch's last arriver miss its turn."""
    import torch
    name = "grid24"
    d, (pc1, pc2, al), want = sample(name)
    k = SHAPES[name][2]
    rng = np.random.default_rng(6)
    sizes = (48, 48, 16, 4, 48)
    split_of = (1, 3, 1, 1, 1)
    rows = [np.concatenate([rng.normal(0, 0.03, (b, 2 * k)), rng.uniform(0, 0.4, (b, 1))], axis=1) for b in sizes]
    rows[0] = np.concatenate([pc1, pc2, al[:, None]], axis=1)      # (the first launch: the points the oracle has)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with vb.LikelihoodContext(d, device=0, stream=stream.cuda_stream) as ctx:
            assert ctx.info()["layout"] == 1
            dev = [torch.tensor(r, device="cuda") for r in rows]
            out = [torch.full((b,), float("nan"), dtype=torch.float64, device="cuda") for b in sizes]
            stream.synchronize()
            took = []
            for r, o, b, s in zip(dev, out, sizes, split_of):
                tunable("split", s)              # (read by the launcher on the host when the launch is queued)
                c = ways_counts()
                ctx.llk_device(r.data_ptr(), o.data_ptr(), b, stream.cuda_stream)
                took.append(ways_taken(c))
            stream.synchronize()
            assert took[0] == {6: 1} and took[4] == {6: 1} and took[2] == {} and took[3] == {}, took
            assert 6 not in took[1] and sum(took[1].values()) == 1, took
            got = [o.cpu().numpy() for o in out]
            for r, g, b, s in zip(rows, got, sizes, split_of):
                tunable("split", s)
                alone = ctx.llk(r[:, :k], r[:, k:2 * k], r[:, 2 * k])        # (a call that waits for its own result)
                assert np.array_equal(g, alone), (b, s)
    assert rel_err(got[0], want) <= LLK_RTOL
