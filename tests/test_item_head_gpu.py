"""The head of a work item in the launches that pull several items per wave through the LDS queue (eval_body, AHEAD: a wave draws
its next item, requests that item's tile record and the first three rows of its list while its present item's epilogue runs, and
the next iteration starts from those registers).  What is carried across the loop's back edge must be the item's own: shapes
chosen for the carried state, not for size -- queues that are empty at a wave's first (early) draw, tiles shorter than the three
rows requested early, all three kinds of first row, waves with one, two and three to four items.  A tile's product keeps its own
slot, so the split launch, the pass-per-group launch and the plain 8-point launches must agree to the bit."""
import os

import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

pytestmark = pytest.mark.gpu

LLK_RTOL = 1e-12

# (markers, depth, --NumPC, known allele frequencies)
SHAPES = [(100, 30, 4, False),        # fewer items than waves: a wave's first draw, or its first early draw, finds the queue empty
          (1500, 0.5, 4, False),      # tiles of 0, 1, 2, 3 rows; all three kinds of first row; waves with exactly one item
          (1500, 3, 2, False),        # as above
          (12500, 30, 4, False),      # about two items per wave
          (30000, 30, 4, False),      # 60 items per workgroup, 3-4 per wave: the carried registers go round more than once
          (30000, 30, 3, False),      # KSEL 0
          (12500, 30, 4, True)]       # a known-AF context
SIZES = (17, 24, 25, 47, 48)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _known_af(d):
    return vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                         d.avg_depth, d.sd_depth, True, {})


@pytest.mark.parametrize("shape", SHAPES)
def test_items_drawn_and_requested_early_give_the_bits_of_every_other_launch(shape, tunable):
    M, depth, k, kaf = shape
    d = vb.synth.make_pileup(M, depth, k, alpha_true=0.04, seed=1010)
    if kaf:
        d = _known_af(d)
    rng = np.random.default_rng(1011)
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
    od = oracle_data(d)
    idx = [0, 7, 8, 40, B - 1]
    ref = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=os.cpu_count() or 1) for i in idx])
    err = rel_err(got[idx], ref)
    print("shape", shape, "rel err against the oracle", err)
    assert err <= LLK_RTOL
