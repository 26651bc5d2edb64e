"""The epilogue of a work item in the 8-point probability-domain shape on the LDS queue (eval_body, EPI_X8): on the split
launch the tile butterfly's exchange over marker bit 3 goes through DPP moves and v_permlane16_swap instead of ds_bpermute.
(Two more parts were built with it and retired: the queue's draw riding the last row's table reads, and the projection
coefficients requested behind that row's multiplies; the shapes below still cover what they could get wrong.)
It may not move a bit: a tile's product keeps its own slot and its pairing order, so the split launch, the pass-per-group
launch, the plain 8-point launches and the narrower wave shapes -- whose exchange goes through __shfl and so pins the pairing
order of the new one -- must agree exactly.  Shapes chosen for what the epilogue and the item loop around it can get wrong,
not for size."""
import os

import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

pytestmark = pytest.mark.gpu

LLK_RTOL = 1e-12

# (markers, depth, --NumPC, known allele frequencies)
SHAPES = [(40, 30, 4, False),         # one partly filled pair of tiles: dead lanes carry the factor 1 through the exchange; the queue is empty at a wave's first draw
          (1500, 0.5, 4, False),      # tiles of 0, 1, 2 rows: the early draw's fallback, and a last row that is also the first
          (1500, 3, 2, False),        # KSEL 2: four coefficient quads
          (5000, 30, 4, False),       # several items per wave: the early draw's value crosses the back edge more than once; the draw past the queue's end
          (5000, 30, 3, False),       # KSEL 0: the general projection
          (5000, 30, 4, True)]        # a known-AF context: no coefficients at all
SIZES = (17, 25, 48)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _known_af(d):
    return vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                         d.avg_depth, d.sd_depth, True, {})


def _chunks(ctx, pc1, pc2, al, bounds):
    return np.concatenate([ctx.llk(pc1[a:b], pc2[a:b], al[a:b]) for a, b in bounds])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_epilogue_gives_the_bits_of_every_other_launch_and_wave_shape(shape, tunable):
    M, depth, k, kaf = shape
    d = vb.synth.make_pileup(M, depth, k, alpha_true=0.04, seed=1111)
    if kaf:
        d = _known_af(d)
    rng = np.random.default_rng(1112)
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
            plain = _chunks(ctx, pc1, pc2, al, [(i, min(i + 8, B)) for i in range(0, B, 8)])
            assert np.array_equal(plain, got), B
            # the 4-point shape (two tiles per wave) over all but the last one to four points, the 1-point shape over those
            n4 = (B - 1) // 4 * 4
            narrow = _chunks(ctx, pc1, pc2, al, [(i, i + 4) for i in range(0, n4, 4)] + [(i, i + 1) for i in range(n4, B)])
            assert np.array_equal(narrow, got), B
    od = oracle_data(d)
    idx = [0, 7, 8, 40, B - 1]
    ref = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=os.cpu_count() or 1) for i in idx])
    err = rel_err(got[idx], ref)
    print("shape", shape, "rel err against the oracle", err)
    assert err <= LLK_RTOL
