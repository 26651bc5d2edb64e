"""The units that read a context through csrc/marker_walk.h agree on a marker's L to the bit: the
source unit's log L (vb2_ctx_marginals), the weight term and the prior term of marker_sum_kernels.hip.

Both identities are exact because the three kernels build the same table values, take the same products over a marker's
steps or runs and sum L = sum W[g1][g2] G1[g1] G2[g2] in the same order: the source kernel's 2^900 start of the
probability-domain products is a power of two (no marker of these shapes comes near the exponent range), a weight row with
one non-zero entry adds +0.0 to the marker's w log L in every sum above it, and a weight of 1 multiplies log L by 1.0.
300 markers at depth 30 are 19 micro-tiles: two tile groups, the second partly filled.

What this does not check: the three kernels take the record decode and the pair numbering from the same header, so a fault
there moves all of them alike and passes here.  The decode is held to the oracle and the restatements by the suites of
each unit (test_derivs_gpu, test_source_gpu, test_replicates_gpu, test_conditioned_gpu).
"""
import numpy as np
import pytest

import verifybamid_amd as vb

pytestmark = pytest.mark.gpu

M, DEPTH = 300, 30
# (--NumPC, layout): the projection compiled for 2 and for 4 PCs and the general one (3 PCs; known AF), both layouts
CASES = [(2, 1), (2, 0), (3, 1), (4, 0)]


def _data(k, known_af=False):
    d = vb.synth.make_pileup(M, mean_depth=25 if known_af else DEPTH, num_pc=k, alpha_true=0.05, seed=40 + k)
    if known_af:
        d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, M), 0.0, 1.0)
    return d


def _points(k, n, seed):
    rng = np.random.default_rng(seed)
    alphas = [0.03, 0.0, 1e-6, 0.5, 1.0, 0.2, 0.07]
    return rng.normal(0, 0.02, (n, k)), rng.normal(0, 0.02, (n, k)), np.array([alphas[i % len(alphas)] for i in range(n)])


@pytest.mark.parametrize("k, pd", CASES)
def test_a_one_hot_weight_row_gives_w_times_the_source_kernels_log_l(k, pd, tunable):
    tunable("pd", pd)
    d = _data(k)
    pc1, pc2, alpha = _points(k, 1, seed=k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        log_l = ctx.marginals(pc1[0], pc2[0], alpha[0])[2]
        live = np.flatnonzero(log_l != 0.0)
        assert len(live) >= 256 + 24                         # counted markers in both tile groups
        pick = live[np.linspace(0, len(live) - 1, 24).astype(int)]
        assert len(set(pick.tolist())) == 24
        w = np.array([(1, 3, 255)[i % 3] for i in range(24)])
        weights = np.zeros((24, M), dtype=np.int64)
        weights[np.arange(24), pick] = w
        with vb.Replicates(ctx, weights) as rep:
            got = rep.eval([1] * 24, np.repeat(pc1, 24, axis=0), np.repeat(pc2, 24, axis=0), np.repeat(alpha, 24))
    want = w.astype(np.float64) * log_l[pick]
    print("k=%d layout=%d: %d of 24 values differ" % (k, pd, int(np.sum(got != want))))
    assert got.tobytes() == want.tobytes(), (got - want).tolist()


@pytest.mark.parametrize("k, pd, known_af", [c + (False,) for c in CASES] + [(2, 1, True)])
def test_all_ones_weights_and_an_all_zero_prior_give_the_same_bits(k, pd, known_af, tunable):
    tunable("pd", pd)
    d = _data(k, known_af)
    num_point = [8, 8, 8, 8, 8, 8, 1]                        # 49 points: one step, two launches (48 + 1)
    pc1, pc2, alpha = _points(k, 49, seed=10 + k)
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == pd
        with vb.Replicates(ctx, np.ones((7, M), dtype=np.int64)) as rep:
            weighted = rep.eval(num_point, pc1, pc2, alpha)
            assert (rep.info()["num_step"], rep.info()["num_launch"]) == (1, 2)
        with vb.Conditioned(ctx, np.zeros((7, M, 3), dtype=np.float32)) as cond:
            conditioned = cond.eval(num_point, pc1, pc2, alpha)
            assert (cond.info()["num_step"], cond.info()["num_launch"]) == (1, 2)
    print("k=%d layout=%d known_af=%d: %d of 49 values differ" % (k, pd, known_af, int(np.sum(weighted != conditioned))))
    assert np.all(weighted < 0.0)
    assert weighted.tobytes() == conditioned.tobytes(), (weighted - conditioned).tolist()
