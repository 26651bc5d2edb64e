"""The run-word kernels of the static deal in their general form (any --NumPC, or known allele frequencies: KSEL 0) at the
4-point and the narrower shapes -- llk_eval_kernel<3, 0, 0, false> and <4, 0, 0, false>, which hold the layout's sizes in scalar
registers of their own (eval_body: kOwnSizes): the same bits as the work queue's kernels give, and the oracle's values."""
import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

pytestmark = pytest.mark.gpu

LLK_RTOL = 1e-12


@pytest.mark.parametrize("shape", [(3000, 3, False), (2500, 4, True), (700, 5, False)], ids=lambda s: "M%d-k%d%s" % (s[0], s[1], "-knownAF" if s[2] else ""))
def test_static_deal_of_the_narrow_run_word_shapes_equals_the_queue_and_the_oracle(shape, tunable):
    M, k, kaf = shape
    d = vb.synth.make_pileup(M, 30, k, alpha_true=0.04, seed=97)
    if kaf:
        d = vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                          d.avg_depth, d.sd_depth, True, {})
    rng = np.random.default_rng(41)
    B = 8
    pc1, pc2, al = rng.normal(0, 0.03, (B, k)), rng.normal(0, 0.03, (B, k)), rng.uniform(0, 0.4, B)
    od = oracle_data(d)
    ref = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=1) for i in range(B)])
    tunable("pd", 0)

    def launches(ctx):
        assert ctx.info()["layout"] == 0
        four = np.concatenate([ctx.llk(pc1[i:i + 4], pc2[i:i + 4], al[i:i + 4]) for i in (0, 4)])
        two = np.concatenate([ctx.llk(pc1[i:i + 2], pc2[i:i + 2], al[i:i + 2]) for i in range(0, B, 2)])
        one = np.concatenate([ctx.llk(pc1[i:i + 1], pc2[i:i + 1], al[i:i + 1]) for i in range(B)])
        return four, two, one

    with vb.LikelihoodContext(d) as ctx:
        queue = launches(ctx)
    tunable("dyn_tiles", 0)
    with vb.LikelihoodContext(d) as ctx:
        static = launches(ctx)
    for q, s in zip(queue, static):
        assert np.array_equal(q, s)
        assert np.array_equal(s, static[0])
        err = float(np.max(np.abs(s - ref) / np.abs(ref)))
        print("max rel err against the oracle %.2e" % err)
        assert err <= LLK_RTOL
