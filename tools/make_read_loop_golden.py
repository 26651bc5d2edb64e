"""The golden values of tests/test_read_loop_gpu.py: the 48- and 41-point launches of its small, shallow samples as the PARENT
commit's library computes them on the GPU -- a change of the read loop's schedule must reproduce every byte.

    VB2_LIB_PATH=build_variants/parent/libvb2.so python tools/make_read_loop_golden.py OUTDIR PARENT_COMMIT_HASH

writes OUTDIR/llk.npy ([case][48 + 41] float64) and OUTDIR/meta.json (the parent's hash, the cases, a hash of each case's
input); copy both to tests/golden/read_loop/.  The cases and their points are defined HERE and imported by the test."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

MARKERS, SEED = 1500, 331
DEPTHS = (0.5, 3, 9, 30)
# (--NumPC, lowest and highest quality, known allele frequencies): KSEL 4, 2 and 0; 42 and 118 codes
CONFIGS = ((4, 20, 40, False), (2, 20, 40, False), (4, 20, 40, True), (4, 2, 60, False))
CASES = tuple((depth,) + cfg for depth in DEPTHS for cfg in CONFIGS)
SIZES = (48, 41)            # a full launch, and a last group that is not full


def make_case(case):
    import verifybamid_amd as vb
    depth, k, q_lo, q_hi, kaf = case
    d = vb.synth.make_pileup(MARKERS, depth, k, alpha_true=0.04, seed=SEED, q_lo=q_lo, q_hi=q_hi)
    if kaf:
        d = vb.PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, np.clip(d.means / 2, 0.01, 0.99),
                          d.avg_depth, d.sd_depth, True, {})
    return d


def points(case):
    k = case[1]
    rng = np.random.default_rng(318 + CASES.index(case))
    return rng.normal(0, 0.03, (48, k)), rng.normal(0, 0.03, (48, k)), rng.uniform(0, 0.4, 48)


def input_sha(d, pts):
    h = hashlib.sha256()
    for a in (d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base) + tuple(pts):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    import verifybamid_amd as vb
    out_dir, commit = sys.argv[1], sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    rows, shas = [], []
    for case in CASES:
        d, (pc1, pc2, al) = make_case(case), points(case)
        with vb.LikelihoodContext(d) as ctx:
            assert ctx.info()["layout"] == 1, case
            rows.append(np.concatenate([ctx.llk(pc1[:B], pc2[:B], al[:B]) for B in SIZES]))
        shas.append(input_sha(d, (pc1, pc2, al)))
    llk = np.array(rows, dtype=np.float64)
    assert np.all(np.isfinite(llk)) and np.all(llk < 0)
    np.save(os.path.join(out_dir, "llk.npy"), llk)
    meta = {"parent_commit": commit, "library": os.environ.get("VB2_LIB_PATH", "the tree's own"), "numpy": np.__version__,
            "cases": [list(c) for c in CASES], "sizes": list(SIZES), "input_sha256": shas,
            "llk_sha256": hashlib.sha256(llk.tobytes()).hexdigest()}
    json.dump(meta, open(os.path.join(out_dir, "meta.json"), "w"), indent=1)
    print("wrote %s: %d cases x %d values, parent %s" % (out_dir, llk.shape[0], llk.shape[1], commit))


if __name__ == "__main__":
    main()
