"""The calibration of the paired interval on the numpy restatement (no GPU): tests/paired_ref.pair_case at 40 fixed seeds --
3 000 markers x 30, k = 2, alpha = 0.03 planted, the contaminant an outsider, the matched-normal rule at 0.99 -- once with
the tumour's allelic shift and once without.  Per seed and variant: the float64 refit through the host seam
(paired_ref.search), the profile interval by plain Newton climbs and bisection (paired_deriv_ref.interval_ref), and whether
it covers the planted alpha.

    python tools/paired_interval_calibration.py [OUT.json]      (default: profiles/paired_interval/calibration_restatement.json)

tests/test_paired_interval_gpu.py holds the device's intervals against this file, seed by seed.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEEDS = list(range(1, 41))
PLANTED = 0.03
HOM_MIN = 0.99


def case(seed, shifted):
    """(tumour, hypothesis [M, 6], pc2_fixed): what both the restatement and the device are given."""
    import paired_ref as pr
    _, shifted_t, plain_t, normal, _ = pr.pair_case(seed=seed, alpha=PLANTED)
    return (shifted_t if shifted else plain_t), pr.normal_rule(pr.normal_q(normal), HOM_MIN), np.zeros(2)


def one(job):
    import paired_deriv_ref as pdr
    import paired_ref as pr
    from deriv_ref import Counts
    seed, shifted = job
    tumour, hyp, pc2 = case(seed, shifted)
    c = Counts(tumour)
    (est,), _ = pr.search([c], [hyp], pc2[None])
    lo, hi = pdr.interval_ref(c, hyp, est, pc2, tol=1e-5)
    row = dict(seed=seed, shifted=shifted, status=int(est["status"]), alpha=float(est["alpha"]), lo=lo, hi=hi,
               covered=bool(lo <= PLANTED <= hi), markers=pr.given_count(c, hyp))
    print(row, flush=True)
    return row


def main():
    import multiprocessing
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paired_interval", "calibration_restatement.json")
    jobs = [(seed, shifted) for seed in SEEDS for shifted in (True, False)]
    with multiprocessing.Pool(max(1, min(8, len(os.sched_getaffinity(0))))) as pool:     # (a case takes about a minute)
        rows = pool.map(one, jobs, chunksize=1)
    summary = {("shifted" if s else "plain"): sum(r["covered"] for r in rows if r["shifted"] == s) for s in (True, False)}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(planted=PLANTED, hom_min=HOM_MIN, seeds=SEEDS, covered_of_40=summary, rows=rows), f, indent=1)
        f.write("\n")
    print("covered of %d: %r" % (len(SEEDS), summary))


if __name__ == "__main__":
    main()
