"""--FindRelated on the clock: the marginal launch per sample with and without the related planes,
the related pair kernels and -- in the same run, on the same set -- the source pair kernels at 100 000 markers for 32, 256
and 1 024 samples (HIP events around the launches, after a warm-up, medians), and what the flag adds to the wall-clock of
a 32-sample cohort run from text files against the same run without it (alternating, three times each).  Writes JSON:

    python tools/related_time.py [--out profiles/related/related_time.json] [--markers 100000] [--cohort 32]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import verifybamid_amd as vb  # noqa: E402
from verifybamid_amd import _abi  # noqa: E402

# The issue-rate FLOOR of a pair and marker: four v_log_f32 (8 cycles per wave instruction, as section 11 counts them), the
# two dots' six FP32 multiply-adds and the three FMAs of the FS and D2 mixtures (4 cycles each) -- the work no formulation
# avoids.  What the kernel issues beyond that (four floors, the flag's multiplies, four conversions and FP64 adds) is what
# the measured time is compared against.
LOG_CYCLES, FMA_CYCLES = 8, 4
NUM_LOG, NUM_FMA = 4, 9
CLOCK_HZ, NUM_CU, SIMD_PER_CU, LANES = 2.4e9, 256, 4, 64
BOTH = vb.SourceSet.SOURCE | vb.SourceSet.RELATED


def issue_floor_ms(n, M):
    """ms of n^2 M pair-markers if only the four logarithms and the nine FMAs issued, every SIMD busy."""
    cycles_per_wave_marker = NUM_LOG * LOG_CYCLES + NUM_FMA * FMA_CYCLES
    waves = n * n * M / LANES
    return 1e3 * waves * cycles_per_wave_marker / (CLOCK_HZ * NUM_CU * SIMD_PER_CU)


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), max_ms=float(ms[-1]), reps=int(len(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--sizes", default="32,256,1024")
    ap.add_argument("--cohort", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    lib = _abi.lib()
    M, k = a.markers, 4
    out = dict(markers=M, assumptions=dict(log_cycles=LOG_CYCLES, fma_cycles=FMA_CYCLES, num_log=NUM_LOG, num_fma=NUM_FMA,
                                           clock_hz=CLOCK_HZ, num_cu=NUM_CU))

    # ---- the marginal launch, per sample (both layouts): source planes alone, related alone, both ----
    d = vb.synth.make_pileup(M, 30, k, 0.05, 2)
    out["marginals"] = {}
    for pd in (1, 0):
        _abi.set_tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx:
            layout = ctx.info()["layout"]
            entry = out["marginals"]["layout %d" % layout] = {}
            for name, planes in (("source", vb.SourceSet.SOURCE), ("related", vb.SourceSet.RELATED), ("both", BOTH)):
                with vb.SourceSet(M, 1, planes=planes) as s:
                    ms = (C.c_double * a.reps)()
                    _abi.check(lib.vb2_debug_source_time_marginals(s._h, ctx._h, C.c_double(0.03), 3, a.reps, ms),
                               "vb2_debug_source_time_marginals")
                    entry[name] = stats(list(ms))
                    print("marginal launch, layout %d, %d markers x 30, planes %-7s: %s" % (layout, M, name, entry[name]))
    _abi.set_tunable("pd", 1)

    # ---- the pair kernels: related and source on the same set ----
    out["pairs"] = {}
    for n in [int(x) for x in a.sizes.split(",")]:
        with vb.SourceSet(M, n, planes=BOTH) as s:
            reps = a.reps if n < 1024 else max(3, a.reps // 3)
            ms = (C.c_double * reps)()
            _abi.check(lib.vb2_debug_related_time_pairs(s._h, n, 7, 2, reps, ms), "vb2_debug_related_time_pairs")
            st = stats(list(ms))
            _abi.check(lib.vb2_debug_source_time_pairs(s._h, n, 7, 2, reps, ms), "vb2_debug_source_time_pairs")
            src = stats(list(ms))
            st["issue_floor_ms"] = issue_floor_ms(n, M)
            st["pair_markers_per_s"] = n * n * M / (1e-3 * st["median_ms"])
            st["source_pair_kernels"] = src
            st["relative_to_source"] = st["median_ms"] / src["median_ms"]
            st["set_bytes"] = n * M * 48
            out["pairs"][str(n)] = st
            print("related pair kernels, %4d samples x %d markers: median %.3f ms (issue floor %.3f ms), %.3g pair-markers/s; "
                  "source pair kernels %.3f ms: %.2f x" % (n, M, st["median_ms"], st["issue_floor_ms"], st["pair_markers_per_s"],
                                                           src["median_ms"], st["relative_to_source"]))

    # ---- a cohort run from text files with and without the flag ----
    if a.cohort > 0:
        S = a.cohort
        tmp = tempfile.mkdtemp()
        base = vb.synth.with_sanity_stats(vb.synth.make_pileup(M, 30, k, 0.05, 2))
        pre = vb.synth.write_files(base, os.path.join(tmp, "panel"))
        piles = []
        for s in range(S):
            dd = vb.synth.make_pileup(M, 30, k, alpha_true=0.01 * (1 + s % 20), seed=1000 + s)
            dd = vb.PileupData(k, base.ud, base.means, dd.read_off, dd.bases, dd.quals, base.alt_base, None, dd.avg_depth,
                               dd.sd_depth, True, dict(base.meta))
            piles.append(vb.synth.write_files(dd, os.path.join(tmp, "s%d" % s)) + ".pileup")
        outs = [os.path.join(tmp, "out%d" % s) for s in range(S)]
        vb.run_cohort_files(pre, piles[:16], outs[:16], num_pc=k)                       # warm-up: runtime, caches, page cache
        runs = dict(plain=[], find_related=[])
        for rep in range(3):
            for name in ("plain", "find_related"):
                t0 = time.perf_counter()
                if name == "plain":
                    res = vb.run_cohort_files(pre, piles, outs, num_pc=k)
                else:
                    res, _ = vb.run_cohort_files(pre, piles, outs, num_pc=k, find_related=True,
                                                 sources_prefix=os.path.join(tmp, "run"))
                runs[name].append(time.perf_counter() - t0)
                assert all(r["status"] == 0 for r in res)
        out["cohort"] = dict(samples=S, seconds=runs, median_plain_s=float(np.median(runs["plain"])),
                             median_find_related_s=float(np.median(runs["find_related"])))
        print("cohort of %d x %d markers: plain %s s, --FindRelated %s s" %
              (S, M, ["%.2f" % t for t in runs["plain"]], ["%.2f" % t for t in runs["find_related"]]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
