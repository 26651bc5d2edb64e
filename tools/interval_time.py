"""What the intervals of a cohort cost on one MI355X, S = 32 samples, at 3 000 x 30 (k = 2) and 100 000 x 30 (k = 4):
  (a) vb2_ctx_interval called sample after sample on S contexts -- all a cohort could do before vb2_batch_interval;
  (b) vb2_batch_interval on the same contexts and estimates (the intervals advancing in lock-step);
  (c) a cohort run from files (vb2_cohort_run) without and with intervals (vb2_cohort_run_intervals).
The sides alternate (a b a b ..., c- c+ c- c+ ...); per side the median and the range over VB2_REPS repetitions.
Writes its table to stdout and, with an argument, to that file as well (profiles/cohort_interval/).
VB2_S, VB2_REPS, VB2_SHAPES ("3000:2,100000:4") size it down."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import verifybamid_amd as vb  # noqa: E402

S = int(os.environ.get("VB2_S", 32))
REPS = int(os.environ.get("VB2_REPS", 5))
SHAPES = [tuple(int(x) for x in s.split(":")) for s in os.environ.get("VB2_SHAPES", "3000:2,100000:4").split(",")]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stats(xs):
    return "median %8.2f ms  (range %8.2f - %8.2f)" % (1e3 * float(np.median(xs)), 1e3 * min(xs), 1e3 * max(xs))


def samples(M, k):
    """One panel and S samples on it."""
    base = vb.synth.with_sanity_stats(vb.synth.make_pileup(M, 30, k, 0.05, 2))
    data = []
    for s in range(S):
        d = vb.synth.make_pileup(M, 30, k, alpha_true=0.01 * (1 + s % 20), seed=1000 + s)
        data.append(vb.PileupData(k, base.ud, base.means, d.read_off, d.bases, d.quals, base.alt_base, None,
                                  d.avg_depth, d.sd_depth, True, dict(base.meta)))
    return base, data


def contexts_side(M, k, data):
    ctxs = [vb.LikelihoodContext(d, cohort_layout=True) for d in data]
    try:
        with vb.CohortBatch(ctxs) as batch:
            ests = batch.optimize()
            alone = [c.interval(e) for c, e in zip(ctxs, ests)]          # (warm: scratch, code objects)
            together = batch.intervals(ests)
            steps = batch.num_interval_step
            for x, y in zip(alone, together):
                assert x["lo"] == y["lo"] and x["hi"] == y["hi"] and x["num_launch"] == y["num_launch"]
            ta, tb = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                for c, e in zip(ctxs, ests):
                    c.interval(e)
                ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                batch.intervals(ests)
                tb.append(time.perf_counter() - t0)
        launches = [x["num_launch"] for x in alone]
        say("%d x 30, k = %d, S = %d: derivative launches per sample %d - %d (sum %d), lock-step steps %d"
            % (M, k, S, min(launches), max(launches), sum(launches), steps))
        say("  (a) vb2_ctx_interval, sample after sample: %s = %.2f ms per sample, %.1f us per launch"
            % (stats(ta), 1e3 * np.median(ta) / S, 1e6 * np.median(ta) / sum(launches)))
        say("  (b) vb2_batch_interval, lock-step:          %s = %.2f ms per sample, %.1f us per step"
            % (stats(tb), 1e3 * np.median(tb) / S, 1e6 * np.median(tb) / steps))
        say("      (a) / (b) = %.2f" % (np.median(ta) / np.median(tb)))
    finally:
        for c in ctxs:
            c.close()


def files_side(M, k, base, data):
    tmp = tempfile.mkdtemp()
    pre = vb.synth.write_files(base, os.path.join(tmp, "panel"))
    piles = [vb.synth.write_files(d, os.path.join(tmp, "s%d" % s)) + ".pileup" for s, d in enumerate(data)]
    outs = [os.path.join(tmp, "out%d" % s) for s in range(S)]
    print("%d pileups written" % S, flush=True)
    vb.run_cohort_files(pre, piles, outs, num_pc=k)                       # (warm: page cache, code objects)
    t = {False: [], True: []}
    for _ in range(REPS):
        for ci in (False, True):
            t0 = time.perf_counter()
            res = vb.run_cohort_files(pre, piles, outs, num_pc=k, confidence_interval=ci)
            t[ci].append(time.perf_counter() - t0)
            assert all(r["status"] == 0 for r in res)
    say("  (c) cohort run from %d files, without intervals: %s = %.2f ms per sample" % (S, stats(t[False]), 1e3 * np.median(t[False]) / S))
    say("      cohort run from %d files, with intervals:    %s = %.2f ms per sample" % (S, stats(t[True]), 1e3 * np.median(t[True]) / S))
    say("      the intervals add %.2f ms per sample to the run" % (1e3 * (np.median(t[True]) - np.median(t[False])) / S))


for M, k in SHAPES:
    base, data = samples(M, k)
    print("%d x 30, k = %d: %d samples drawn" % (M, k, S), flush=True)
    contexts_side(M, k, data)
    files_side(M, k, base, data)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
