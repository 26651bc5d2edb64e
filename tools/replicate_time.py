"""What a set of likelihood replicates costs on one MI355X, two ways:
  (new)    vb2_replicates_*: weight rows over the ONE resident sample, all searches in lock-step (create + optimize);
  (parent) what the library could do before: one context per replicate built from the EXPANDED input (marker i repeated
           w_i times, tests/replicate_ref.py), searched with vb2_batch_optimize_llk in groups of at most 64 contexts (the
           cohort runner's group limit), context creation included -- the host-side expansion itself is not counted.
for  (A) the 22 + 22 chromosome set ("only" and "without") on a hapmap-panel sample, depth 30, k = 2, and
     (B) a 200-replicate marker bootstrap of a 100 000 x 30 sample, k = 4.
Per run: wall-clock of each way, time per lock-step step and per replicate, device bytes both ways, and how far the two
ways' FREEMIX estimates are apart.  Writes its table to stdout and, with an argument, to that file (profiles/replicates/).
VB2_RUNS ("A,B"), VB2_BOOT (200), VB2_BOOT_SHAPE ("100000:4") size it down."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import verifybamid_amd as vb  # noqa: E402
import replicate_ref  # noqa: E402

HAPMAP = os.path.join(ROOT, "tests", "golden", "hapmap", "hapmap_3.3.b37.dat")
RUNS = os.environ.get("VB2_RUNS", "A,B").split(",")
BOOT = int(os.environ.get("VB2_BOOT", 200))
BOOT_M, BOOT_K = (int(x) for x in os.environ.get("VB2_BOOT_SHAPE", "100000:4").split(":"))
GROUP = 64
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def freemix(e):
    return e["alpha"] if e["alpha"] < 0.5 else 1 - e["alpha"]


def new_way(d, weights):
    with vb.LikelihoodContext(d) as ctx:
        ctx.optimize()                                                    # (warm: code objects, the slab cache)
        with vb.Replicates(ctx, weights[:2]) as rep:
            rep.optimize()
        t0 = time.perf_counter()
        with vb.Replicates(ctx, weights) as rep:
            t1 = time.perf_counter()
            est = rep.optimize()
            t2 = time.perf_counter()
            info = rep.info()
        sample_bytes = ctx.info()["device_bytes"]
    return dict(create=t1 - t0, search=t2 - t1, steps=info["num_step"], launches=info["num_launch"],
                bytes=info["device_bytes"], sample_bytes=sample_bytes, est=est)


def parent_way(d, weights):
    R = len(weights)
    est, t_create, t_search, t_expand, dev_bytes, steps = [], 0.0, 0.0, 0.0, 0, 0
    for lo in range(0, R, GROUP):
        ctxs = []
        try:
            for r in range(lo, min(R, lo + GROUP)):
                t0 = time.perf_counter()
                e = replicate_ref.expand(d, weights[r])
                t1 = time.perf_counter()
                ctxs.append(vb.LikelihoodContext(e, cohort_layout=True))
                t_expand += t1 - t0
                t_create += time.perf_counter() - t1
            dev_bytes += sum(c.info()["device_bytes"] for c in ctxs)       # (a group's contexts are alive together)
            t0 = time.perf_counter()
            with vb.CohortBatch(ctxs) as batch:
                est += batch.optimize()
            t_search += time.perf_counter() - t0
        finally:
            for c in ctxs:
                c.close()
    return dict(create=t_create, search=t_search, expand=t_expand, bytes=dev_bytes, est=est)


def report(title, d, weights):
    R = len(weights)
    a = new_way(d, weights)
    b = parent_way(d, weights)
    ok = [r for r in range(R) if a["est"][r]["status"] == 0]
    gap = max(abs(freemix(a["est"][r]) - freemix(b["est"][r])) for r in ok)
    ta, tb = a["create"] + a["search"], b["create"] + b["search"]
    say(title)
    say("  replicates over the resident sample: create %8.2f ms + search %9.2f ms = %9.2f ms; %d lock-step steps (%d marker "
        "launches), %.1f us per step, %.2f ms per replicate; device bytes %.2f MB beside the sample's %.2f MB"
        % (1e3 * a["create"], 1e3 * a["search"], 1e3 * ta, a["steps"], a["launches"], 1e6 * a["search"] / max(1, a["steps"]),
           1e3 * ta / R, a["bytes"] / 1e6, a["sample_bytes"] / 1e6))
    say("  one context per replicate (expanded): create %8.2f ms + search %9.2f ms = %9.2f ms; %.2f ms per replicate; device "
        "bytes %.2f MB (at most %d contexts alive together: %.2f MB); host-side expansion, not counted: %.2f ms"
        % (1e3 * b["create"], 1e3 * b["search"], 1e3 * tb, 1e3 * tb / R, b["bytes"] / 1e6, GROUP,
           b["bytes"] / 1e6 * min(1.0, GROUP / R), 1e3 * b["expand"]))
    say("  %s wins at %d replicates: %.2f x the other's time; the two ways' FREEMIX differ by at most %.2g"
        % ("the replicate set" if ta < tb else "one context per replicate", R, max(ta, tb) / min(ta, tb), gap))


if "A" in RUNS:
    chrs, poss, refs, alts = vb.synth.read_bed_rows(HAPMAP + ".bed")
    mu = vb.synth.read_mu_column(HAPMAP + ".mu")
    off, bases, quals = vb.synth.reads_on_panel(mu, refs, alts, 30.0, 0.05, 1)
    ud = np.loadtxt(HAPMAP + ".UD")[:, :2]
    d = vb.synth.with_sanity_stats(vb.PileupData(2, ud, mu, off, bases, quals, alts, None, float(off[-1]) / len(chrs), 0.0, True))
    cw = vb.chromosome_weights(HAPMAP + ".bed", d.num_marker)
    report("(A) hapmap panel, %d markers x 30, k = 2: 22 + 22 chromosome replicates" % d.num_marker, d,
           np.concatenate([cw["only"], cw["without"]]))
if "B" in RUNS:
    d = vb.synth.make_pileup(BOOT_M, 30, BOOT_K, 0.05, 2)
    report("(B) %d x 30, k = %d: %d bootstrap replicates" % (BOOT_M, BOOT_K, BOOT), d, vb.bootstrap_weights(BOOT_M, BOOT, 1))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
