"""What the likelihood given a hypothesised contaminant costs on one MI355X:
  (1) a 48-point launch pair of llk_sum_marker_kernel under the prior term (marker_sum_kernels.hip) + its reduction at
      100 000 x 30, k = 4, in both layouts, beside the yardstick: the same kernel under the weight term on the SAME context
      with all-ones weight rows -- the two terms differ by three float loads and a select.  HIP events around the launches (vb2_debug_conditioned_time /
      vb2_debug_replicates_time), after a warm-up; the two are timed in alternating rounds and medians reported, with the
      spread of the rounds' medians.
  (2) the wall-clock --RefitSource adds to a cohort run (32 samples x 100 000 x 30, k = 4, 8 of them contaminated at 5 % by
      another member): vb2_cohort_run_sources against vb2_cohort_run_source_fits on the same files, three alternating
      repetitions each after one warm-up run of each.
Writes JSON and a text table under --out (profiles/conditioned/).  --markers / --cohort size it down (a rehearsal)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import verifybamid_amd as vb  # noqa: E402
from verifybamid_amd import _abi  # noqa: E402
import source_ref as sr  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, handle, points, warmup, reps):
    ms = (C.c_double * reps)()
    _abi.check(fn(handle, points, warmup, reps, ms), "time_launch")
    return list(ms)


def launch_pairs(M, k, points, rounds, reps, out):
    lib = _abi.lib()
    d = vb.synth.make_pileup(M, 30, k, 0.05, 2)
    rng = np.random.default_rng(3)
    prior = rng.dirichlet(np.ones(3), size=(6, M)).astype(np.float32)        # six hypotheses of non-zero triples
    out["launch_pair"] = {}
    for pd in (1, 0):
        _abi.set_tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx, vb.Conditioned(ctx, prior) as cond, \
                vb.Replicates(ctx, np.ones((6, M), dtype=np.uint8)) as rep:
            layout = ctx.info()["layout"]
            # the same values first (section 6 of the measuring rules): all-zero triples are the weighted kernel's all-ones row
            with vb.Conditioned(ctx, np.zeros((1, M, 3), dtype=np.float32)) as zero:
                p1, p2, al = np.full((1, k), 0.01), np.full((1, k), 0.01), np.array([0.03])
                a, b = zero.eval([1], p1, p2, al)[0], rep.eval([1, 0, 0, 0, 0, 0], p1, p2, al)[0]
                assert abs(a - b) <= 1e-12 * abs(b), (a, b)
            new, old = [], []
            for r in range(rounds):                                           # alternating, each with its own warm-up
                new.append(timed(lib.vb2_debug_conditioned_time, cond._h, points, 3, reps))
                old.append(timed(lib.vb2_debug_replicates_time, rep._h, points, 3, reps))
            mn, mo = [float(np.median(x)) for x in new], [float(np.median(x)) for x in old]
            res = dict(points=points, markers=M, num_pc=k, conditioned_ms=float(np.median(np.concatenate(new))),
                       weighted_ms=float(np.median(np.concatenate(old))), conditioned_round_medians_ms=mn,
                       weighted_round_medians_ms=mo, num_read=int(ctx.info()["num_read"]))
            res["ratio"] = res["conditioned_ms"] / res["weighted_ms"]
            out["launch_pair"]["layout %d" % layout] = res
            say("launch pair, %d points, %d x 30, k = %d, layout %d: conditioned %.4f ms (rounds %.4f .. %.4f), weighted all-ones "
                "%.4f ms (rounds %.4f .. %.4f): %.3f x" % (points, M, k, layout, res["conditioned_ms"], min(mn), max(mn),
                                                           res["weighted_ms"], min(mo), max(mo), res["ratio"]))
    _abi.set_tunable("pd", 1)


def cohort(M, k, S, contaminated, reps, out):
    tmp = tempfile.mkdtemp()
    panel = sr.make_panel(M, k, seed=5)
    G = sr.draw_individuals(panel, S + 1, seed=6)
    data = []
    for i in range(S):
        src, alpha = ((i + 1) % S, 0.05) if i < contaminated else (S, 1e-3)
        data.append(sr.make_sample(panel, G[i], G[src], 30, alpha, 100 + i))
    prefix = vb.synth.write_files(vb.synth.with_sanity_stats(data[0]), os.path.join(tmp, "panel"))
    chrs, poss = ["1"] * M, 1000 + 10 * np.arange(M)
    piles = []
    for i, d in enumerate(data):
        p = os.path.join(tmp, "s%02d.pileup" % i)
        vb.synth.write_pileup_text(p, chrs, poss, panel["ref"], d.read_off, d.bases, d.quals)
        piles.append(p)
    outs = [os.path.join(tmp, "o%02d" % i) for i in range(S)]

    def run(refit):
        t0 = time.perf_counter()
        res, src = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=k, find_source=True, refit_source=refit,
                                       sources_prefix=os.path.join(tmp, "run"))
        return time.perf_counter() - t0, res, src
    run(False), run(True)                                                     # warm: code objects, the page cache, the slabs
    plain, fits, last = [], [], None
    for _ in range(reps):
        plain.append(run(False)[0])
        t, res, last = run(True)
        fits.append(t)
    refitted = [f for f in last["fit"] if f["status"] == 0]
    right = sum(1 for i in range(contaminated) if last["fit"][i]["status"] == 0 and last["fit"][i]["candidate"] == (i + 1) % S)
    out["cohort"] = dict(samples=S, markers=M, num_pc=k, contaminated=contaminated, find_source_s=plain, refit_source_s=fits,
                         added_s=float(np.median(fits) - np.median(plain)), refits=len(refitted), true_source_refits=right)
    say("cohort of %d x %d x 30, k = %d, %d contaminated: --FindSource %s s, with --RefitSource %s s: the flag adds %.3f s "
        "(medians; %d refits, %d of them given the true source)"
        % (S, M, k, contaminated, ", ".join("%.3f" % t for t in plain), ", ".join("%.3f" % t for t in fits),
           out["cohort"]["added_s"], len(refitted), right))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--points", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cohort", type=int, default=32)
    ap.add_argument("--contaminated", type=int, default=8)
    a = ap.parse_args()
    out = {}
    launch_pairs(a.markers, 4, a.points, a.rounds, a.reps, out)
    if a.cohort > 0:
        cohort(a.markers, 4, a.cohort, min(a.contaminated, a.cohort), 3, out)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "conditioned_time.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "conditioned_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
