"""What the reference bias costs on one MI355X.  Reports, asserts nothing but equal values:
  (1) a 48-point launch pair of llk_bias_marker_kernel (refbias_kernels.hip) + its reduction at 100 000 x 30, k = 4, in both
      layouts, beside the yardstick on the SAME context: llk_sum_marker_kernel under the prior term with all-zero hypotheses
      (marker_sum_kernels.hip) -- the bias kernel builds a table of fourteen columns instead of six and carries a seventh
      product per step.  HIP events around the launches (vb2_debug_refbias_time / vb2_debug_conditioned_time), after a
      warm-up; the two are timed in alternating rounds and medians reported, with the spread of the rounds' medians.
  (2) the wall-clock --RefBias adds to a one-sample run (100 000 x 30, k = 4, beta planted at 0.58): vb2_run against
      vb2_run_refbias on the same files, three alternating repetitions each after one warm-up run of each -- 28 refits in five
      lock-step calls behind the run's own search.
Writes JSON and a text table under --out (profiles/refbias/).  --markers sizes it down (a rehearsal)."""
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
import refbias_ref as rr  # noqa: E402

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
    betas = [0.25, 0.4, 0.5, 0.58, 0.66, 0.75]
    out["launch_pair"] = {}
    for pd in (1, 0):
        _abi.set_tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx, vb.RefBias(ctx, betas) as rb, \
                vb.Conditioned(ctx, np.zeros((6, M, 3), dtype=np.float32)) as cond:
            layout = ctx.info()["layout"]
            # the same values first: the row at 0.5 is the prior term's all-zero hypothesis
            p1, p2, al = np.full((1, k), 0.01), np.full((1, k), 0.01), np.array([0.03])
            a, b = rb.eval([0, 0, 1, 0, 0, 0], p1, p2, al)[0], cond.eval([1, 0, 0, 0, 0, 0], p1, p2, al)[0]
            assert abs(a - b) <= 1e-12 * abs(b), (a, b)
            new, old = [], []
            for r in range(rounds):                                           # alternating, each with its own warm-up
                new.append(timed(lib.vb2_debug_refbias_time, rb._h, points, 3, reps))
                old.append(timed(lib.vb2_debug_conditioned_time, cond._h, points, 3, reps))
            mn, mo = [float(np.median(x)) for x in new], [float(np.median(x)) for x in old]
            res = dict(points=points, markers=M, num_pc=k, refbias_ms=float(np.median(np.concatenate(new))),
                       prior_ms=float(np.median(np.concatenate(old))), refbias_round_medians_ms=mn, prior_round_medians_ms=mo,
                       num_read=int(ctx.info()["num_read"]))
            res["ratio"] = res["refbias_ms"] / res["prior_ms"]
            out["launch_pair"]["layout %d" % layout] = res
            say("launch pair, %d points, %d x 30, k = %d, layout %d: bias %.4f ms (rounds %.4f .. %.4f), prior term all-zero "
                "%.4f ms (rounds %.4f .. %.4f): %.3f x" % (points, M, k, layout, res["refbias_ms"], min(mn), max(mn),
                                                           res["prior_ms"], min(mo), max(mo), res["ratio"]))
    _abi.set_tunable("pd", 1)


def one_sample(M, k, reps, out):
    tmp = tempfile.mkdtemp()
    d = rr.make_sample(M, 30, k, 0.03, 0.58, 7, q_lo=20, q_hi=40)
    prefix = vb.synth.write_files(d, os.path.join(tmp, "s"))

    def run(bias):
        t0 = time.perf_counter()
        res = vb.run_files(prefix, prefix + ".pileup", os.path.join(tmp, "o"), num_pc=k, disable_sanity=True, ref_bias=bias)
        return time.perf_counter() - t0, res
    run(False), run(True)                                                     # warm: code objects, the page cache, the slabs
    plain, biased, last, search = [], [], None, []
    for _ in range(reps):
        t, res = run(False)
        plain.append(t)
        search.append(res["seconds_optimize"])
        t, last = run(True)
        biased.append(t)
    f = last["ref_bias"]
    out["one_sample"] = dict(markers=M, num_pc=k, run_s=plain, run_refbias_s=biased, search_s=search,
                             added_s=float(np.median(biased) - np.median(plain)), beta=f["beta"], beta_se=f["beta_se"], lrt=f["lrt"],
                             freemix=min(last["alpha"], 1 - last["alpha"]), freemix_bias=f["freemix_bias"], num_step=f["num_step"],
                             num_refit=f["num_refit"])
    say("one sample of %d x 30, k = %d, beta planted at 0.58: run %s s (search %.4f s), with --RefBias %s s: the flag adds %.3f s "
        "= %.0f x the search (medians; %d refits, %d lock-step steps); beta %.4f (SE %.4f), LRT %.1f, FREEMIX %.4f fitted, %.4f at 0.5"
        % (M, k, ", ".join("%.3f" % t for t in plain), float(np.median(search)), ", ".join("%.3f" % t for t in biased),
           out["one_sample"]["added_s"], out["one_sample"]["added_s"] / max(float(np.median(search)), 1e-9), f["num_refit"],
           f["num_step"], f["beta"], f["beta_se"], f["lrt"], f["freemix_bias"], out["one_sample"]["freemix"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--points", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {}
    launch_pairs(a.markers, 4, a.points, a.rounds, a.reps, out)
    one_sample(a.markers, 4, 3, out)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "refbias_time.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "refbias_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
