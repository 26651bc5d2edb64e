"""What the derivatives of the paired likelihood and --PairInterval cost on one MI355X, on
tools/paired_time.py's protocol:
  (1) a 4-point launch pair of the prior-aware marker kernel (deriv_kernels.hip: PairPrior) + the reduction at 100 000 x 30,
      k = 4, in both layouts, beside the yardstick: the anonymous pair of vb2_llk_derivs_batch on the SAME context.  First with
      all-zero priors (the same arithmetic: the cost of the Prior alone), then under the matched-normal rule at 0.99, where
      about a third of the markers are left out and not walked.  HIP events around the launches
      (vb2_debug_paired_derivs_time), after a warm-up; the three are timed in five alternating rounds and medians reported,
      with the spread of the rounds' medians.
  (2) the wall-clock --PairInterval adds to a --MatchedNormal cohort run (32 samples x 100 000 x 30, k = 4, 8 tumour-normal
      pairs): vb2_cohort_run_paired against vb2_cohort_run_paired_intervals on the same files, three alternating repetitions
      each after one warm-up run of each.
Writes JSON and a text table under --out (profiles/paired_interval/).  --markers / --cohort size it down (a rehearsal)."""
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
import paired_ref as pr  # noqa: E402
import source_ref as sr  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(handle, hyp, points, warmup, reps):
    ms = (C.c_double * reps)()
    _abi.check(_abi.lib().vb2_debug_paired_derivs_time(handle, hyp, points, warmup, reps, ms), "vb2_debug_paired_derivs_time")
    return list(ms)


def launch_pairs(M, k, points, rounds, reps, out):
    d = vb.synth.make_pileup(M, 30, k, 0.05, 2)
    normal = vb.synth.make_pileup(M, 30, k, 1e-3, 4)
    z = np.zeros(k)
    rule = pr.normal_rule(sr.sample_rows(normal, z, z, 1e-3)[1].astype(np.float32), 0.99)
    out["launch_pair"] = {}
    for pd in (1, 0):
        _abi.set_tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, np.stack([pr.hypothesis(M), rule])) as pair:
            layout = ctx.info()["layout"]
            # the same values first: all-zero priors give the anonymous kernels' bits
            p1, p2, al = np.full((points, k), 0.01), np.full((points, k), 0.01), np.full(points, 0.03)
            for x, y in zip(pair.derivatives([points, 0], p1, p2, al), ctx.derivatives(p1, p2, al)):
                assert np.array_equal(x, y)
            anon, zero, thin = [], [], []
            for r in range(rounds):                                           # alternating, each with its own warm-up
                zero.append(timed(pair._h, 0, points, 3, reps))
                anon.append(timed(pair._h, -1, points, 3, reps))
                thin.append(timed(pair._h, 1, points, 3, reps))
            ma, mz, mt = ([float(np.median(x)) for x in y] for y in (anon, zero, thin))
            res = dict(points=points, markers=M, num_pc=k, anonymous_ms=float(np.median(np.concatenate(anon))),
                       zero_priors_ms=float(np.median(np.concatenate(zero))), rule_ms=float(np.median(np.concatenate(thin))),
                       anonymous_round_medians_ms=ma, zero_priors_round_medians_ms=mz, rule_round_medians_ms=mt,
                       rule_given=int(pair.info()["given"][1]), num_active=int(ctx.info()["num_active_marker"]))
            res["zero_ratio"] = res["zero_priors_ms"] / res["anonymous_ms"]
            res["rule_ratio"] = res["rule_ms"] / res["anonymous_ms"]
            out["launch_pair"]["layout %d" % layout] = res
            say("launch pair, %d points, %d x 30, k = %d, layout %d: anonymous %.4f ms (rounds %.4f .. %.4f); all-zero priors "
                "%.4f ms (rounds %.4f .. %.4f): %.3f x; under the 0.99 rule (%d of %d markers walked) %.4f ms (rounds %.4f .. "
                "%.4f): %.3f x"
                % (points, M, k, layout, res["anonymous_ms"], min(ma), max(ma), res["zero_priors_ms"], min(mz), max(mz),
                   res["zero_ratio"], res["rule_given"], res["num_active"], res["rule_ms"], min(mt), max(mt), res["rule_ratio"]))
    _abi.set_tunable("pd", 1)


def cohort(M, k, S, pairs, reps, out):
    tmp = tempfile.mkdtemp()
    panel = sr.make_panel(M, k, seed=5)
    G = sr.draw_individuals(panel, S + 1, seed=6)
    data, listed = [], []
    for i in range(S):
        if i < 2 * pairs and i % 2 == 0:                                      # a tumour: 5 % of an outsider, then its normal
            data.append(sr.make_sample(panel, G[i], G[S], 30, 0.05, 100 + i))
            listed.append((i, i + 1))
        elif i < 2 * pairs:
            data.append(sr.make_sample(panel, G[i - 1], G[S], 30, 1e-3, 100 + i))
        else:
            data.append(sr.make_sample(panel, G[i], G[S], 30, 1e-3, 100 + i))
    prefix = vb.synth.write_files(vb.synth.with_sanity_stats(data[0]), os.path.join(tmp, "panel"))
    chrs, poss = ["1"] * M, 1000 + 10 * np.arange(M)
    piles = []
    for i, d in enumerate(data):
        p = os.path.join(tmp, "s%02d.pileup" % i)
        vb.synth.write_pileup_text(p, chrs, poss, panel["ref"], d.read_off, d.bases, d.quals)
        piles.append(p)
    outs = [os.path.join(tmp, "o%02d" % i) for i in range(S)]

    def run(interval):
        t0 = time.perf_counter()
        got = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=k, matched_normal=listed, pair_interval=interval,
                                  sources_prefix=os.path.join(tmp, "run"))
        return time.perf_counter() - t0, got
    run(False), run(True)                                                     # warm: code objects, the page cache, the slabs
    plain, with_flag, last = [], [], None
    for _ in range(reps):
        plain.append(run(False)[0])
        t, last = run(True)
        with_flag.append(t)
    fits = last[1]
    done = [f for f in fits if "interval" in f]
    out["cohort"] = dict(samples=S, markers=M, num_pc=k, pairs=pairs, matched_normal_s=plain, pair_interval_s=with_flag,
                         added_s=float(np.median(with_flag) - np.median(plain)), intervals=len(done),
                         alpha_paired=[f["alpha_paired"] for f in fits], lo=[f["interval"]["lo"] for f in done],
                         hi=[f["interval"]["hi"] for f in done], num_launch=[f["interval"]["num_launch"] for f in done])
    say("cohort of %d x %d x 30, k = %d, %d pairs: --MatchedNormal %s s, with --PairInterval %s s: the flag adds %.3f s (medians; "
        "%d intervals, %d .. %d derivative launches each)"
        % (S, M, k, pairs, ", ".join("%.3f" % t for t in plain), ", ".join("%.3f" % t for t in with_flag), out["cohort"]["added_s"],
           len(done), min(out["cohort"]["num_launch"]), max(out["cohort"]["num_launch"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--points", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cohort", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=8)
    a = ap.parse_args()
    out = {}
    launch_pairs(a.markers, 4, a.points, a.rounds, a.reps, out)
    if a.cohort > 0:
        cohort(a.markers, 4, a.cohort, min(a.pairs, a.cohort // 2), 3, out)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "paired_interval_time.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "paired_interval_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
