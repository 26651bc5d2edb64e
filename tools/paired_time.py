"""What the likelihood given priors on both components costs on one MI355X:
  (1) a 48-point launch pair of llk_sum_marker_kernel under the pair term (marker_sum_kernels.hip) + its reduction at
      100 000 x 30, k = 4, in both layouts, beside the yardstick: the same kernel under the prior term on the SAME context
      with the same triples as pi1 -- the two terms differ by three more float loads, the left-out test and three more
      selects.  HIP events around the launches (vb2_debug_paired_time / vb2_debug_conditioned_time), after a warm-up; the two
      are timed in alternating rounds and medians reported, with the spread of the rounds' medians.  A third figure: the pair
      term under the matched-normal rule at 0.99, where about a third of the markers are left out and not walked.
  (2) the wall-clock --MatchedNormal adds to a cohort run (32 samples x 100 000 x 30, k = 4, 8 tumour-normal pairs):
      vb2_cohort_run against vb2_cohort_run_paired on the same files, three alternating repetitions each after one warm-up
      run of each.
Writes JSON and a text table under --out (profiles/paired/).  --markers / --cohort size it down (a rehearsal)."""
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


def timed(fn, handle, points, warmup, reps):
    ms = (C.c_double * reps)()
    _abi.check(fn(handle, points, warmup, reps, ms), "time_launch")
    return list(ms)


def launch_pairs(M, k, points, rounds, reps, out):
    lib = _abi.lib()
    d = vb.synth.make_pileup(M, 30, k, 0.05, 2)
    rng = np.random.default_rng(3)
    prior = rng.dirichlet(np.ones(3), size=(6, M)).astype(np.float32)        # six hypotheses of non-zero triples
    both = np.concatenate([prior, prior[::-1]], axis=2)                       # ... on both sides
    # the matched-normal rule on a clean sample's posterior: what a paired refit evaluates
    normal = vb.synth.make_pileup(M, 30, k, 1e-3, 4)
    z = np.zeros(k)
    rule = pr.normal_rule(sr.sample_rows(normal, z, z, 1e-3)[1].astype(np.float32), 0.99)
    out["launch_pair"] = {}
    for pd in (1, 0):
        _abi.set_tunable("pd", pd)
        with vb.LikelihoodContext(d) as ctx, vb.Paired(ctx, both) as pair, vb.Conditioned(ctx, prior) as cond, \
                vb.Paired(ctx, np.stack([rule] * 6)) as ruled:
            layout = ctx.info()["layout"]
            # the same values first: with pi2 all zero the pair term is the prior term
            with vb.Paired(ctx, np.concatenate([prior[:1], np.zeros_like(prior[:1])], axis=2)) as half:
                p1, p2, al = np.full((1, k), 0.01), np.full((1, k), 0.01), np.array([0.03])
                a, b = half.eval([1], p1, p2, al)[0], cond.eval([1, 0, 0, 0, 0, 0], p1, p2, al)[0]
                assert abs(a - b) <= 1e-12 * abs(b), (a, b)
            new, old, thin = [], [], []
            for r in range(rounds):                                           # alternating, each with its own warm-up
                new.append(timed(lib.vb2_debug_paired_time, pair._h, points, 3, reps))
                old.append(timed(lib.vb2_debug_conditioned_time, cond._h, points, 3, reps))
                thin.append(timed(lib.vb2_debug_paired_time, ruled._h, points, 3, reps))
            mn, mo, mt = ([float(np.median(x)) for x in y] for y in (new, old, thin))
            res = dict(points=points, markers=M, num_pc=k, paired_ms=float(np.median(np.concatenate(new))),
                       conditioned_ms=float(np.median(np.concatenate(old))), rule_ms=float(np.median(np.concatenate(thin))),
                       paired_round_medians_ms=mn, conditioned_round_medians_ms=mo, rule_round_medians_ms=mt,
                       rule_given=int(ruled.info()["given"][0]), num_active=int(ctx.info()["num_active_marker"]),
                       num_read=int(ctx.info()["num_read"]))
            res["ratio"] = res["paired_ms"] / res["conditioned_ms"]
            res["rule_ratio"] = res["rule_ms"] / res["conditioned_ms"]
            out["launch_pair"]["layout %d" % layout] = res
            say("launch pair, %d points, %d x 30, k = %d, layout %d: paired %.4f ms (rounds %.4f .. %.4f), conditioned %.4f ms "
                "(rounds %.4f .. %.4f): %.3f x; under the 0.99 rule (%d of %d markers walked) %.4f ms (rounds %.4f .. %.4f): %.3f x"
                % (points, M, k, layout, res["paired_ms"], min(mn), max(mn), res["conditioned_ms"], min(mo), max(mo), res["ratio"],
                   res["rule_given"], res["num_active"], res["rule_ms"], min(mt), max(mt), res["rule_ratio"]))
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

    def run(paired):
        t0 = time.perf_counter()
        got = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=k, matched_normal=listed if paired else None,
                                  sources_prefix=os.path.join(tmp, "run"))
        return time.perf_counter() - t0, got
    run(False), run(True)                                                     # warm: code objects, the page cache, the slabs
    plain, with_flag, last = [], [], None
    for _ in range(reps):
        plain.append(run(False)[0])
        t, last = run(True)
        with_flag.append(t)
    fits = last[1]
    done = [f for f in fits if f["status"] == 0]
    out["cohort"] = dict(samples=S, markers=M, num_pc=k, pairs=pairs, plain_s=plain, matched_normal_s=with_flag,
                         added_s=float(np.median(with_flag) - np.median(plain)), refits=len(done),
                         alpha_paired=[f["alpha_paired"] for f in fits], freemix=[f["freemix"] for f in fits],
                         markers_given=[f["markers"] for f in fits])
    say("cohort of %d x %d x 30, k = %d, %d pairs: plain %s s, with --MatchedNormal %s s: the flag adds %.3f s (medians; %d refits, "
        "ALPHA_PAIRED %.4f .. %.4f for a planted 0.05)"
        % (S, M, k, pairs, ", ".join("%.3f" % t for t in plain), ", ".join("%.3f" % t for t in with_flag), out["cohort"]["added_s"],
           len(done), min(f["alpha_paired"] for f in done), max(f["alpha_paired"] for f in done)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--points", type=int, default=48)
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
        with open(os.path.join(a.out, "paired_time.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "paired_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
