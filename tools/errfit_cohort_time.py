"""What the cohort form of the error-rate fit costs and what pooling buys.

On the device (default), 32 samples of 100 000 x 30, k = 4, on one shared panel:
  * the batched E-step (one vb2_errstat_batch_eval) against the parent's way, 32 vb2_errstat_eval back to back on the same
    samples, points and table -- alternated, five rounds each after a warm-up; a gain is claimed only where the medians lie
    apart by at least three times the larger range (the bar of profiles/r15);
  * the launch's time against the bytes it must read, by section 23's arithmetic;
  * where the time of a cohort fit goes (E-steps, contexts, searches), per sample and pooled, and the device bytes held.
Raw output to profiles/errfit_cohort/errfit_cohort_time.{txt,json}.

    python tools/errfit_cohort_time.py [--samples 32] [--markers 100000] [--depth 30] [--pcs 4]

With --stat (no device: the numpy restatement), the statistical claim: 8 samples of 3 000 x depth 10 with one planted q - 5
shift, over four seed sets -- how far the pooled and the per-sample rates lie from the planted ones in SE_BINOM units, and
FREEMIX before and after.  Raw output to profiles/errfit_cohort/pooling_stat.{txt,json}.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import verifybamid_amd as vb  # noqa: E402

STEP_TBPS = 5.0                   # what the cohort step reaches: the yardstick of the floor


def _writer(out_dir, name):
    os.makedirs(out_dir, exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def done(res):
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
    return say, done


def _spread(xs):
    return max(xs) - min(xs)


def device(a):
    say, done = _writer(a.out, "errfit_cohort_time")
    S, k = a.samples, a.pcs
    d0 = vb.synth.make_pileup(a.markers, mean_depth=a.depth, num_pc=k, alpha_true=0.03, seed=7)
    datas = [d0]
    for s in range(1, S):                       # the samples of a cohort share the panel: the same ud / means arrays
        off, ch, q = vb.synth.reads_on_panel(d0.means, d0.meta["ref_base"], d0.alt_base, mean_depth=a.depth, alpha_true=0.03,
                                             seed=100 + s)
        datas.append(vb.PileupData(k, d0.ud, d0.means, off, ch, q, d0.alt_base, None, 0.0, 0.0, True, dict(d0.meta)))
    noms = []
    for d in datas:
        with vb.LikelihoodContext(d) as ctx:
            noms.append(ctx.optimize())
    table = vb.nominal_err_table()
    p1, p2, al = [n["pc"] for n in noms], [n["pc2"] for n in noms], [n["alpha"] for n in noms]
    singles = [vb.ErrStat(d) for d in datas]
    batch = vb.ErrStatBatch(datas)
    info = batch.info()

    def parent_way():
        return [es.eval(table, p1[i], p2[i], al[i]) for i, es in enumerate(singles)]

    def batched():
        return batch.eval(table, p1, p2, al)
    want, got = parent_way(), batched()                                          # warm-up, and the same bits
    for i in range(S):
        assert got[0][i].tobytes() == want[i][0].tobytes() and got[1][i].tobytes() == want[i][1].tobytes()
        assert np.float64(got[2][i]).tobytes() == np.float64(want[i][2]).tobytes()
    t_par, t_bat = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        parent_way()
        t_par.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        batched()
        t_bat.append(time.perf_counter() - t0)
    grid = batch.info()["last_grid"]
    single_bytes = sum(es.info()["device_bytes"] for es in singles)
    for es in singles:
        es.close()
    R, M = sum(d.num_read for d in datas), sum(d.num_marker for d in datas)
    panel = M * (8 * k + 8 + 8 + 1)                          # panel row, mean, offset, alt per marker and sample
    traffic_23 = 2 * 2 * R + panel                           # section 23: two passes over bases and qualities
    traffic_once = 2 * R + panel                             # a group that is one chunk is staged once for both passes
    med_par, med_bat = statistics.median(t_par), statistics.median(t_bat)
    apart = abs(med_par - med_bat)
    bar = 3 * max(_spread(t_par), _spread(t_bat))
    say("%d samples, %d markers and %d reads in all, k = %d, %d panel cop%s on the device; the set holds %d bytes "
        "(%d single sets: %d)" % (S, M, R, k, info["num_panel"], "y" if info["num_panel"] == 1 else "ies", info["device_bytes"],
                                  S, single_bytes))
    say("parent's way, %d vb2_errstat_eval back to back: median %.3f ms (%s)"
        % (S, med_par * 1e3, ", ".join("%.3f" % (t * 1e3) for t in t_par)))
    say("one vb2_errstat_batch_eval, %d workgroups: median %.3f ms (%s)"
        % (grid, med_bat * 1e3, ", ".join("%.3f" % (t * 1e3) for t in t_bat)))
    say("  medians apart by %.3f ms, three times the larger range is %.3f ms: a gain of %.1fx is %s; the results are the same bits"
        % (apart * 1e3, bar * 1e3, med_par / med_bat, "shown" if apart >= bar and med_bat < med_par else "NOT shown"))
    say("  the launch must read %d bytes by section 23's arithmetic (two passes): %.1f us at %.1f TB/s; %d bytes = %.1f us with "
        "the reads staged once; the call took %.1fx the first, %.1fx the second"
        % (traffic_23, traffic_23 / (STEP_TBPS * 1e12) * 1e6, STEP_TBPS, traffic_once, traffic_once / (STEP_TBPS * 1e12) * 1e6,
           med_bat / (traffic_23 / (STEP_TBPS * 1e12)), med_bat / (traffic_once / (STEP_TBPS * 1e12))))
    res = dict(samples=S, markers=M, reads=R, pcs=k, device_bytes=info["device_bytes"], single_sets_device_bytes=single_bytes,
               num_panel=info["num_panel"], grid=grid, parent_ms=[t * 1e3 for t in t_par], batched_ms=[t * 1e3 for t in t_bat],
               parent_ms_median=med_par * 1e3, batched_ms_median=med_bat * 1e3, gain_shown=bool(apart >= bar and med_bat < med_par),
               traffic_bytes_section23=traffic_23, traffic_bytes_staged_once=traffic_once, fits={})
    batch.close()
    for pooled in (False, True):
        vb.errfit_cohort(datas, noms, pooled=pooled, max_iter=2)                 # warm-up
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            fits, pool = vb.errfit_cohort(datas, noms, pooled=pooled)
            walls.append(time.perf_counter() - t0)
        name = "pooled" if pooled else "per sample"
        say("vb2_errfit_cohort_inputs, %s: median %.1f ms (%s); %d iterations, %d E-steps %.1f ms, contexts %.1f ms, searches %.1f ms "
            "(%d likelihood evaluations); summed LRT %.1f; E-step set %d bytes"
            % (name, statistics.median(walls) * 1e3, ", ".join("%.1f" % (t * 1e3) for t in walls), pool["num_iter"], pool["num_estep"],
               pool["seconds_stats"] * 1e3, pool["seconds_context"] * 1e3, pool["seconds_search"] * 1e3, pool["num_step"],
               pool["lrt_sum"], pool["device_bytes"]))
        res["fits"][name] = dict(wall_ms=[t * 1e3 for t in walls], iterations=pool["num_iter"], esteps=pool["num_estep"],
                                 estep_ms=pool["seconds_stats"] * 1e3, context_ms=pool["seconds_context"] * 1e3,
                                 search_ms=pool["seconds_search"] * 1e3, evaluations=pool["num_step"], lrt_sum=pool["lrt_sum"],
                                 freemix_nominal=[n["alpha"] for n in noms], freemix_fit=[f["alpha_fit"] for f in fits])
    done(res)


def stat(a):
    import errfit_cohort_ref as ecr
    import errfit_ref as er
    say, done = _writer(a.out, "pooling_stat")
    qs = list(er.SAMPLE_QUALS)
    res = dict(samples=8, markers=3000, depth=10, shift=5, seed_sets=[])
    say("8 samples of 3 000 x depth 10, alpha 0.03, the rates of q - 5 planted in all; qualities %s; float64 restatement" % qs)
    say("seed set  |fitted - planted| / SE_BINOM, worst over samples and qualities: per sample, pooled   "
        "mean |FREEMIX - 0.03|: nominal, per sample, pooled")
    for base in a.seed_sets:
        seeds = [base + i for i in range(8)]
        made = [er.sample(3000, s, depth=10, shift=5) for s in seeds]
        datas, planted = [m[0] for m in made], made[0][1]
        co = ecr.Cohort(datas)
        noms = co.nominal_estimates()
        pfits, pool = co.pooled_fit(noms)
        own = [co.ev[i].fit(2, True, nominal_est=noms[i])[0] for i in range(8)]
        z_own = max(float(np.max(np.abs(f["err"][qs] - planted[qs]) / np.sqrt(f["err"][qs] * (1 - f["err"][qs]) / f["n"][qs])))
                    for f in own)
        e = pool["err"][qs]
        z_pool = float(np.max(np.abs(e - planted[qs]) / np.sqrt(e * (1 - e) / pool["n"][qs])))
        # the same distances in ONE unit, the pooled SE (a pooled rate's SE is about sqrt(8) smaller than a sample's)
        rel_own = max(float(np.max(np.abs(f["err"][qs] - planted[qs]) / planted[qs])) for f in own)
        rel_pool = float(np.max(np.abs(e - planted[qs]) / planted[qs]))
        fm = lambda x: min(x, 1 - x)
        d_nom = float(np.mean([abs(fm(n["alpha"]) - 0.03) for n in noms]))
        d_own = float(np.mean([abs(f["freemix_fit"] - 0.03) for f in own]))
        d_pool = float(np.mean([abs(f["freemix_fit"] - 0.03) for f in pfits]))
        say("%-8d  %.2f  %.2f   worst relative error of a rate: per sample %.3f, pooled %.3f   %.5f  %.5f  %.5f   (%d pooled "
            "iterations, per sample %s)" % (base, z_own, z_pool, rel_own, rel_pool, d_nom, d_own, d_pool, pool["num_iter"],
                                            [f["num_iter"] for f in own]))
        res["seed_sets"].append(dict(seeds=seeds, z_per_sample=z_own, z_pooled=z_pool, rel_per_sample=rel_own, rel_pooled=rel_pool,
                                     freemix_dist_nominal=d_nom, freemix_dist_per_sample=d_own, freemix_dist_pooled=d_pool,
                                     pooled_iterations=pool["num_iter"], pooled_converged=bool(pool["converged"]),
                                     freemix_nominal=[fm(n["alpha"]) for n in noms], freemix_per_sample=[f["freemix_fit"] for f in own],
                                     freemix_pooled=[f["freemix_fit"] for f in pfits]))
    done(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--pcs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stat", action="store_true")
    ap.add_argument("--seed-sets", type=int, nargs="+", default=[100, 200, 300, 400])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errfit_cohort"))
    a = ap.parse_args()
    (stat if a.stat else device)(a)


if __name__ == "__main__":
    main()
