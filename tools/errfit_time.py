"""What --FitError costs: one vb2_errstat_eval at 100 000 x 30, k = 4, next to the bytes it must read,
and the time the fit adds to a one-sample run at that size.  Medians of five alternating rounds after a warm-up, one
device; raw output to profiles/errfit/errfit_time.{txt,json}.

    python tools/errfit_time.py [--markers 100000] [--depth 30] [--pcs 4] [--out profiles/errfit]
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
import verifybamid_amd as vb  # noqa: E402

STEP_TBPS = 5.0                   # what the cohort step reaches: the yardstick of the floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--pcs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errfit"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    d = vb.synth.make_pileup(a.markers, mean_depth=a.depth, num_pc=a.pcs, alpha_true=0.03, seed=7)
    k = a.pcs
    table = vb.nominal_err_table()
    z = np.zeros(k)
    lines = []

    def say(s):
        print(s)
        lines.append(s)
    with vb.LikelihoodContext(d) as ctx, vb.ErrStat(d) as es:
        nominal = ctx.optimize()
        info = es.info()
        es.eval(table, nominal["pc"], nominal["pc2"], nominal["alpha"])            # warm-up
        vb.errfit(d, nominal)
        t_eval, t_fit, t_search, fits = [], [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            es.eval(table, nominal["pc"], nominal["pc2"], nominal["alpha"])
            t_eval.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.optimize()
            t_search.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            fits.append(vb.errfit(d, nominal))
            t_fit.append(time.perf_counter() - t0)
    R, M = d.num_read, d.num_marker
    traffic = 2 * 2 * R + M * (8 * k + 8 + 8 + 1)          # two passes over bases and qualities; panel row, mean, offset, alt
    floor_us = traffic / (STEP_TBPS * 1e12) * 1e6
    fit = fits[-1]
    res = dict(markers=M, reads=R, pcs=k, device_bytes=info["device_bytes"],
               errstat_eval_us=[t * 1e6 for t in t_eval], errstat_eval_us_median=statistics.median(t_eval) * 1e6,
               traffic_bytes=traffic, floor_us_at_5TBps=floor_us,
               search_ms=[t * 1e3 for t in t_search], search_ms_median=statistics.median(t_search) * 1e3,
               fit_ms=[t * 1e3 for t in t_fit], fit_ms_median=statistics.median(t_fit) * 1e3,
               iterations=fit["num_iter"], converged=fit["converged"], evaluations=fit["num_step"], lrt=fit["lrt"],
               freemix_nominal=nominal["alpha"], freemix_fit=fit["alpha_fit"])
    say("%d markers, %d reads, k = %d; vb2_errstat holds %d bytes" % (M, R, k, info["device_bytes"]))
    say("vb2_errstat_eval (host call, two launches, synchronous): median %.1f us (%s)"
        % (res["errstat_eval_us_median"], ", ".join("%.1f" % t for t in res["errstat_eval_us"])))
    say("  it must read %d bytes: %.1f us at %.1f TB/s" % (traffic, floor_us, STEP_TBPS))
    say("vb2_ctx_optimize_llk on the resident context: median %.2f ms" % res["search_ms_median"])
    say("vb2_errfit_input: median %.1f ms (%s); %d iterations, %d likelihood evaluations, converged %s"
        % (res["fit_ms_median"], ", ".join("%.1f" % t for t in res["fit_ms"]), fit["num_iter"], fit["num_step"], fit["converged"]))
    say("FREEMIX %.5f -> %.5f, LRT %.2f" % (nominal["alpha"], fit["alpha_fit"], fit["lrt"]))
    with open(os.path.join(a.out, "errfit_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "errfit_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
