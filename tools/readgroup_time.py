"""What --PerReadGroup costs on one MI355X, next to what a user does without it.

The sample is tools/bam_time.py's (the bundled 10 000-marker panel x --depth reads of --read-len bases, seeded), its reads
dealt round-robin to G groups for every G of --groups (default 1, 8, 64).  Per G, after one warm-up and in alternating
repetitions on the same box:
  (1) vb2_flat_load of the BAM (no groups) and vb2_flat_load_groups: wall clock, the host stages (index; inflate + record
      walk, which holds the walk over the auxiliary fields) and the device stages (whole sample: upload, kernels, sort,
      copy-back; groups: second keys, second sort, sites over groups x slots, copy-back) of each;
  (2) run_files of the whole sample with and without per_read_group: the difference is the groups' load and their
      lock-step search; the search alone (contexts + vb2_batch_optimize_llk) is what the groups' seconds_optimize sum to;
  (3) today's way: one BAM per group, written by this script, and one --BamFile run each.
The groups' estimates of (2) and (3) are compared before anything is reported.  Writes JSON and a text table under --out
(profiles/readgroups/)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import bam_ref as br  # noqa: E402
import readgroup_ref as rr  # noqa: E402
from bam_time import DEFAULT_PANEL, make_records  # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panel", default=DEFAULT_PANEL)
    ap.add_argument("--work", required=True, help="directory for the BAMs (reused when present)")
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--groups", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--num-pc", type=int, default=2)
    ap.add_argument("--make-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    t0 = time.perf_counter()
    recs, rows, chroms = make_records(a.panel, a.depth, a.read_len, a.seed)
    refs = [(c, 1 << 28) for c in chroms]
    say("%d reads over %d markers drawn in %.1f s" % (len(recs), len(rows), time.perf_counter() - t0))
    Gs = [int(x) for x in a.groups.split(",")]
    for G in Gs:
        ids = ["rg%02d" % g for g in range(G)]
        whole = os.path.join(a.work, "all_%d.bam" % G)
        if os.path.exists(whole + ".bai") and all(os.path.exists(os.path.join(a.work, "only_%d_%d.bam.bai" % (G, g))) for g in range(G)):
            continue
        t0 = time.perf_counter()
        for i, r in enumerate(recs):
            rr.tag(r, ids[i % G])
        enc = [br.encode_record(r) for r in recs]
        vo, ve, _ = br.write_bam(whole, refs, recs, 60000, rr.rg_header(refs, ids), encoded=enc)
        br.write_bai(whole + ".bai", len(refs), recs, vo, ve)
        for g in range(G):
            one = os.path.join(a.work, "only_%d_%d.bam" % (G, g))
            mine = recs[g::G]
            vo, ve, _ = br.write_bam(one, refs, mine, 60000, rr.rg_header(refs, [ids[g]]), encoded=enc[g::G])
            br.write_bai(one + ".bai", len(refs), mine, vo, ve)
        say("G = %d: wrote %s (%.1f MB) and %d per-group BAMs in %.1f s" % (G, whole, os.path.getsize(whole) / 1e6, G, time.perf_counter() - t0))
    if a.make_only:
        return
    import verifybamid_amd as vb
    from verifybamid_amd import _abi
    if _abi.lib().vb2_device_count() < 1:
        raise SystemExit("readgroup_time.py: no gfx950 device is visible; nothing is timed without one")
    med = lambda v: float(np.median(v))
    result = dict(markers=len(rows), reads=len(recs), depth=a.depth, read_len=a.read_len, reps=a.reps, by_groups={})
    say("%-4s %-26s %9s %9s %9s %9s %9s %9s %9s" % ("G", "what (medians, seconds)", "wall", "index", "inflate", "device", "copyback", "grp dev", "grp copy"))
    for G in Gs:
        whole = os.path.join(a.work, "all_%d.bam" % G)
        kw = dict(num_pc=a.num_pc)
        vb.api.load_bam_groups(a.panel, whole, **kw)                   # warm-up
        vb.api.load_bam(a.panel, whole, **kw)
        plain, grouped = [], []
        for _ in range(a.reps):                                        # alternating
            t0 = time.perf_counter()
            p = vb.api.load_bam(a.panel, whole, **kw)
            plain.append((time.perf_counter() - t0, p["stats"]))
            t0 = time.perf_counter()
            g = vb.api.load_bam_groups(a.panel, whole, **kw)
            grouped.append((time.perf_counter() - t0, g["stats"], g["groups_seconds_device"], g["groups_seconds_copyback"]))
            assert g["bases"] == p["bases"] and g["quals"] == p["quals"] and len(g["groups"]) == G
            assert sum(x["num_bases"] for x in g["groups"]) == p["num_bases"] and g["unassigned"] == 0
        stage = lambda runs, k: med([r[1][k] for r in runs])
        row = dict(
            load=dict(wall=med([r[0] for r in plain]), index=stage(plain, "seconds_index"), inflate=stage(plain, "seconds_inflate"),
                      device=stage(plain, "seconds_device"), copyback=stage(plain, "seconds_copyback")),
            load_groups=dict(wall=med([r[0] for r in grouped]), index=stage(grouped, "seconds_index"),
                             inflate=stage(grouped, "seconds_inflate"), device=stage(grouped, "seconds_device"),
                             copyback=stage(grouped, "seconds_copyback"), groups_device=med([r[2] for r in grouped]),
                             groups_copyback=med([r[3] for r in grouped])))
        for name in ("load", "load_groups"):
            d = row[name]
            say("%-4d %-26s %9.4f %9.4f %9.4f %9.4f %9.4f %9s %9s"
                % (G, "vb2_flat_" + name, d["wall"], d["index"], d["inflate"], d["device"], d["copyback"],
                   "%.4f" % d["groups_device"] if "groups_device" in d else "-", "%.4f" % d["groups_copyback"] if "groups_copyback" in d else "-"))
        # (2) the runs
        out = os.path.join(a.work, "out_%d" % G)
        run_kw = dict(num_pc=a.num_pc, disable_sanity=True, bam_path=whole)
        with_g = vb.run_files(a.panel, None, out, per_read_group=True, **run_kw)      # warm-up, and the estimates
        t_with, t_without, t_search = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            vb.run_files(a.panel, None, out + "_plain", **run_kw)
            t_without.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r = vb.run_files(a.panel, None, out, per_read_group=True, **run_kw)
            t_with.append(time.perf_counter() - t0)
            t_search.append(sum(x["seconds_optimize"] for x in r["read_groups"]))
        # (3) one run per per-group BAM
        t_each, worst = [], 0.0
        for rep in range(a.reps if G <= 8 else 1):                    # (64 runs once)
            t0 = time.perf_counter()
            for g in range(G):
                one = vb.run_files(a.panel, None, out + "_only", num_pc=a.num_pc, disable_sanity=True,
                                   bam_path=os.path.join(a.work, "only_%d_%d.bam" % (G, g)))
                if rep == 0:
                    worst = max(worst, abs(one["alpha"] - with_g["read_groups"][g]["alpha"]))
            t_each.append(time.perf_counter() - t0)
        row.update(run_plain=med(t_without), run_groups=med(t_with), groups_search=med(t_search), run_each_group=med(t_each),
                   max_alpha_difference=worst)
        say("%-4d run without the flag %.4f, with it %.4f (contexts + lock-step search of the groups %.4f); one --BamFile run per "
            "group over %d per-group BAMs %.4f; largest |alpha difference| between the two ways %.1e"
            % (G, row["run_plain"], row["run_groups"], row["groups_search"], G, row["run_each_group"], worst))
        result["by_groups"][str(G)] = row
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "readgroup_time.json"), "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "readgroup_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
