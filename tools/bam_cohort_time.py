"""What a cohort costs when its list names BAMs instead of text pileups, and what the device inflate (tunable bam_inflate;
DESIGN.md section 21) changes, on one MI355X.  The sample is tools/bam_time.py's (10 000 markers x 30, 60 000-byte blocks;
`tools/bam_time.py --work DIR --make-only` writes it without a device):
  (1) a cohort of --samples lines of that BAM with bam_inflate 0, the same with bam_inflate 1, and the same cohort from the
      sample's text pileup: one warm-up each, then --reps alternating repetitions; wall-clock and samples/s;
  (2) a single vb2_flat_load of the BAM under both settings, alternating, with the stage times of the device inflate
      (vb2_bgzf_inflate_stats: upload, kernel, copy-back, staging) beside the reader's own (vb2_bam_stats);
  (3) --inflate-only: nothing but one vb2_bgzf_inflate of the whole file -- the process to put under
      `rocprofv3 --kernel-trace --stats` for the kernel's own time.
Writes JSON and a text table under --out (profiles/bam_cohort/).  Reported, nothing asserted -- except that the three
cohorts give the same estimates."""
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

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def main():
    import bam_time
    ap = argparse.ArgumentParser()
    ap.add_argument("--panel", default=bam_time.DEFAULT_PANEL)
    ap.add_argument("--work", required=True, help="directory with sample.bam / sample.bam.bai (tools/bam_time.py --make-only)")
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--num-pc", type=int, default=2)
    ap.add_argument("--threads", type=int, default=0, help="reader threads of the cohort (0: the library's default)")
    ap.add_argument("--inflate-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import verifybamid_amd as vb
    from verifybamid_amd import _abi
    if _abi.lib().vb2_device_count() < 1:
        raise SystemExit("bam_cohort_time.py: no gfx950 device is visible; nothing is timed without one")
    bam = os.path.join(a.work, "sample.bam")
    if a.inflate_only:
        data = open(bam, "rb").read()
        vb.api.bgzf_inflate(bam_time.br.BGZF_EOF)                     # warm-up: the runtime and the code object
        vb.api.bgzf_inflate_stats(reset=True)
        out, st = vb.api.bgzf_inflate(data)
        s = vb.api.bgzf_inflate_stats()
        say("vb2_bgzf_inflate of %s: %d blocks (%d refused), %.1f MB -> %.1f MB; kernel %.3f ms (%.1f us per block, %.2f GB/s inflated), "
            "upload %.3f ms, copy-back %.3f ms" % (bam, len(st), int((st != 0).sum()), len(data) / 1e6, len(out) / 1e6, 1e3 * s["seconds_kernel"],
                                                    1e6 * s["seconds_kernel"] / max(len(st), 1), len(out) / 1e9 / max(s["seconds_kernel"], 1e-12),
                                                    1e3 * s["seconds_upload"], 1e3 * s["seconds_copyback"]))
        return
    pile = os.path.join(a.work, "sample.Pileup")
    got = vb.api.load_bam(a.panel, bam, num_pc=a.num_pc)
    rows = bam_time.br.read_bed_rows(a.panel + ".bed")
    with open(pile, "w") as fh:
        off = got["read_off"]
        for i, (c, p, ref, _) in enumerate(rows[:len(off) - 1]):
            n = int(off[i + 1] - off[i])
            if n:
                fh.write("%s\t%d\t%s\t%d\t%s\t%s\n" % (c, p, ref, n, got["bases"][off[i]:off[i + 1]].decode(), got["quals"][off[i]:off[i + 1]].decode()))

    def cohort(paths, inflate):
        _abi.set_tunable("bam_inflate", inflate)
        t0 = time.perf_counter()
        res = vb.run_cohort_files(a.panel, paths, None, num_pc=a.num_pc, disable_sanity=True, num_host_thread=a.threads)
        dt = time.perf_counter() - t0
        assert all(r["status"] == 0 for r in res), [r["status"] for r in res]
        return dt, res

    configs = [("bam_host", [bam] * a.samples, 0), ("bam_device", [bam] * a.samples, 1), ("text", [pile] * a.samples, 0)]
    first = {}
    for name, paths, inflate in configs:                              # one warm-up of each
        first[name] = cohort(paths, inflate)[1][0]
    for name in ("bam_device", "text"):
        assert first[name]["alpha"] == first["bam_host"]["alpha"] and first[name]["llk1"] == first["bam_host"]["llk1"], name
    times = {name: [] for name, _, _ in configs}
    vb.api.bgzf_inflate_stats(reset=True)
    for _ in range(a.reps):                                           # alternating
        for name, paths, inflate in configs:
            times[name].append(cohort(paths, inflate)[0])
    cohort_dev = vb.api.bgzf_inflate_stats(reset=True)
    for name, _, _ in configs:
        t = times[name]
        say("cohort of %d x %-10s: %s s  -> %s samples/s (range %.1f .. %.1f)" % (a.samples, name, ", ".join("%.3f" % x for x in t),
            ", ".join("%.1f" % (a.samples / x) for x in t), a.samples / max(t), a.samples / min(t)))
    # ---- one load, both settings ----
    single = {0: [], 1: []}
    stats = {0: [], 1: []}
    dev = []
    for _ in range(a.reps + 1):                                       # (the first of each is the warm-up)
        for inflate in (0, 1):
            _abi.set_tunable("bam_inflate", inflate)
            vb.api.bgzf_inflate_stats(reset=True)
            t0 = time.perf_counter()
            g = vb.api.load_bam(a.panel, bam, num_pc=a.num_pc)
            single[inflate].append(time.perf_counter() - t0)
            stats[inflate].append(g["stats"])
            if inflate:
                dev.append(vb.api.bgzf_inflate_stats(reset=True))
    _abi.set_tunable("bam_inflate", 0)
    med = lambda v: float(np.median(v))
    for inflate in (0, 1):
        s = stats[inflate][1:]
        say("vb2_flat_load, bam_inflate %d: %s s (median %.4f); reader's stages (medians): index %.4f, inflate + walk %.4f, device %.4f, copy-back %.4f"
            % (inflate, ", ".join("%.4f" % t for t in single[inflate][1:]), med(single[inflate][1:]), med([x["seconds_index"] for x in s]),
               med([x["seconds_inflate"] for x in s]), med([x["seconds_device"] for x in s]), med([x["seconds_copyback"] for x in s])))
    d = dev[1:]
    say("device inflate of one load (medians): %d blocks in %d batch(es), %d refused, %.1f MB -> %.1f MB: upload %.3f ms, kernel %.3f ms "
        "(%.1f us per block, %.2f GB/s inflated), copy-back %.3f ms, out of the staging buffer %.3f ms"
        % (d[-1]["blocks"], d[-1]["batches"], d[-1]["refused"], d[-1]["bytes_raw"] / 1e6, d[-1]["bytes_inflated"] / 1e6,
           1e3 * med([x["seconds_upload"] for x in d]), 1e3 * med([x["seconds_kernel"] for x in d]),
           1e6 * med([x["seconds_kernel"] for x in d]) / max(d[-1]["blocks"], 1),
           d[-1]["bytes_inflated"] / 1e9 / max(med([x["seconds_kernel"] for x in d]), 1e-12),
           1e3 * med([x["seconds_copyback"] for x in d]), 1e3 * med([x["seconds_stage"] for x in d])))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        out = dict(samples=a.samples, reps=a.reps, threads=a.threads, cohort_s=times, cohort_device_inflate=cohort_dev,
                   single_load_s={str(k): v[1:] for k, v in single.items()}, single_load_stats={str(k): v[1:] for k, v in stats.items()},
                   single_load_device_inflate=d, bam_bytes=os.path.getsize(bam), pileup_bytes=os.path.getsize(pile))
        with open(os.path.join(a.out, "bam_cohort_time.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "bam_cohort_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
