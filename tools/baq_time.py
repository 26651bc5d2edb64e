"""What --ApplyBAQ costs on one MI355X, next to the same load without the switch:
  (1) tools/bam_time.py's seeded sample (--depth reads of --read-len bases over every marker of the bundled 10 000-marker
      panel), but drawn from a seeded genome with --sub substitutions, and that genome as a FASTA with its .fai.  The
      FASTA is a SPARSE file: the sequences have the panel's real lengths, one line each, and only the windows around the
      markers are written (the rest reads as NUL, which the reader takes as N) -- the reader fetches only the spans the
      records can touch.  --make-only stops here: no device needed.
  (2) vb2_flat_load of the BAM with and without the switch, alternating, --reps each after one warm-up of both: wall
      clock, vb2_bam_stats, and with the switch vb2_baq_stats (FASTA read, the kernel per tier, the cap round trip).
  (3) the yardstick of the kernel: the sequential host core of the same header (csrc/baq_core.h through vb2_baq_records,
      where = 0) over the same records, on --threads processes each taking a slice of the markers' .bed.
Writes JSON and a text table under --out (profiles/baq/)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import bam_ref as br  # noqa: E402

DEFAULT_PANEL = os.path.join(ROOT, "tests", "golden", "panels", "1000g.phase3.10k.b37.vcf.gz.dat")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_sample(panel, depth, read_len, sub, seed, out_dir):
    rows = br.read_bed_rows(panel + ".bed")
    chroms = []
    for c, _, _, _ in rows:
        if c not in chroms:
            chroms.append(c)
    tid_of = {c: i for i, c in enumerate(chroms)}
    last = {c: max(p for cc, p, _, _ in rows if cc == c) for c in chroms}
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    pad = 2 * read_len + 32
    windows = {}          # (chrom, start) -> bytes of the genome there
    recs = []
    for c, p, ref, alt in rows:
        w0 = max(0, p - 1 - pad)
        win = letters[rng.integers(0, 4, size=2 * pad)].copy()
        windows[(c, w0)] = win
        n = int(rng.poisson(depth))
        for j in range(n):
            off = int(min(rng.integers(0, read_len), p - 1))
            pos = p - 1 - off
            s = win[pos - w0:pos - w0 + read_len].copy()
            flip = rng.random(read_len) < sub
            s[flip] = letters[rng.integers(0, 4, size=int(flip.sum()))]
            recs.append(dict(name="r%d" % len(recs), tid=tid_of[c], pos=pos, mapq=60, flag=16 if j & 1 else 0, cigar=[("M", read_len)],
                             seq=s.tobytes().decode(), qual=rng.integers(20, 41, size=read_len).astype(np.uint8).tobytes(), mtid=-1,
                             mpos=-1, tlen=0))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    refs = [(c, last[c] + pad + 1) for c in chroms]
    bam = os.path.join(out_dir, "sample.bam")
    br.write_indexed_bam(bam, refs, recs, block_payload=60000)
    fasta = os.path.join(out_dir, "genome.fa")
    off, fai = 0, []
    with open(fasta, "wb") as f:
        for c, n in refs:
            head = (">%s\n" % c).encode()
            f.seek(off)
            f.write(head)
            start = off + len(head)
            fai.append("%s\t%d\t%d\t%d\t%d\n" % (c, n, start, n, n + 1))
            for (cc, w0), win in windows.items():      # (later windows overwrite where two markers' windows overlap: the
                if cc == c:                            # reads of the earlier marker then carry a few more mismatches)
                    f.seek(start + w0)
                    f.write(win[:max(0, min(len(win), n - w0))].tobytes())
            f.seek(start + n)
            f.write(b"\n")
            off = start + n + 1
    open(fasta + ".fai", "w").write("".join(fai))
    return bam, fasta, len(recs)


def host_slice(job):
    import verifybamid_amd as vb
    bam, bed, fasta = job
    t0 = time.time()
    r = vb.api.baq_records(bam, bed, fasta, where=0)
    return time.time() - t0, len(r["mapq"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panel", default=DEFAULT_PANEL)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--sub", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--work", default="/tmp/baq_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baq"))
    ap.add_argument("--make-only", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    t0 = time.time()
    bam, fasta, n = make_sample(a.panel, a.depth, a.read_len, a.sub, a.seed, a.work)
    say("%d records of %d bases, substitution rate %g, BAM %.1f MB, FASTA sparse (%.0f MB apparent); made in %.0f s"
        % (n, a.read_len, a.sub, os.path.getsize(bam) / 1e6, os.path.getsize(fasta) / 1e6, time.time() - t0))
    if a.make_only:
        return
    res = dict(records=n, read_len=a.read_len, depth=a.depth, with_switch=[], without=[], baq=[], bam=[])
    # the yardstick first, before this process touches the device: the sequential host core on --threads fresh processes,
    # each over a slice of the .bed
    rows = open(a.panel + ".bed").read().splitlines()
    jobs = []
    for k in range(a.threads):
        part = rows[k * len(rows) // a.threads:(k + 1) * len(rows) // a.threads]
        bed = os.path.join(a.work, "part%d.bed" % k)
        open(bed, "w").write("\n".join(part) + "\n")
        jobs.append((bam, bed, fasta))
    t = time.time()
    import multiprocessing
    with ProcessPoolExecutor(a.threads, mp_context=multiprocessing.get_context("spawn")) as ex:
        parts = list(ex.map(host_slice, jobs))
    res["host_wall"] = time.time() - t
    res["host_records"] = sum(p[1] for p in parts)
    res["host_slowest"] = max(p[0] for p in parts)
    say("host core, %d processes over slices of the .bed (scan, FASTA and HMM each): wall %.3f s, slowest slice %.3f s, %d records"
        % (a.threads, res["host_wall"], res["host_slowest"], res["host_records"]))
    import verifybamid_amd as vb
    for rep in range(a.reps + 1):
        for on in (False, True):
            t = time.time()
            got = vb.api.load_bam(a.panel, bam, apply_baq=on, reference_path=fasta if on else None)
            dt = time.time() - t
            if rep == 0:
                continue
            res["with_switch" if on else "without"].append(dt)
            if on:
                res["baq"].append(got["baq"])
                res["bam"].append(got["stats"])
    med = lambda v: float(np.median(v))  # noqa: E731
    say("vb2_flat_load without the switch: %s s (median %.4f)" % (", ".join("%.4f" % x for x in res["without"]), med(res["without"])))
    say("vb2_flat_load with --ApplyBAQ:    %s s (median %.4f)" % (", ".join("%.4f" % x for x in res["with_switch"]), med(res["with_switch"])))
    b = res["baq"]
    say("stage (medians): FASTA %.4f s (%d bases), kernel LDS tier %.4f s (%d records), global tier %.4f s (%d records), cap round trip "
        "%.4f s, whole stage %.4f s; realigned %d, dropped by the cap %d, undefined rows %d"
        % (med([x["seconds_fasta"] for x in b]), b[0]["fasta_bytes"], med([x["seconds_lds"] for x in b]), b[0]["records_lds"],
           med([x["seconds_global"] for x in b]), b[0]["records_global"], med([x["seconds_cap"] for x in b]),
           med([x["seconds_stage"] for x in b]), b[0]["realigned"], b[0]["dropped_cap"], b[0]["undefined_rows"]))
    json.dump(res, open(os.path.join(a.out, "baq_time.json"), "w"), indent=1)
    open(os.path.join(a.out, "baq_time.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
