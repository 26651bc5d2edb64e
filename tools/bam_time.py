"""What a --BamFile load through the built-in reader costs on one MI355X, stage by stage, next to
the text path on the same sample:
  (1) a seeded BAM of --depth reads of --read-len bases over every marker of the panel behind --panel (default: the bundled
      10 000-marker 1000 Genomes panel), written with the test writer (tests/bam_ref.py; 60 000-byte blocks, seeded), and
      its .bai.  --make-only stops here: no device needed.
  (2) vb2_flat_load of it, --reps times after one warm-up: wall clock, and the stage times of vb2_bam_stats -- index (open,
      header, .bai, plan), inflate (inflate + record walk), device (upload, kernels, sort), copy-back (pools + add_site).
  (3) the same sample's .Pileup, written from what (2) loaded, through read_pileup (vb2_flat_load of the text), in
      alternating repetitions on the same box.
Writes JSON and a text table under --out (profiles/bam/).  The load is checked against tests/bam_ref.py's restatement
on a sample of the sites before anything is timed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def make_records(panel, depth, read_len, seed):
    """the seeded sample: (records in file order, bed rows, sequence names)"""
    rows = br.read_bed_rows(panel + ".bed")
    chroms = []
    for c, _, _, _ in rows:
        if c not in chroms:
            chroms.append(c)
    tid_of = {c: i for i, c in enumerate(chroms)}
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for c, p, ref, alt in rows:
        n = int(rng.poisson(depth))
        offs = rng.integers(0, read_len, size=n)
        seqs = letters[rng.integers(0, 4, size=(n, read_len))]
        quals = rng.integers(20, 41, size=(n, read_len)).astype(np.uint8)
        pick = rng.random(n) < 0.5
        for j in range(n):
            off = int(min(offs[j], p - 1))
            seqs[j, off] = ord(ref if pick[j] else alt) if (ref in "ACGT" and alt in "ACGT") else seqs[j, off]
            recs.append(dict(name="r%d" % len(recs), tid=tid_of[c], pos=p - 1 - off, mapq=60, flag=16 if j & 1 else 0,
                             cigar=[("M", read_len)], seq=seqs[j].tobytes().decode(), qual=quals[j].tobytes(), mtid=-1, mpos=-1, tlen=0))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs, rows, chroms


def flat_load(args):
    from verifybamid_amd import _abi
    L = _abi.lib()
    h = C.c_void_p()
    t0 = time.perf_counter()
    _abi.check(L.vb2_flat_load(C.byref(args), C.byref(h)), "vb2_flat_load")
    dt = time.perf_counter() - t0
    st = _abi.BamStats()
    have = L.vb2_flat_bam_stats(h, C.byref(st)) == 0
    L.vb2_flat_free(h)
    return dt, ({n: getattr(st, n) for n, _ in _abi.BamStats._fields_} if have else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panel", default=DEFAULT_PANEL)
    ap.add_argument("--work", required=True, help="directory for sample.bam / sample.Pileup (reused when present)")
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num-pc", type=int, default=2)
    ap.add_argument("--make-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    bam = os.path.join(a.work, "sample.bam")
    t0 = time.perf_counter()
    parsed, rows, chroms = make_records(a.panel, a.depth, a.read_len, a.seed)
    refs = [(c, 1 << 28) for c in chroms]
    if not (os.path.exists(bam) and os.path.exists(bam + ".bai")):
        br.write_indexed_bam(bam, refs, parsed, block_payload=60000)
        say("wrote %s: %d reads, %.1f MB, in %.1f s" % (bam, len(parsed), os.path.getsize(bam) / 1e6, time.perf_counter() - t0))
    if a.make_only:
        return
    import verifybamid_amd as vb
    from verifybamid_amd import _abi
    if _abi.lib().vb2_device_count() < 1:
        raise SystemExit("bam_time.py: no gfx950 device is visible; nothing is timed without one")
    got = vb.api.load_bam(a.panel, bam, num_pc=a.num_pc)            # (also the warm-up)
    # the same values first: a sample of the sites against the restatement of the seeded records
    sample = list(range(0, len(rows), max(1, len(rows) // 40)))
    by_tid = {}
    for r in parsed:
        by_tid.setdefault(r["tid"], []).append(r)
    for i in sample:
        c, p, ref, _ = rows[i]
        tid = [n for n, _ in refs].index(c)
        near = [r for r in by_tid.get(tid, []) if p - 1 - a.read_len <= r["pos"] <= p]
        want = br.pileup_ref(near, refs, [rows[i]])["rows"][0]
        off = got["read_off"]
        have = (got["bases"][off[i]:off[i + 1]].decode(), got["quals"][off[i]:off[i + 1]].decode())
        assert have == want, (rows[i], have, want)
    say("checked %d sites against the restatement: identical" % len(sample))
    pile = os.path.join(a.work, "sample.Pileup")
    with open(pile, "w") as fh:
        off = got["read_off"]
        for i, (c, p, ref, _) in enumerate(rows[:len(off) - 1]):
            n = int(off[i + 1] - off[i])
            if n:
                fh.write("%s\t%d\t%s\t%d\t%s\t%s\n" % (c, p, ref, n, got["bases"][off[i]:off[i + 1]].decode(),
                                                        got["quals"][off[i]:off[i + 1]].decode()))
    args_bam, keep1 = vb.api._run_args(a.panel, None, a.num_pc, True, None, None)
    args_bam.bam_path = bam.encode()
    args_txt, keep2 = vb.api._run_args(a.panel, pile, a.num_pc, True, None, None)
    flat_load(args_txt)                                              # warm-up of the text path
    tb, tt, stats = [], [], []
    for _ in range(a.reps):                                          # alternating
        dt, st = flat_load(args_bam)
        tb.append(dt)
        stats.append(st)
        tt.append(flat_load(args_txt)[0])
    med = lambda v: float(np.median(v))
    stage = {k: med([s[k] for s in stats]) for k in ("seconds_index", "seconds_inflate", "seconds_device", "seconds_copyback")}
    s0 = stats[-1]
    out = dict(markers=len(rows), reads=int(s0["records_seen"]), records_kept=int(s0["records_kept"]), entries=int(s0["entries"]),
               sites=int(s0["sites"]), bam_bytes=os.path.getsize(bam), bytes_inflated=int(s0["bytes_inflated"]),
               blocks=int(s0["blocks"]), chunks=int(s0["chunks"]), batches=int(s0["batches"]), threads=_abi.get_tunable("bam_threads"),
               bam_load_s=tb, text_load_s=tt, bam_load_median_s=med(tb), text_load_median_s=med(tt), stage_median_s=stage,
               pileup_bytes=os.path.getsize(pile), num_bases=got["num_bases"])
    say("%d markers, %d records walked (%d sent up, %d entries, %d sites), BAM %.1f MB (%.1f MB inflated in %d blocks of %d chunks), %d batch(es)"
        % (out["markers"], out["reads"], out["records_kept"], out["entries"], out["sites"], out["bam_bytes"] / 1e6,
           out["bytes_inflated"] / 1e6, out["blocks"], out["chunks"], out["batches"]))
    say("vb2_flat_load from the BAM: %s s (median %.4f); stages (medians): index %.4f, inflate + walk %.4f, device %.4f, copy-back %.4f"
        % (", ".join("%.4f" % t for t in tb), out["bam_load_median_s"], stage["seconds_index"], stage["seconds_inflate"],
           stage["seconds_device"], stage["seconds_copyback"]))
    say("vb2_flat_load from the same sample's .Pileup (%.1f MB): %s s (median %.4f)"
        % (out["pileup_bytes"] / 1e6, ", ".join("%.4f" % t for t in tt), out["text_load_median_s"]))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bam_time.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        with open(os.path.join(a.out, "bam_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
