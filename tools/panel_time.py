"""Wall-clock of the --RefVCF panel builder by stage, on a synthetic GT-only panel (gzip'd VCF).

    python tools/panel_time.py [--markers 100000] [--samples 2504] [--threads 16] [--out DIR]

The synthetic VCF and the panel files go to a temporary directory; panel_time.json / panel_time.txt go to --out
(default profiles/panel).

Stages (vb2_panel_view.seconds): parse (the whole read, with the device work it overlaps), upload, Gram, centring,
eigensolve, projection (device stages event-timed) and write.  Also the Gram kernel's int8 rate against the MI355X
dense int8 peak and the projection's bytes per second against HBM, and a CPU baseline: numpy FP64 G^T G + eigh on
the same matrix (the stand-in for the reference's Eigen path), on --threads BLAS threads.
"""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_INT8_TOPS = 5033.0      # MI355X dense int8 MFMA: twice the dense bf16 rate
HBM_TBS = 8.0                # MI355X HBM3E


def write_gt_vcf(path, M, N, seed):
    """Balding-Nichols panel of three populations, hard calls only, written with numpy bytes (fast)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=M)
    F = 0.1
    freqs = rng.beta((p * (1 - F) / F)[None, :].repeat(3, 0), ((1 - p) * (1 - F) / F)[None, :].repeat(3, 0))
    pop = np.arange(N) % 3
    with gzip.open(path, "wb", compresslevel=1) as f:
        f.write(b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
                "\t".join("S%05d" % j for j in range(N)).encode() + b"\n")
        tab = np.frombuffer(b"0/0\t0/1\t1/1\t", dtype=np.uint8).reshape(3, 4)
        step = 5000
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            G = rng.binomial(2, freqs[pop][:, m0:m1].T)               # (m1-m0) x N
            body = tab[G].reshape(m1 - m0, 4 * N)
            body[:, -1] = ord("\n")
            for i in range(m1 - m0):
                f.write(b"1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % (1000 + 10 * (m0 + i)))
                f.write(body[i].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import verifybamid_amd as vb

    os.makedirs(a.out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="panel_time_")
    vcf = os.path.join(tmp, "panel_%d_%d.vcf.gz" % (a.markers, a.samples))
    t = time.time()
    write_gt_vcf(vcf, a.markers, a.samples, seed=1)
    gen_s = time.time() - t
    size = os.path.getsize(vcf)

    runs = []
    for rep in range(2):                       # the first run also loads rocSOLVER and warms the device
        t = time.time()
        r = vb.build_panel(vcf, output_prefix=vcf, num_svd_pcs=a.pcs, num_thread=a.threads, device=0)
        wall = time.time() - t
        runs.append(dict(wall=wall, seconds=r["seconds"], total=r["seconds_total"]))
    sec = runs[-1]["seconds"]
    M, N, k = a.markers, a.samples, r["num_pc"]
    n_pad = (N + 63) // 64 * 64
    tiles = (n_pad // 64) * (n_pad // 64 + 1) // 2
    chunks = -(-M // 16384)
    gram_ops = 2.0 * tiles * 64 * 64 * chunks * 16384            # operations the lower-tile kernel executes
    gram_ops_useful = 2.0 * N * (N + 1) / 2 * M
    proj_bytes = float(n_pad) * chunks * 16384 * ((k + 15) // 16)  # one pass over the slab per 16 columns
    out = dict(markers=M, samples=N, num_pc=k, vcf_bytes=size, vcf_generate_s=gen_s, reader_threads=a.threads,
               stages_s=sec, build_total_s=runs[-1]["total"], first_run_total_s=runs[0]["total"],
               gram_tops_executed=gram_ops / sec["gram"] / 1e12 if sec["gram"] > 0 else None,
               gram_tops_useful=gram_ops_useful / sec["gram"] / 1e12 if sec["gram"] > 0 else None,
               int8_peak_tops=PEAK_INT8_TOPS,
               project_gbs=proj_bytes / sec["project"] / 1e9 if sec["project"] > 0 else None,
               hbm_tbs=HBM_TBS, parse_mb_per_s=size / sec["parse"] / 1e6)

    if not a.no_cpu:
        os.environ.setdefault("OMP_NUM_THREADS", str(a.threads))
        d = vb.read_vcf(vcf, num_thread=a.threads)
        G = d["genotypes"].astype(np.float64)
        mu = (d["genotypes"].sum(axis=1).astype(np.float32) / np.float32(N)).astype(np.float64)
        t = time.time()
        A = G - mu[:, None]
        S = A.T @ A
        gram_s = time.time() - t
        t = time.time()
        w, U = np.linalg.eigh(S)
        eig_s = time.time() - t
        sig_cpu = np.sqrt(np.maximum(w[::-1], 0))
        out["cpu_baseline"] = dict(threads=a.threads, what="numpy FP64 (G - mu)^T (G - mu) + eigh", gram_s=gram_s,
                                   eigh_s=eig_s, total_s=gram_s + eig_s,
                                   sigma_max_rel_diff=float(np.max(np.abs(sig_cpu[:k] - r["sigma"][:k]) / sig_cpu[:k])))
    lines = ["panel %d markers x %d samples (GT, gz %.1f MB), %d PCs, %d reader threads" % (M, N, size / 1e6, k, a.threads)]
    for st in ("parse", "upload", "gram", "centre", "eigensolve", "project", "write"):
        lines.append("  %-11s %9.3f ms" % (st, sec[st] * 1e3))
    lines.append("  total       %9.3f ms (first run %.3f ms)" % (runs[-1]["total"] * 1e3, runs[0]["total"] * 1e3))
    if out["gram_tops_executed"]:
        lines.append("  Gram: %.1f int8 TOPS executed (%.1f useful, lower triangle) = %.1f %% of %.0f peak" %
                     (out["gram_tops_executed"], out["gram_tops_useful"], 100 * out["gram_tops_executed"] / PEAK_INT8_TOPS,
                      PEAK_INT8_TOPS))
    if out["project_gbs"]:
        lines.append("  projection: %.0f GB/s of slab = %.1f %% of %.1f TB/s HBM" %
                     (out["project_gbs"], 100 * out["project_gbs"] / (HBM_TBS * 1e3), HBM_TBS))
    lines.append("  parse: %.0f MB/s of compressed VCF" % out["parse_mb_per_s"])
    if "cpu_baseline" in out:
        c = out["cpu_baseline"]
        lines.append("  CPU baseline (%d threads): Gram %.3f s + eigh %.3f s = %.3f s" % (c["threads"], c["gram_s"], c["eigh_s"],
                                                                                       c["total_s"]))
    txt = "\n".join(lines)
    print(txt)
    with open(os.path.join(a.out, "panel_time.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, "panel_time.txt"), "w") as f:
        f.write(txt + "\n")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
