#!/usr/bin/env python
"""bench.py -- LLK evaluations per second on the BASELINE.json workload.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1 runs one process per GPU over RCCL.  Started under `python -m torch.distributed.run
--nproc-per-node N ... bench.py --gpus N` the ranks come from the environment; started plainly
(`python bench.py --gpus N`) the script spawns the N ranks itself on 127.0.0.1.

Workload (config.workload): synthetic pileup of 100 000 markers x depth 30, --NumPC 4
(BASELINE.json configs[2], the shape the metric is quoted on), resident in HBM before the
timed region.  One STEP = one pass of the hot path over that pileup for a batch of `--batch`
parameter points (default 48, the most one launch carries): one `vb2_llk_eval_batch_device`
call = one launch of the dominant kernel (llk_eval_kernel<2,true>: 8 points per group, 6
groups).  One "eval" = one (pc1, pc2, alpha) point = one call of the reference's
ComputeMixLLKs.

N > 1, `--mode sample` (default): every rank owns a different sample of the same shape
(sample-parallel, BASELINE.json configs[4]); no data-path collective, weak scaling; `value` is
the whole-job rate.  The JSON also carries `marker_sharded`: ONE sample's markers sharded over
the N ranks by the library's own C++ group (vb2_shard_group_create_rank: launch +
ncclAllReduce of the batch's partial LLKs per step, BASELINE.json configs[3]) -- its evals/s
and its OptimizeLLK wall-clock.  `--mode marker` makes that the primary metric (strong scaling).

Prints ONE JSON line on rank 0.  A plain run does only what that line's headline needs: set up,
warm up, time the K steps (`ms_per_step` = wall-clock of one), write the outputs if asked, print.
`--dump-outputs DIR` writes what the last timed step computed -- the batch's LLKs, the array a
caller of the launch receives -- as DIR/llk.npy (float64; rank 0's sample).  The inputs are seeded:
the same arguments give the same inputs on every run and every build.

`--full` adds everything else the line has carried: the roofline (with the issue ceiling measured
on the device), the marker-sharded leg, search_point, create_ms, the wide and mid quality
alphabets, OptimizeLLK, the cohort legs, the parity probe against the oracle and the CPU baseline.
The oracle (oracle/) is used only as the checker of that parity probe and as the cpu_baseline leg;
it is never the thing timed as `value`.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 achievable
FP64_VALU_NOTE = ("FP64 vector peak 78.6 TFLOP/s = 16 FMA lanes/clk/SIMD: a wave64 FP64 instruction "
                  "occupies its SIMD for 4 cycles")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prewarm-ms", type=float, default=100.0,
                    help="keep the GPU busy this long before the warmup steps: an idle MI355X needs ~40 ms of "
                         "load to reach its sustained clocks (tools/warm_curve.py: 113 -> 87 us per launch)")
    ap.add_argument("--batch", type=int, default=48, help="parameter points per step (one launch carries up to 48)")
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--num-pc", type=int, default=4)
    ap.add_argument("--q-lo", type=int, default=20, help="base qualities of the synthetic reads: uniform in q-lo..q-hi "
                    "(SURVEY 8d: 20..40; 2..60 = the BAQ-like alphabet of roofline_wide_alphabet, for its profile passes)")
    ap.add_argument("--q-hi", type=int, default=40)
    ap.add_argument("--mode", choices=["sample", "marker"], default="sample")
    ap.add_argument("--cohort-samples", type=int, default=32, help="samples of the single-GPU cohort leg (0 = skip)")
    ap.add_argument("--cohort-files", type=int, default=256,
                    help="samples of the cohort-from-text-files leg (BASELINE configs[4] per GPU; 0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="also the legs beyond the headline: roofline, marker_sharded, search_point, create_ms, quality "
                         "alphabets, optimize, cohort, parity probe, cpu_baseline (the --no-* options trim these)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the LLKs the last timed step computed to DIR/llk.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-optimize", action="store_true")
    ap.add_argument("--soft-exit", action="store_true",
                    help="(the default: the run leaves through the interpreter's normal exit, where profilers and exit "
                         "handlers see the process whole; kept for existing command lines)")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip search_point / cohort / marker_sharded legs (profiling runs)")
    return ap.parse_args()


def self_spawn(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks here (one per GPU)."""
    import ctypes
    try:        # fail fast (and cheaply: no torch import) when the box has fewer GPUs than ranks
        lib = ctypes.CDLL(os.path.join(ROOT, "verifybamid_amd", "libvb2.so"))
        have = lib.vb2_device_count()
    except OSError:
        have = -1
    if 0 <= have < n and os.environ.get("VB2_BENCH_SHARE_GPU", "") != "1":
        raise SystemExit("bench.py --gpus %d: only %d gfx950 device(s) visible" % (n, have))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    # a rank that dies must not leave the others waiting in a rendezvous
    rcs = [None] * n
    while any(rc is None for rc in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
        if any(rc not in (None, 0) for rc in rcs):
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.05)
    for p in procs:
        p.wait()
    sys.exit(max(abs(p.returncode) for p in procs))


def cpus_allowed():
    """CPUs this process may use: affinity, capped by the cgroup's CFS quota (what the library sizes its reader threads by)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, round(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    return n


def latest_profile(name):
    pdir = os.path.join(ROOT, "profiles")
    if not os.path.isdir(pdir):
        return None, None
    for rnd in sorted(os.listdir(pdir), reverse=True):
        f = os.path.join(pdir, rnd, name)
        if os.path.exists(f):
            return json.load(open(f)), os.path.relpath(f, ROOT)
    return None, None


ROOFLINE = {}        # what the later legs need of the headline's roofline (ceiling, instruction count, per-point time)


def timed_launches(ctx, pts, out, B, stream, steps, torch):
    for _ in range(100):
        ctx.llk_device(pts.data_ptr(), out.data_ptr(), B, stream.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        ctx.llk_device(pts.data_ptr(), out.data_ptr(), B, stream.cuda_stream)
    e1.record(stream)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / steps          # us per launch


_REAL_STDOUT = None


def emit(result):
    """The JSON line, on the process's real stdout (see main)."""
    data = (json.dumps(result) + "\n").encode()
    fd = _REAL_STDOUT if _REAL_STDOUT is not None else 1
    while data:
        data = data[os.write(fd, data):]


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_spawn(args.gpus)

    # stdout carries ONE line, the JSON: whatever native libraries print there on the way (librccl's version banner at
    # communicator creation, ...) goes to stderr -- file descriptor 1 points at stderr until emit() writes the line
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch
    import verifybamid_amd as vb

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (no CPU fallback)")
    # VB2_BENCH_SHARE_GPU=1 (plumbing check on a one-GPU box, never a measurement): every rank uses
    # device 0, the ranks talk over gloo, and the RCCL leg is skipped
    share_gpu = os.environ.get("VB2_BENCH_SHARE_GPU", "") == "1"
    if share_gpu:
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("rank %d has no GPU: %d visible" % (local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dist = None
    red_dev = "cpu" if share_gpu else "cuda"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        if share_gpu:
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank),
                                    timeout=datetime.timedelta(seconds=120))

    k, B = args.num_pc, args.batch
    # ---- inputs (synthetic, seeded), flattened into HBM before timing ----
    qkw = dict(q_lo=args.q_lo, q_hi=args.q_hi)
    shared = vb.synth.make_pileup(args.markers, args.depth, k, alpha_true=0.05, seed=2, **qkw)   # the sample every rank knows
    if args.mode == "sample":
        data = shared if rank == 0 else vb.synth.make_pileup(args.markers, args.depth, k, alpha_true=0.05,
                                                             seed=2 + rank, **qkw)
    else:
        data = shared
    # an explicit (non-null) stream: the kernels and the HIP events all go on it, so the events
    # bracket exactly the timed launches
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rng = np.random.default_rng(123)
    stride = 2 * k + 1
    pts_h = np.concatenate([rng.normal(0, 0.03, size=(B, 2 * k)), rng.uniform(0.01, 0.3, size=(B, 1))], axis=1)
    pc1_h, pc2_h, al_h = (np.ascontiguousarray(pts_h[:, :k]), np.ascontiguousarray(pts_h[:, k:2 * k]),
                          np.ascontiguousarray(pts_h[:, 2 * k]))
    pts = torch.tensor(pts_h, dtype=torch.float64, device="cuda")
    out = torch.zeros(B, dtype=torch.float64, device="cuda")

    group = None
    uid = None
    if share_gpu and args.mode == "marker":
        raise SystemExit("VB2_BENCH_SHARE_GPU=1 cannot run --mode marker (RCCL needs one device per rank)")
    uid_error = None
    if (world > 1 or not args.no_extras) and (args.full or args.mode == "marker") and not share_gpu:
        # the library's own marker-shard group (C++: contexts + ncclAllReduce bound from librccl)
        box = [None, None]
        if rank == 0:
            try:
                box[0] = vb.ShardGroup.unique_id()
            except Exception as exc:                 # noqa: BLE001 -- (e.g. librccl not loadable) reported, not fatal
                box[1] = "%s: %s" % (type(exc).__name__, exc)
        if dist is not None:
            dist.broadcast_object_list(box, src=0)
        uid, uid_error = box[0], box[1]
        if uid_error and args.mode == "marker":
            raise SystemExit(uid_error)
    if args.mode == "marker":
        group = vb.ShardGroup(shared, device=local_rank, rank=rank, nranks=world, unique_id=uid)
        ctx, info = None, None
        llk_host = np.zeros(B)

        def step():
            llk_host[:] = group.llk(pc1_h, pc2_h, al_h)       # launch + ncclAllReduce + sync, every rank
    else:
        ctx = vb.LikelihoodContext(data, device=local_rank, stream=stream.cuda_stream)
        info = ctx.info()

        def step():
            ctx.llk_device(pts.data_ptr(), out.data_ptr(), B, stream.cuda_stream)

    # untimed: bring the clocks up (same work as a step), then the W warmup steps
    t_pw = time.perf_counter()
    while 1e3 * (time.perf_counter() - t_pw) < args.prewarm_ms:
        for _ in range(50):
            step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.steps):
        step()
    ev1.record(stream)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    if dist is not None:
        t = torch.tensor([wall, dev_ms], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, dev_ms = float(t[0]), float(t[1])

    evals_per_step = B * (world if args.mode == "sample" else 1)
    value = evals_per_step * args.steps / wall
    llk_dev = llk_host.copy() if args.mode == "marker" else out.cpu().numpy().copy()
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "llk.npy"), np.asarray(llk_dev, dtype=np.float64))

    if info is None:
        info = dict(num_read=shared.num_read, num_active_marker=shared.num_marker, num_code=-1, arch="gfx950",
                    algorithmic_bytes_per_eval=2 * shared.num_read + shared.num_marker * (8 * k + 12))
    result = {
        "metric": "llk_evals_per_sec", "value": value, "unit": "evals/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * wall / args.steps,
        "higher_is_better": True, "scaling": "weak" if args.mode == "sample" else "strong",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {
            "workload": "synthetic pileup %d markers x depth %g, --NumPC %d (BASELINE.json configs[2] shape)%s"
                        % (args.markers, args.depth, k,
                           "" if (args.q_lo, args.q_hi) == (20, 40) else ", base qualities %d..%d" % (args.q_lo, args.q_hi)),
            "batch_points_per_step": B, "prewarm_ms": args.prewarm_ms,
            "parallelism": ("1 GPU" if world == 1 else
                            ("sample-parallel x%d (one sample per GPU, no collective)" % world
                             if args.mode == "sample" else
                             "marker-sharded x%d + ncclAllReduce of %d doubles per step (libvb2 vb2_shard_group)"
                             % (world, B))),
            "rccl_world_size": (dist.get_world_size() if dist is not None else 1),
            "shared_gpu_plumbing_check": share_gpu,
            "launched_by": "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else
                           ("self-spawned ranks" if world > 1 else "single process"),
            "reads": int(info["num_read"]), "active_markers": int(info["num_active_marker"]),
            "distinct_codes": int(info["num_code"]), "device": info["arch"],
        },
    }

    if rank == 0 and args.mode == "sample" and args.full:
        # ---- roofline of the dominant kernel: frac = t_ideal / t_measured, t_ideal = the LONGEST of the three
        # times the launch would take if one resource alone ran at its peak --
        #   lds : bytes the read loops gather from the LDS tables (48 B per step and point: vb2_info.num_step, computed by the
        #         library for THIS context; + the projection's coefficient reads) / 157.3 TB/s (256 B/clk/CU x 256 CUs x 2.4 GHz)
        #   fp64: FP64 vector flops of the launch (instruction classes counted by the committed PMC pass) / 78.6 TFLOP/s
        #   hbm : HBM-side bytes of the launch (FETCH_SIZE x 2 + WRITE_SIZE of the committed PMC pass) / 8 TB/s
        # `bound` names the longest.  The fraction rises when the launch gets shorter for the same work and when work is
        # taken out of the BINDING term only if another term then binds -- it cannot fall because an idle unit got idler.
        # PMC-derived inputs carry the hash of the kernel sources they were measured on (tools/update_profiles.py): a figure
        # of another hash is dropped (its term is null, `stale_profile` says so) instead of pricing the old kernel.
        from verifybamid_amd import _abi as abi_
        khash = abi_.kernel_source_hash()
        stale = []

        def fresh(name):
            pj, psrc = latest_profile(name)
            if not pj or pj.get("markers") != args.markers or pj.get("num_pc") != k or pj.get("batch", B) != B:
                return None, None
            if pj.get("kernel_src_hash") != khash:
                stale.append(psrc)
                return None, psrc
            return pj, psrc

        bytes_per_launch = info["algorithmic_bytes_per_eval"] * B
        step_us = 1e3 * dev_ms / args.steps
        t_meas = step_us * 1e-6
        achieved = bytes_per_launch / t_meas / 1e9
        tj, traffic_src = fresh("traffic_b%d.json" % B)
        traffic = tj["traffic_bytes_per_launch"] if tj else None
        vj, vsrc = fresh("valu_b%d.json" % B)
        valu = None
        if vj:
            valu = {"busy_frac": vj["valu_busy_frac"],
                    "lane_instr_per_marker_point": vj["lane_instr_per_marker_point"],
                    "lds_busy_frac": vj.get("lds_busy_frac"),
                    "lds_bank_conflict_frac": (vj["SQ_LDS_BANK_CONFLICT"] / vj["SQ_LDS_IDX_ACTIVE"]) if vj.get("SQ_LDS_IDX_ACTIVE") else None,
                    "source": vsrc, "note": FP64_VALU_NOTE}
        import ctypes
        ceil3 = (ctypes.c_double * 3)()
        lib_ = abi_.lib()
        lib_.vb2_debug_issue_ceiling.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        lib_.vb2_debug_issue_ceiling.restype = ctypes.c_int
        ceiling = None
        if lib_.vb2_debug_issue_ceiling(local_rank, ceil3) == 0 and ceil3[2] > 0:
            ceiling = {"fp64_fma_alone": ceil3[0], "fp64_fma_fed_by_table_reads": ceil3[1],
                       "valu_with_table_reads": ceil3[2], "unit": "lane-instructions/s",
                       "nominal_at_2.4GHz": 1024 * 16 * 2.4e9,
                       "source": "measured on this device after the timed region: vb2_debug_issue_ceiling "
                                 "(verifybamid_amd/csrc/calib_kernels.hip; stand-alone: tools/ubench/lds_fma_mix.hip)"}
        ROOFLINE["ceiling"] = ceiling
        valu_issue_frac = None
        if valu and ceiling:
            valu_issue_frac = (valu["lane_instr_per_marker_point"] * info["num_active_marker"] * B / t_meas) / ceiling["fp64_fma_alone"]
        fj, fsrc = fresh("flops_b%d.json" % B)
        LDS_PEAK = 256.0 * 256 * 2.4e9          # B/s: ds_read_b128 moves 256 B per clock and CU (MI355X_MICROARCH.md, LDS)
        FP64_PEAK = 78.6e12
        lds_bytes = (48.0 * info["num_step"] + 16.0 * k * info["num_active_marker"]) * B
        terms = {"lds": {"bytes_per_launch": lds_bytes, "peak_TBps": LDS_PEAK / 1e12, "t_us": 1e6 * lds_bytes / LDS_PEAK,
                         "steps_per_marker": info["num_step"] / max(1, info["num_active_marker"]), "table_rows": int(info["num_table_row"]),
                         "note": "the floor of THIS context's layout: a dictionary that needs fewer steps lowers t_ideal and the launch "
                                 "time together (DESIGN.md section 7) -- compare throughput across layouts, frac within one",
                         "source": "vb2_info.num_step x 48 B (one table row per step and point) + 16 B x --NumPC per marker and "
                                   "point (the projection's coefficients), x points; peak = 256 B/clk/CU x 256 CUs x 2.4 GHz"},
                 "fp64": None, "hbm": None}
        if fj:
            fl_ = float(fj["fp64_flops_per_launch"])
            terms["fp64"] = {"flops_per_launch": fl_, "peak_TFLOPs": FP64_PEAK / 1e12, "t_us": 1e6 * fl_ / FP64_PEAK,
                             "fp64_flops_per_marker_point": fj["fp64_flops_per_marker_point"],
                             "fp64_instr_per_marker_point": fj["fp64_instr_per_marker_point"], "source": fsrc,
                             "achieved_TFLOPs": fl_ / t_meas / 1e12, "frac_of_peak": fl_ / t_meas / FP64_PEAK}
        if traffic:
            terms["hbm"] = {"bytes_per_launch": traffic, "peak_TBps": HBM_PEAK_GBPS / 1e3,
                            "t_us": 1e6 * traffic / (HBM_PEAK_GBPS * 1e9), "source": traffic_src}
        have = {n: t["t_us"] for n, t in terms.items() if t}
        bound = max(have, key=have.get)
        t_ideal_us = have[bound]
        frac = t_ideal_us / step_us
        ROOFLINE["frac_headline"] = frac
        ROOFLINE["us_per_point_headline"] = step_us / B
        result["config"]["layout"] = ("probability domain (%d table rows)" % info["num_table_row"]) if info.get("layout") else "run words"
        result["roofline"] = {
            "bound": bound, "frac": frac, "t_ideal_us": t_ideal_us, "t_measured_us": step_us, "terms": terms,
            "achieved": {"lds": lds_bytes / t_meas / 1e12, "unit": "TB/s gathered from LDS"}["lds"] if bound == "lds" else
                        (terms["fp64"]["achieved_TFLOPs"] if bound == "fp64" else traffic / t_meas / 1e12),
            "peak": LDS_PEAK / 1e12 if bound == "lds" else (FP64_PEAK / 1e12 if bound == "fp64" else HBM_PEAK_GBPS / 1e3),
            "unit": "TB/s" if bound != "fp64" else "TFLOP/s",
            "stale_profile": stale or None, "kernel_src_hash": khash,
            "valu_issue_frac": valu_issue_frac, "ceiling": ceiling,
            "nominal": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": achieved / HBM_PEAK_GBPS,
                        "note": "SURVEY 8d: algorithmic bytes per evaluation x points / time / 8 TB/s.  Passes 1 by construction: "
                                "the 48 points of a launch are served by one L2/LDS-resident copy of the pileup -- the HBM "
                                "side moves `traffic` bytes per launch (`hbm_actual_GBps`)"},
            "traffic": traffic, "traffic_source": traffic_src,
            "hbm_actual_GBps": (traffic / t_meas / 1e9) if traffic else None,
            "valu": valu, "fp64": terms["fp64"], "mfma_util": 0.0,
            "mfma_note": "no MFMA instruction on the path: FP64 MFMA and FP64 VALU share the unit on gfx950 "
                         "(profiles/r01/ubench_mfma_overlap.txt), and the UD x PC projection is 2k FMAs per marker",
            "kernel": ("llk_eval_split_kernel" if (info.get("layout") and B > 16) else "llk_eval_kernel<%d,...>" % (2 if B > 4 else 3)),
            "launches_per_step": (B + 47) // 48,
            "algorithmic_bytes_per_launch": int(bytes_per_launch),
            "device_us_per_launch": step_us,
            "note": "device time = HIP events on the launch stream over the timed region / steps",
        }
    # ---- the other multi-GPU mode as a sub-object: one sample's markers over all ranks ----
    # Guarded: whatever happens in here (librccl missing, a communicator that does not come up, a
    # rank that dies and leaves the others in a collective) must not cost the run its main line --
    # an exception is recorded, and a watchdog prints what there is and ends every rank after 4 minutes.
    if args.full and args.mode == "sample" and not args.no_extras and not share_gpu:
        import threading

        def bail():
            result["marker_sharded"] = {"error": "the marker-sharded leg did not finish within 240 s"}
            if rank == 0:
                import ctypes
                ctypes.CDLL(None).fflush(None)
                emit(result)
            os._exit(0)
        watchdog = threading.Timer(240.0, bail)
        watchdog.daemon = True
        watchdog.start()
        try:
            if uid_error:
                raise RuntimeError(uid_error)
            g2 = vb.ShardGroup(shared, device=local_rank, rank=rank, nranks=world, unique_id=uid)
            step_sh, got_sh = g2.prepared_llk(pc1_h, pc2_h, al_h)          # (marshalling done once)
            for _ in range(20):
                step_sh()
            if dist is not None:
                dist.barrier()
            n2 = 200
            t1 = time.perf_counter()
            for _ in range(n2):
                step_sh()
            dt = time.perf_counter() - t1
            # the same through ONE call of NCH x B points: the library queues the NCH launches back to back and
            # reduces all their sums in ONE all-reduce (what multi-start / batched restarts hand over), so the
            # launch, collective and host hand-off latencies are paid once per call instead of once per B points
            NCH = 5
            step_pl, got_pl = g2.prepared_llk(np.tile(pc1_h, (NCH, 1)), np.tile(pc2_h, (NCH, 1)), np.tile(al_h, NCH))
            for _ in range(5):
                step_pl()
            if dist is not None:
                dist.barrier()
            n2p = 50
            t1 = time.perf_counter()
            for _ in range(n2p):
                step_pl()
            dtp = time.perf_counter() - t1
            # (one rank: bit for bit; several: the collective may add a 240-element and a 48-element buffer in different orders)
            if not (np.array_equal(got_pl[:B], got_sh) if world == 1 else
                    np.allclose(got_pl[:B], got_sh, rtol=1e-12, atol=0.0)):
                raise RuntimeError("marker-sharded: the %d-point call and the %d-point call disagree" % (NCH * B, B))
            g2.optimize()
            t_opt = []
            for _ in range(3):
                if dist is not None:
                    dist.barrier()
                t1 = time.perf_counter()
                est_sh = g2.optimize()
                t_opt.append(time.perf_counter() - t1)
            gi = g2.info()
            vals = torch.tensor([dt, min(t_opt), dtp], dtype=torch.float64, device="cuda")
            if dist is not None:
                dist.all_reduce(vals, op=dist.ReduceOp.MAX)
            result["marker_sharded"] = {
                "what": "ONE sample's markers sharded over the %d rank(s) by libvb2 (vb2_shard_group_create_rank): per "
                        "step a launch per rank + one ncclAllReduce of %d doubles + host sync; strong scaling, "
                        "latency-bound" % (world, B),
                "evals_per_s": B * n2 / float(vals[0]), "ms_per_step": 1e3 * float(vals[0]) / n2,
                "pipelined": {"points_per_call": NCH * B, "launches_per_call": NCH, "allreduces_per_call": 1,
                              "evals_per_s": NCH * B * n2p / float(vals[2]),
                              "ms_per_%d_points" % B: 1e3 * float(vals[2]) / (n2p * NCH)},
                "optimize_wall_ms": 1e3 * float(vals[1]), "alpha": est_sh["alpha"], "num_eval": est_sh["num_eval"],
                "uses_rccl": gi["uses_rccl"], "allreduces": gi["num_allreduce"],
                "shard_reads_rank0": gi["num_read"],
                #  what to hold a measured multi-GPU line against -- a PREDICTION, not a measurement: a rank's
                # launch over markers / N (13 us fixed + 0.38 us per 1 000 markers: the 10 000- and 100 000-marker launches of
                # profiles/r06) + the step's fixed part measured here at one rank (launch, all-reduce, publish, host wait:
                # ms_per_step - the plain launch) + ~1.5 us per doubling for the ring.  Strong scaling of a ~50 us step is
                # latency-bound: near-linear scaling is the sample-parallel mode's (config.parallelism), not this one's.
                "predicted_us_per_step_by_ranks": {
                    str(nr): round(13.0 + 0.38 * (args.markers / 1000.0) / nr +
                                   max(0.0, 1e6 * float(vals[0]) / n2 - (13.0 + 0.38 * args.markers / 1000.0)) * (1 if world == 1 else 0) +
                                   1.5 * (nr.bit_length() - 1), 1) for nr in (1, 2, 4, 8)} if world == 1 else None,
            }
            g2.close()
        except Exception as exc:                     # noqa: BLE001 -- recorded, not fatal
            result["marker_sharded"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        watchdog.cancel()

    if rank == 0 and args.mode == "sample" and args.full:
        if world == 1 and not args.no_extras:
            # the operating points of the actual search: a 4-point launch (one Nelder-Mead
            # iteration: R, E, C_A, C_R) and a single point
            sp = {}
            for nb in (4, 1):
                us = timed_launches(ctx, pts, out, nb, stream, 1500, torch)
                # frac: against the ceiling that binds -- the time these points take at the headline launch's rate per point,
                # scaled by the headline's own fraction of the measured issue ceiling; nominal_frac: SURVEY 8d bytes / 8 TB/s
                vf = ROOFLINE.get("frac_headline")
                sp["points_%d" % nb] = {"device_us_per_launch": us, "evals_per_s": nb / us * 1e6,
                                        "frac": (vf * ROOFLINE["us_per_point_headline"] * nb / us) if vf else None,
                                        "us_at_headline_rate": ROOFLINE["us_per_point_headline"] * nb,
                                        "nominal_frac": info["algorithmic_bytes_per_eval"] * nb / (us * 1e-6) / 1e9 / HBM_PEAK_GBPS}
            result["search_point"] = sp
            # the unfavourable quality alphabets (VERDICT r3 missing #3, r4 weak #3): the same sample shape with BAQ-like
            # qualities 2..60 -- what BAM-derived pileups look like (the reference's own pileup applies BAQ and a
            # min-BQ of 13: SimplePileupViewer.cpp:457-476) -- 118 dictionary codes, ~29 runs per marker instead of
            # ~21: the cost of the path is per RUN, so this is where it is slowest; and the middle of the range,
            # qualities 10..45 (72 codes).  Same 48 points, same launch.  create_ms: vb2_ctx_create of that sample
            # (median of 5): wall-clock and CPU time of the calling thread (classification, run-length coding and
            # packing run on the device: flatten_kernels.hip).
            def create_times(dd):
                vb.LikelihoodContext(dd, device=local_rank).close()
                wl, cp = [], []
                for _ in range(5):
                    t1, c1 = time.perf_counter(), time.thread_time()
                    cx = vb.LikelihoodContext(dd, device=local_rank)
                    wl.append(time.perf_counter() - t1); cp.append(time.thread_time() - c1)
                    cx.close()
                cj, csrc = latest_profile("create_kernel_stats.json")
                return {"wall": 1e3 * sorted(wl)[2], "host_cpu": 1e3 * sorted(cp)[2],
                        "device_kernels_from_profile": cj, "profile_source": csrc}
            result["create_ms"] = {"q20_40": create_times(data)}

            def alphabet_leg(q_lo, q_hi, pmc_name):
                wide = vb.synth.make_pileup(args.markers, args.depth, k, alpha_true=0.05, seed=2, q_lo=q_lo, q_hi=q_hi)
                wctx = vb.LikelihoodContext(wide, device=local_rank, stream=stream.cuda_stream)
                winfo = wctx.info()
                wout = torch.zeros(B, dtype=torch.float64, device="cuda")
                w_us = timed_launches(wctx, pts, wout, B, stream, 1000, torch)
                w_llk = wout.cpu().numpy().copy()
                wopt = None
                if not args.no_optimize:
                    wctx.optimize()
                    t_w = []
                    for _ in range(3):
                        t1 = time.perf_counter()
                        west = wctx.optimize()
                        t_w.append(time.perf_counter() - t1)
                    wopt = {"wall_ms_to_converged_alpha": 1e3 * min(t_w), "alpha": west["alpha"], "num_eval": west["num_eval"]}
                wctx.close()
                wj, wsrc = latest_profile(pmc_name) if pmc_name else (None, None)
                from verifybamid_amd import _abi as abi_w
                if wj and wj.get("kernel_src_hash") != abi_w.kernel_source_hash():
                    wj = None                                  # (measured on other kernel sources: dropped)
                li = wj.get("lane_instr_per_marker_point") if wj else None
                nominal = winfo["algorithmic_bytes_per_eval"] * B / (w_us * 1e-6) / 1e9
                lds_us = 1e6 * (48.0 * winfo["num_step"] + 16.0 * k * winfo["num_active_marker"]) * B / (256.0 * 256 * 2.4e9)
                obj = {
                    "what": "the headline launch on the same sample shape with base qualities uniform in %d..%d "
                            "(%d dictionary codes instead of %d)" % (q_lo, q_hi, winfo["num_code"], info["num_code"]),
                    "distinct_codes": int(winfo["num_code"]), "reads": int(winfo["num_read"]),
                    "device_us_per_launch": w_us, "evals_per_s": B / w_us * 1e6,
                    # frac: the time the launch's LDS gathers alone would take at the LDS peak (the headline's binding term:
                    # roofline.terms.lds) over the measured time; nominal: SURVEY 8d bytes against 8 TB/s
                    "bound": "lds", "frac": lds_us / w_us, "t_ideal_us": lds_us,
                    "layout": "probability domain" if winfo.get("layout") else "run words",
                    "table_rows": int(winfo["num_table_row"]), "steps_per_marker": winfo["num_step"] / max(1, winfo["num_active_marker"]),
                    "nominal": {"bound": "hbm", "achieved": nominal, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                "frac": nominal / HBM_PEAK_GBPS},
                    "ratio_to_headline": (B / w_us * 1e6) / (B / (1e3 * dev_ms / args.steps) * 1e6),
                    "lane_instr_per_marker_point": li,
                    "valu_busy_frac": wj.get("valu_busy_frac") if wj else None,
                    "lds_busy_frac": wj.get("lds_busy_frac") if wj else None,
                    "lds_bank_conflict_frac": wj.get("lds_bank_conflict_frac") if wj else None, "pmc_source": wsrc,
                    "optimize": wopt, "create_ms": create_times(wide),
                    "launch": ("ONE launch, the six point groups split between sets of two or three workgroups (llk_eval_split_kernel)"
                               if winfo.get("layout") else
                               ("one launch of two passes of 24 points (llk_eval_passes_kernel)" if winfo["num_code"] > 80 else
                                "two launches of llk_eval_kernel<2,...>, 32 + 16 points")),
                }
                return obj, wide, w_llk
            result["roofline_wide_alphabet"], wide, wide_llk = alphabet_leg(2, 60, "valu_b%d_wide.json" % B)
            result["roofline_mid_alphabet"], _, _ = alphabet_leg(10, 45, "valu_b%d_mid.json" % B)
        if world == 1 and not args.no_optimize:
            # second half of the metric: wall-clock of OptimizeLLK (Initialize + Homo + Heter +
            # LLK0), best of 3; measured before the CPU leg so no OpenMP threads are around
            ctx.optimize()
            t_opt = []
            for _ in range(3):
                t1 = time.perf_counter()
                est = ctx.optimize()
                t_opt.append(time.perf_counter() - t1)
            w_opt = min(t_opt)
            result["optimize"] = {
                "wall_ms_to_converged_alpha": 1e3 * w_opt,
                "alpha": est["alpha"], "alpha_true": 0.05, "num_eval": est["num_eval"],
                "num_launch_point": est["num_launch_point"],
                # the search against the same nominal roofline: the reference's evaluations (num_eval) x the
                # algorithmic bytes of one, over the wall-clock; and the same for every point actually launched
                # (the speculative {R, E, C_A, C_R} batches evaluate 2.5 points per committed one)
                "useful_evals_per_s": est["num_eval"] / w_opt,
                "algorithmic_GBps": info["algorithmic_bytes_per_eval"] * est["num_eval"] / w_opt / 1e9,
                # frac: the launched points at the headline launch's rate per point (x its fraction of the measured issue
                # ceiling) over the wall-clock; nominal_*: SURVEY 8d bytes of the useful / launched evaluations over 8 TB/s
                "frac": (ROOFLINE["frac_headline"] * ROOFLINE["us_per_point_headline"] * est["num_launch_point"] / (1e6 * w_opt))
                        if ROOFLINE.get("frac_headline") else None,
                "nominal_frac": info["algorithmic_bytes_per_eval"] * est["num_eval"] / w_opt / 1e9 / HBM_PEAK_GBPS,
                "nominal_frac_launched_points": info["algorithmic_bytes_per_eval"] * est["num_launch_point"] / w_opt / 1e9
                                                / HBM_PEAK_GBPS,
                "us_per_round": 1e6 * w_opt / max(1.0, est["num_launch_point"] / 4.0),
            }
        if world == 1 and not args.no_extras and args.cohort_samples > 0:
            # BASELINE.json configs[4] per GPU: a cohort of C3-shaped samples searched in lock-step
            S = args.cohort_samples
            # (8 distinct synthetic samples, each uploaded several times: every context has its own
            # copy in HBM, so the device sees S independent samples; generating S of them would
            # take a second of numpy each)
            distinct = [data] + [vb.synth.make_pileup(args.markers, args.depth, k, alpha_true=0.02 + 0.02 * s,
                                                      seed=1000 + s) for s in range(1, min(S, 8))]
            datas = [distinct[s % len(distinct)] for s in range(S)]
            cctx = [ctx] + [vb.LikelihoodContext(dd, device=local_rank) for dd in datas[1:]]
            with vb.CohortBatch(cctx) as batch:
                npt = np.full(S, 4, dtype=np.int32)
                p1 = np.zeros((S, 8, k)); p2 = np.zeros((S, 8, k)); al = np.full((S, 8), 0.1)
                p1[:, :4] = pts_h[:4, :k]; p2[:, :4] = pts_h[:4, k:2 * k]; al[:, :4] = pts_h[:4, 2 * k]
                def time_steps(npts_arr, n3=200):
                    step_c, _ = batch.prepared_eval(npts_arr, p1, p2, al)     # (marshalling done once)
                    for _ in range(20):
                        step_c()
                    t1 = time.perf_counter()
                    for _ in range(n3):
                        step_c()
                    return (time.perf_counter() - t1) / n3
                dt4 = time_steps(npt)
                dt1 = time_steps(np.full(S, 1, dtype=np.int32))
                dt2 = time_steps(np.full(S, 2, dtype=np.int32))
                batch.optimize()
                t1 = time.perf_counter()
                ests = batch.optimize()
                dto = time.perf_counter() - t1
            step_bytes = sum(c.info()["cohort_step_bytes"] for c in cctx)        # HBM bytes one step streams (all samples)
            alg_bytes = sum(c.info()["algorithmic_bytes_per_eval"] for c in cctx)   # SURVEY 8d, one point per sample
            for c in cctx[1:]:
                c.close()
            # per step shape: algorithmic bytes (points x SURVEY 8d's per-evaluation figure, summed over the
            # samples), the device bytes the step streams from HBM (every sample's run lists, panel rows and
            # constants once, whatever the points), and both against the 8 TB/s peak.  `traffic` = the same
            # launch's PMC FETCH_SIZE (profiles/<round>/cohort_traffic.json) when a committed pass matches.
            ctj, ctsrc = latest_profile("cohort_traffic.json")
            shapes = {}
            for npnt, dt_s in ((1, dt1), (2, dt2), (4, dt4)):
                tr = None
                if ctj and ctj.get("samples") == S and ctj.get("markers") == args.markers:
                    tr = ctj.get("traffic_bytes_per_step", {}).get(str(npnt))
                shapes["points_%d" % npnt] = {
                    "step_us": 1e6 * dt_s, "algorithmic_bytes": int(alg_bytes * npnt),
                    # frac: the bytes the step really streams from HBM (every sample's lists and rows once) against 8 TB/s;
                    # nominal_frac: SURVEY 8d's per-evaluation bytes x points, which the points of a sample share
                    "bound": "hbm", "frac": step_bytes / dt_s / 1e9 / HBM_PEAK_GBPS,
                    "nominal_frac": alg_bytes * npnt / dt_s / 1e9 / HBM_PEAK_GBPS,
                    "streamed_bytes": int(step_bytes), "streamed_GBps": step_bytes / dt_s / 1e9,
                    "streamed_frac": step_bytes / dt_s / 1e9 / HBM_PEAK_GBPS,
                    "traffic": tr, "traffic_source": ctsrc if tr else None,
                }
            result["cohort"] = {
                "step_shapes": shapes, "streamed_bytes_per_sample": int(step_bytes / S),
                "what": "%d samples of the workload's shape on ONE GPU, searched in lock-step (vb2_batch_*: one launch "
                        "per Nelder-Mead step for all samples)" % S,
                "samples": S, "step_us_4_points_per_sample": 1e6 * dt4, "evals_per_s": 4 * S / dt4,
                "step_us_2_points_per_sample": 1e6 * dt2, "step_us_1_point_per_sample": 1e6 * dt1,
                "num_eval_first": ests[0]["num_eval"], "points_launched_first": ests[0]["num_launch_point"],
                "optimize_ms_per_sample": 1e3 * dto / S, "samples_per_s_search_only": S / dto,
                "alpha_first": ests[0]["alpha"],
                "search_note": "two half-cohorts take turns on the device; when half of a lane's samples have converged the "
                               "rest are regrouped with twice the workgroups each (VB2_COHORT_REGROUP=0: not)",
            }
        if world == 1 and not args.no_extras and args.cohort_samples > 0 and args.cohort_files > 0:
            # the same cohort from TEXT files (vb2_cohort_run: the panel read once, pileups parsed and
            # flattened by host threads while the device searches the previous group) -- BASELINE.json
            # configs[4] per GPU, end to end.  8 distinct pileups, read cyclically.
            import shutil
            import tempfile
            tmp = tempfile.mkdtemp(prefix="vb2_bench_")
            try:
                base = vb.synth.with_sanity_stats(data)
                pre = vb.synth.write_files(base, os.path.join(tmp, "panel"))
                piles = []
                for s_ in range(8):
                    # reads drawn ON the panel the files are run against (round 3 drew each pileup with its own
                    # random panel and alleles and then swapped the panel in: the bytes were right, the likelihood
                    # surface -- hence the search length -- was not)
                    off_, ch_, qu_ = vb.synth.reads_on_panel(base.means, base.meta["ref_base"], base.alt_base,
                                                             args.depth, alpha_true=0.01 * (1 + s_), seed=2000 + s_)
                    dep_ = np.diff(off_).astype(np.float64)
                    dd = vb.PileupData(k, base.ud, base.means, off_, ch_, qu_, base.alt_base, None,
                                       float(dep_[dep_ > 0].mean()), 0.0, True, dict(base.meta))
                    piles.append(vb.synth.write_files(dd, os.path.join(tmp, "s%d" % s_)) + ".pileup")
                nf = args.cohort_files
                paths = [piles[i % len(piles)] for i in range(nf)]
                outs = [os.path.join(tmp, "out%d" % i) for i in range(nf)]
                with open(os.devnull, "w") as devnull:          # (the reference's NOTICE lines: 3 per sample)
                    saved = os.dup(2)
                    os.dup2(devnull.fileno(), 2)
                    try:
                        # (an untimed call on 64 of the files first: the reader threads' buffers, the pinned and device slabs
                        # and the page cache of the eight files are one-time costs of the process, not of a sample)
                        vb.run_cohort_files(pre, paths[:64], outs[:64], num_pc=k)
                        t1, c1 = time.perf_counter(), time.process_time()
                        res = vb.run_cohort_files(pre, paths, outs, num_pc=k)
                        dtf, cpuf = time.perf_counter() - t1, time.process_time() - c1
                    finally:
                        os.dup2(saved, 2)
                        os.close(saved)
                ok = sum(1 for r in res if r["status"] == 0)
                result["cohort"]["from_text"] = {
                    "what": "vb2_cohort_run on %d C3-shaped text pileups (7.6 MB each) + one panel, outputs written; "
                            "wall-clock of the call (after an untimed call on 64 of the files: thread buffers, slabs, page cache).  32 slots on the device: a converged sample hands its slot to the next "
                            "one the reader threads have ready (VB2_COHORT_STREAM=0: groups of 32 one after the other)" % nf,
                    "host_cpus_by_affinity": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
                    "samples": nf, "samples_ok": ok, "seconds": dtf, "samples_per_s": nf / dtf,
                    # host or device bound: CPU seconds the process consumed during the call (readers: parse,
                    # resolve, create; one spinning pipeline thread per device; the releaser) against what its CPU allowance
                    # (cgroup quota / affinity) offers in that wall-clock; the device side of a sample is the search-only rate
                    "host_cpu_seconds": cpuf, "host_cpu_ms_per_sample": 1e3 * cpuf / nf,
                    "cpus_allowed": cpus_allowed(), "host_utilisation": cpuf / (dtf * cpus_allowed()),
                    "device_ms_per_sample_search_only": result["cohort"].get("optimize_ms_per_sample"),
                    "bound": "host" if cpuf / (dtf * cpus_allowed()) > 0.8 else
                             ("device" if result["cohort"].get("optimize_ms_per_sample") and
                              1e-3 * result["cohort"]["optimize_ms_per_sample"] * nf / dtf > 0.8 else "pipeline (neither side above 80 %)"),
                    "alpha_first": res[0]["alpha"], "alpha_true_first": 0.01,
                    "alpha_by_distinct_sample": [res[i]["alpha"] for i in range(min(nf, 8))],
                    "alpha_true_by_distinct_sample": [0.01 * (1 + i) for i in range(min(nf, 8))],
                }
                # (the reads belong to the panel: every estimate sits next to the value the reads were drawn with)
                if ok and abs(res[0]["alpha"] - 0.01) > 5e-3:
                    result["cohort"]["from_text"]["error"] = "alpha_first %.4g is not within 5e-3 of 0.01" % res[0]["alpha"]
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        # small parity probe against the oracle (checker only; after the GPU legs: its OpenMP threads
        # spin for a while after the call and would slow the launching thread down)
        from oracle.bridge import oracle_data
        od = oracle_data(data)
        # every timed point (round 3 probed the first two of the 48)
        want = np.array([od.llk(pts_h[i, :k], pts_h[i, k:2 * k], pts_h[i, 2 * k],
                                num_thread=min(os.cpu_count() or 1, 16)) for i in range(B)])
        result["parity_probe_max_rel_err"] = float(np.max(np.abs(llk_dev[:len(want)] - want) / np.abs(want)))
        result["parity_probe_points"] = int(len(want))
        if world == 1 and "roofline_wide_alphabet" in result:
            odw = oracle_data(wide)
            nw = min(B, 8)
            want_w = np.array([odw.llk(pts_h[i, :k], pts_h[i, k:2 * k], pts_h[i, 2 * k],
                                       num_thread=min(os.cpu_count() or 1, 16)) for i in range(nw)])
            result["roofline_wide_alphabet"]["parity_probe_max_rel_err"] = float(
                np.max(np.abs(wide_llk[:nw] - want_w) / np.abs(want_w)))
            result["roofline_wide_alphabet"]["parity_probe_points"] = nw
        if world == 1 and not args.no_cpu_baseline:
            # bounded sample (~10 s wall): the C oracle on the SAME pileup, OpenMP over
            # markers like the reference; thread counts 1, 4 (the reference's default
            # --NumThread) and powers of two up to the cores this process may use; the
            # best one is reported.
            try:
                navail = len(os.sched_getaffinity(0))
            except AttributeError:
                navail = os.cpu_count() or 1
            quota = None                 # a container's CFS quota: the host's cores are visible, the time is not
            try:
                q, per = open("/sys/fs/cgroup/cpu.max").read().split()
                if q != "max":
                    quota = max(1, round(int(q) / int(per)))
            except (OSError, ValueError):
                pass
            # (thread counts beyond twice the quota only measure the throttling)
            top = min(navail, 2 * quota) if quota else navail
            sweep = sorted({1, 4} | {t for t in (8, 16, 32, 64, 128, 256) if t <= top})
            rates = {}
            for nt in sweep:
                n_cpu, tc = 0, time.perf_counter()
                while time.perf_counter() - tc < 10.0 / len(sweep) or n_cpu < 2:
                    od.llk(pts_h[n_cpu % B, :k], pts_h[n_cpu % B, k:2 * k], pts_h[n_cpu % B, 2 * k],
                           num_thread=nt)
                    n_cpu += 1
                rates[nt] = n_cpu / (time.perf_counter() - tc)
            best = max(rates, key=rates.get)
            # second half of the metric on the CPU (SURVEY 8d "CPU baseline beside it"): the oracle's OptimizeLLK
            # (same algorithm, same 780 evaluations) on the same pileup at --NumThread 1, 4 (the reference's
            # default, main.cpp:79) and the best thread count of the sweep -- one run each, ~10 + 2.5 + 0.7 s
            cpu_opt, cpu_alpha = {}, None
            if not args.no_optimize:
                for nt in sorted({1, 4, best}):
                    tc = time.perf_counter()
                    r_cpu = od.optimize(num_thread=nt)
                    cpu_opt[str(nt)] = 1e3 * (time.perf_counter() - tc)
                    cpu_alpha = r_cpu["alpha"]
            result["cpu_baseline"] = {
                "value": rates[best], "unit": "evals/s", "cores": best, "kind": "port",
                "evals_per_s_by_threads": {str(t): r for t, r in rates.items()},
                "optimize_wall_ms_by_threads": cpu_opt, "optimize_alpha": cpu_alpha,
                "sample": "C oracle (oracle/vb2_oracle.c, OpenMP over markers like the reference) on the "
                          "same %d-marker pileup, ~%.1f s per thread count; evals/s by threads: %s; one full "
                          "OptimizeLLK per thread count in optimize_wall_ms_by_threads; "
                          "%d hardware threads visible, CPU quota of the container: %s"
                          % (args.markers, 10.0 / len(sweep), {t: round(r, 1) for t, r in rates.items()}, navail,
                             "%d CPUs" % quota if quota else "none"),
            }
            # the two speed-ups the north star asks about (>= 50x), both against the best CPU figure and
            # against the reference's default --NumThread 4
            sp_up = {"evals_per_s_vs_best_cpu": value / rates[best], "evals_per_s_vs_numthread_4": value / rates[4]}
            if cpu_opt and "optimize" in result:
                g_ms = result["optimize"]["wall_ms_to_converged_alpha"]
                sp_up["optimize_wall_vs_best_cpu"] = cpu_opt[str(best)] / g_ms
                sp_up["optimize_wall_vs_numthread_4"] = cpu_opt["4"] / g_ms
                sp_up["optimize_wall_vs_numthread_1"] = cpu_opt["1"] / g_ms
                sp_up["alpha_gpu_minus_cpu"] = result["optimize"]["alpha"] - cpu_alpha
            result["speedup_vs_cpu"] = sp_up
    if ctx is not None:
        ctx.close()
    if group is not None:
        group.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    # RCCL prints a version banner through C stdio when its first communicator comes up; push that
    # out first, so that the JSON line is the LAST line of stdout (whatever prints after it, on the way
    # out of the interpreter, goes to file descriptor 1 = stderr)
    import ctypes
    ctypes.CDLL(None).fflush(None)
    if rank == 0:
        emit(result)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
