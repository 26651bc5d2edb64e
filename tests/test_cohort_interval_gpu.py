"""--CohortInterval on the MI355X: the derivatives of several samples in one launch pair (vb2_batch_derivs) are the
single-sample kernels' bits; the intervals of a batch advancing in lock-step (vb2_batch_interval) are vb2_ctx_interval's,
field for field and bit for bit, in every model, whatever the batch holds; the steps are shared; and the cohort runner end
to end, streamed and group at a time, with slots that change hands and a sample that fails its sanity check."""
import os
import subprocess

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
CHUNK = 4                                            # kDerivChunk (csrc/deriv_kernels.h)


def _num_cu(ctx):
    import torch
    return torch.cuda.get_device_properties(ctx.info()["device"]).multi_processor_count


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


# ---- 1. batched derivatives ----

ALPHAS = [1e-6, -0.1, 0.3, 0.03, 0.5, 0.97, 1.2]     # (1e-6; two outside [0, 1])


def _derivative_samples(k):
    """(data, points of the ragged call): 1, 17, 300, 3 000 and 20 000 markers and a sample that falls back to run words."""
    specs = [(1, 30, 0), (17, 30, 1), (300, 30, 3), (3000, 30, 4), (20000, 8, 7), (200, 1500, 4)]
    return [(vb.synth.make_pileup(M, mean_depth=depth, num_pc=k, alpha_true=0.1, seed=5 + i), n)
            for i, (M, depth, n) in enumerate(specs)]


def _points(k, n, seed):
    rng = np.random.default_rng(seed)
    scale = np.where(np.arange(n) % 2 == 0, 0.01, 0.05)[:, None]
    return rng.normal(0, 1, (n, k)) * scale, rng.normal(0, 1, (n, k)) * scale, np.array(ALPHAS[:n], dtype=np.float64)


@pytest.mark.parametrize("k", [2, 4])
def test_batched_derivatives_are_the_single_sample_bits(k, tunable):
    tunable("pd", 1)
    samples = _derivative_samples(k)
    ctxs = [vb.LikelihoodContext(d) for d, _ in samples]
    try:
        layouts = [c.info()["layout"] for c in ctxs]
        assert layouts[5] == 0 and layouts[3] == 1 and layouts[4] == 1          # both layout classes in one call
        # the 20 000-marker sample: more groups of 16 micro-tiles than the stripe workgroups it gets -- in the first step of
        # the ragged call (1 + 3 + 4 + 4 + 4 points) and when every sample asks for 4 -- so its stripe loop runs again
        ntile_grp = (ctxs[4].info()["num_tile"] + 15) // 16
        for total in (16, 4 * len(ctxs)):
            gx = max(1, (4 * _num_cu(ctxs[4]) + total - 1) // total)
            assert ntile_grp > gx, (ntile_grp, gx)
        for counts in ([n for _, n in samples], [CHUNK] * len(ctxs)):
            pts = [_points(k, n, 100 + s) for s, n in enumerate(counts)]
            alone = [c.derivatives(*p) if n else None for c, p, n in zip(ctxs, pts, counts)]
            cat = [np.concatenate([p[j] for p in pts]) for j in range(3)]
            with vb.CohortBatch(ctxs) as batch:
                got = batch.derivatives(counts, *cat)
                again = batch.derivatives(counts, *cat)
            for x, y in zip(got, again):
                assert _bits(x) == _bits(y)
            o = 0
            for s, n in enumerate(counts):
                for j in range(3):
                    if n:
                        assert _bits(got[j][o:o + n]) == _bits(alone[s][j]), (k, s, n, "llk grad hess".split()[j])
                o += n
            assert np.isfinite(got[0]).all()
    finally:
        for c in ctxs:
            c.close()


# ---- 2. and 3. lock-step intervals ----

MODELS = [("default", {}, False), ("within", dict(within_ancestry=True), False), ("fixpc", dict(fix_pc=[0.01, 0.02]), False),
          ("fixalpha", dict(fix_alpha=0.05), False), ("knownaf", {}, True)]


def _interval_samples(known_af):
    out = [vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=a, seed=31 + i) for i, a in enumerate((0.0, 0.03, 0.2))]
    # -H at the estimate not positive definite under the default model, and lo = 0 (test_hessian_not_negative_definite_gives_na)
    out.append(vb.synth.make_pileup(300, mean_depth=10, num_pc=2, alpha_true=0.0, seed=11))
    if known_af:
        for d in out:
            d.known_af = np.clip(d.means / 2.0, 0.01, 0.99)
    return out


def _same_interval(a, b, what):
    """Every field of two interval dicts, bit for bit (NaN = NaN)."""
    assert a.keys() == b.keys()
    for key in a:
        if key == "rows":
            assert len(a["rows"]) == len(b["rows"]), what
            for ra, rb in zip(a["rows"], b["rows"]):
                assert ra["param"] == rb["param"] and ra["method"] == rb["method"], what
                for f in ("estimate", "stderr", "lo", "hi"):
                    assert _bits(ra[f]) == _bits(rb[f]), (what, ra, rb)
        elif isinstance(a[key], float):
            assert _bits(a[key]) == _bits(b[key]), (what, key, a[key], b[key])
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


@pytest.mark.parametrize("name,kw,kaf", MODELS, ids=[m[0] for m in MODELS])
def test_lockstep_intervals_are_the_single_sample_intervals(name, kw, kaf):
    data = _interval_samples(kaf)
    ctxs = [vb.LikelihoodContext(d) for d in data]
    try:
        ests = [c.optimize(**kw) for c in ctxs]
        alone = [dict(c.interval(e, **kw), status=0) for c, e in zip(ctxs, ests)]
        if name == "default":
            assert not alone[3]["pos_def"] and alone[3]["lo"] == 0.0 and all(a["pos_def"] for a in alone[1:3])
        if name == "fixalpha":
            assert all(a["num_launch"] == 1 and not a["alpha_free"] for a in alone)
        launches = [a["num_launch"] for a in alone]
        if name != "fixalpha":
            assert len(set(launches)) > 1                                # samples finish at different steps

        def run(order):
            with vb.CohortBatch([ctxs[s] for s in order]) as batch:
                got = batch.intervals([ests[s] for s in order], **kw)
                steps = batch.num_interval_step
            for s, ci in zip(order, got):
                _same_interval(ci, alone[s], (name, order, s))
            # 3. the steps are shared: as many as the slowest sample's, not the sum
            assert steps == max(launches[s] for s in order), (steps, [launches[s] for s in order])
        run([0, 1, 2, 3])
        run([3, 2, 0, 1])
        run([1, 3, 0])
        for s in range(4):
            run([s])
    finally:
        for c in ctxs:
            c.close()


# ---- 4. end to end ----

@pytest.fixture(scope="module")
def cohort_files(tmp_path_factory):
    """One synthetic panel and eight pileups of 2 500 markers on it; sample 5 covers 300 markers and fails its sanity check."""
    tmp = tmp_path_factory.mktemp("cohort_interval")
    k, M = 2, 2500
    base = vb.synth.with_sanity_stats(vb.synth.make_pileup(M, 14, k, alpha_true=0.03, seed=50))
    pre = vb.synth.write_files(base, str(tmp / "panel"))
    piles = []
    for s in range(8):
        d = vb.synth.make_pileup(M, 10 + 2 * s, k, alpha_true=(0.0, 0.02, 0.05, 0.1, 0.2, 0.05, 0.0, 0.3)[s], seed=60 + s)
        off, bases, quals = d.read_off, d.bases, d.quals
        if s == 5:
            off = off.copy()
            off[301:] = off[300]
            bases, quals = bases[:off[300]], quals[:off[300]]
        d = vb.PileupData(k, base.ud, base.means, off, bases, quals, base.alt_base, None, d.avg_depth, d.sd_depth,
                          True, dict(base.meta))
        piles.append(vb.synth.write_files(d, str(tmp / ("s%d" % s))) + ".pileup")
    return dict(k=k, pre=pre, piles=piles, tmp=tmp, bad=5)


def _ostream(v):
    """A double in the default ostream format (6 significant digits), NA for none."""
    return "NA" if np.isnan(v) else "%g" % v


def _ci_rows(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "#PARAM\tESTIMATE\tSTDERR\tCI_LOW\tCI_HIGH\tMETHOD"
    return [ln.split("\t") for ln in lines[1:]]


def _struct_rows(ci):
    return [[r["param"], _ostream(r["estimate"]), _ostream(r["stderr"]), _ostream(r["lo"]), _ostream(r["hi"]), r["method"]]
            for r in ci["rows"]]


@pytest.mark.parametrize("stream", [1, 0])
def test_cohort_run_with_intervals(cohort_files, stream, tunable):
    f = cohort_files
    k, tmp, bad = f["k"], f["tmp"], f["bad"]
    good = [s for s in range(8) if s != bad]
    tunable("cohort_stream", stream)
    plain = [str(tmp / ("plain%d_%d" % (stream, s))) for s in range(8)]
    res0 = vb.run_cohort_files(f["pre"], f["piles"], plain, num_pc=k, group_size=3)
    outs = [str(tmp / ("ci%d_%d" % (stream, s))) for s in range(8)]
    res = vb.run_cohort_files(f["pre"], f["piles"], outs, num_pc=k, group_size=3, confidence_interval=True)   # three slots
    assert [r["status"] for r in res] == [r["status"] for r in res0] == \
        [_abi.VB2_ERR_SANITY if s == bad else 0 for s in range(8)]
    # the failed sample has no .CI and no interval; nobody else is affected
    assert not os.path.exists(outs[bad] + ".CI") and "interval" not in res[bad]
    for s in good:
        for ext in (".selfSM", ".Ancestry"):
            assert open(outs[s] + ext, "rb").read() == open(plain[s] + ext, "rb").read(), (s, ext)
        assert not os.path.exists(plain[s] + ".CI")
        assert _bits(res[s]["alpha"]) == _bits(res0[s]["alpha"]) and _bits(res[s]["llk1"]) == _bits(res0[s]["llk1"])
    # every number of each .CI is vb2_ctx_interval's at the sample's cohort estimate; and where that estimate is the single
    # run's, bit for bit, the file is that of --PileupFile --ConfidenceInterval (checked first)
    same_as_single = 0
    for s in good:
        single_out = str(tmp / ("single%d_%d" % (stream, s)))
        single = vb.run_files(f["pre"], f["piles"][s], single_out, num_pc=k, confidence_interval=True)
        if all(_bits(single[key]) == _bits(res[s][key]) for key in ("alpha", "llk1", "pc", "pc2")):
            same_as_single += 1
            assert open(outs[s] + ".CI", "rb").read() == open(single_out + ".CI", "rb").read(), s
        flat = vb.PileupData.from_files(f["pre"], f["piles"][s], num_pc=k, disable_sanity=False)
        with vb.LikelihoodContext(flat) as ctx:
            direct = ctx.interval(res[s])
        _same_interval(dict(direct, status=0), dict(res[s]["interval"], status=0), ("cohort", stream, s))
        assert _ci_rows(outs[s] + ".CI") == _struct_rows(direct), s
    # (tests/test_model_paths_gpu.py pins the cohort's .selfSM and .Ancestry to the single run's, not the estimate's last bits:
    # a cohort step and a single sample's search sum a marker's reads in different kernels)
    print("cohort_stream %d: %d of %d cohort estimates are the single run's bit for bit" % (stream, same_as_single, len(good)))
    # the samples without the failed one: everybody's files are what they were
    outs7 = [str(tmp / ("ci7_%d_%d" % (stream, s))) for s in good]
    res7 = vb.run_cohort_files(f["pre"], [f["piles"][s] for s in good], outs7, num_pc=k, group_size=3, confidence_interval=True)
    assert [r["status"] for r in res7] == [0] * 7
    for o7, s in zip(outs7, good):
        for ext in (".selfSM", ".Ancestry", ".CI"):
            assert open(o7 + ext, "rb").read() == open(outs[s] + ext, "rb").read(), (s, ext)


def _cli(f, lst, out, extra, stream):
    env = dict(os.environ, VB2_COHORT_STREAM=str(stream))
    p = subprocess.run([EXE, "--SVDPrefix", f["pre"], "--Reference", "x.fa", "--NumPC", str(f["k"]), "--PileupList", lst,
                        "--Output", out] + extra, capture_output=True, text=True, timeout=300, env=env)
    return p


@pytest.mark.parametrize("stream", [1, 0])
def test_command_line_with_cohort_interval_and_find_source(cohort_files, stream):
    f = cohort_files
    tmp, bad = f["tmp"], f["bad"]
    runs = {}
    for tag, extra in (("a", []), ("b", ["--CohortInterval"]), ("c", ["--FindSource"]), ("d", ["--FindSource", "--CohortInterval"])):
        outs = [str(tmp / ("cli%d%s_%d" % (stream, tag, s))) for s in range(8)]
        lst = str(tmp / ("list%d%s.txt" % (stream, tag)))
        with open(lst, "w") as fh:
            for p, o in zip(f["piles"], outs):
                fh.write("%s\t%s\n" % (p, o))
        p = _cli(f, lst, str(tmp / ("cli%d%s" % (stream, tag))), extra, stream)
        assert p.returncode != 0 and "FATAL" not in p.stderr, p.stderr[-2000:]      # (one sample failed its own check)
        runs[tag] = (p, outs)
    strip = lambda text, tag: text.replace("cli%d%s" % (stream, tag), "cliX")     # (the output prefixes are in the table)
    for tag in "bcd":
        assert strip(runs[tag][0].stdout, tag) == strip(runs["a"][0].stdout, "a")
        for s in range(8):
            for ext in (".selfSM", ".Ancestry"):
                if s != bad:
                    assert open(runs[tag][1][s] + ext, "rb").read() == open(runs["a"][1][s] + ext, "rb").read(), (tag, s, ext)
            assert os.path.exists(runs[tag][1][s] + ".CI") == (tag in "bd" and s != bad), (tag, s)
    for s in range(8):
        if s != bad:
            assert open(runs["b"][1][s] + ".CI", "rb").read() == open(runs["d"][1][s] + ".CI", "rb").read()
    src_c = open(str(tmp / ("cli%dc.Sources" % stream))).read()
    src_d = open(str(tmp / ("cli%dd.Sources" % stream))).read()
    assert strip(src_d, "d") == strip(src_c, "c") and src_c.count("\n") > 1
    # interval NOTICE lines of a cohort run name the sample's output prefix (sample 0 and 6: alpha_true 0)
    notices = [ln for ln in runs["b"][0].stderr.splitlines() if "not negative definite" in ln or "higher log-likelihood" in ln]
    for ln in notices:
        assert any(("NOTICE - %s: " % o) in ln for o in runs["b"][1]), ln
