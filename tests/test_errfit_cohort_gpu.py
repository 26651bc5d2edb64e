"""The batched E-step of the error-rate fit on the GPU: vb2_errstat_batch_eval
against vb2_errstat_eval, sample by sample and BIT FOR BIT -- n, s and llk as bytes.  Nothing here has a tolerance: the
batched kernel adds a marker's reads in the single kernel's order, forms w and r by its expressions, and everything behind r
is integer.

The shapes are where the kernel can go wrong, not the workload's: marker counts around the group of 256, k with and without
an unrolled projection, known allele frequencies, depth 1, a marker of 900 reads, and -- because the kernel stages a group's
reads in chunks of kErrMultiChunk = 8 192 (errstat_multi_kernels.h) -- a marker of 9 000 reads, which no chunk holds, a
group of 300 x 40 = 12 000 reads, which takes two, and 17 x 600, whose one group ends inside the second chunk.
"""
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CHUNK = 8192                      # kErrMultiChunk: what the deep shapes below were chosen against
ALPHAS = [0.03, 0.0, 1.0, 0.5, 1e-6]


def _with_depths(d, depth):
    """d with marker m holding depth[m] reads, its own taken round and round (a marker that had none: marker 0's)."""
    M = d.num_marker
    off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(depth, out=off[1:])
    bases = np.empty(int(off[-1]), dtype=np.uint8)
    quals = np.empty(int(off[-1]), dtype=np.uint8)
    for m in range(M):
        lo, hi = int(off[m]), int(off[m + 1])
        src = m if d.read_off[m + 1] > d.read_off[m] else int(np.argmax(np.diff(d.read_off) > 0))
        olo, n = int(d.read_off[src]), int(d.read_off[src + 1] - d.read_off[src])
        take = olo + np.arange(hi - lo) % max(1, n)
        bases[lo:hi] = d.bases[take]
        quals[lo:hi] = d.quals[take]
    return vb.PileupData(d.num_pc, d.ud, d.means, off, bases, quals, d.alt_base, d.known_af, d.avg_depth, d.sd_depth,
                         d.sanity_disabled, dict(d.meta))


def _make(M, k, seed, depth=30, known_af=False, **kw):
    d = vb.synth.make_pileup(M, mean_depth=depth, num_pc=k, alpha_true=0.05, seed=seed, **kw)
    if known_af:
        d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(seed).normal(0, 0.02, M), 0.0, 1.0)
    return d


def _build_samples():
    out = []
    for i, (M, k) in enumerate([(1, 1), (255, 2), (256, 4), (257, 5), (300, 4), (3000, 4), (3000, 2)]):
        out.append(_make(M, k, 30 + i, depth=40 if M == 1 else 30))
    out.append(_make(300, 1, 40, known_af=True))
    out.append(_make(3000, 2, 41, known_af=True))
    out.append(_make(257, 4, 42, depth=1))                                       # depth 1: most markers one read or none
    d = _make(300, 2, 43)
    depth = np.diff(d.read_off)
    depth[7], depth[299] = 900, 9000                                             # 9 000 > CHUNK: no chunk holds the marker
    out.append(_with_depths(d, depth))
    d = _make(300, 4, 44, depth=40)                                              # 12 000 reads in group 0: two chunks
    assert d.read_off[256] > CHUNK
    out.append(d)
    d = _make(17, 4, 45, depth=600, q_lo=2, q_hi=60)                             # one group, 10 200 reads, wide alphabet
    assert CHUNK < d.num_read < 2 * CHUNK
    out.append(d)
    d = _make(300, 2, 46)
    out.append(_with_depths(d, np.zeros(300, dtype=np.int64)))                   # markers, no read at all
    out.append(vb.synth.with_sanity_stats(_make(300, 2, 47, missing_frac=0.1)))  # the depth filter on
    out.append(vb.synth.with_sanity_stats(_make(3000, 4, 48, missing_frac=0.05)))
    return out


def _table(d, i):
    """Table i of a sample: shifted by 3 + i % 5 qualities; every third one with its two most frequent qualities at 0 and 1."""
    t = vb.nominal_err_table()
    q = np.clip(d.quals.astype(np.int64) - 33, 0, 93)
    for v in np.unique(q):
        t[v] = min(1.0, 10.0 ** (-(int(v) - (3 + i % 5)) / 10.0))
    if i % 3 == 2 and q.size:
        top = np.bincount(q, minlength=94).argsort()[::-1]
        t[top[0]], t[top[1]] = 0.0, 1.0
    return t


def _point(d, i):
    rng = np.random.default_rng(1000 + i)
    return rng.normal(0, 0.02, d.num_pc), rng.normal(0, 0.02, d.num_pc), ALPHAS[i % len(ALPHAS)]


def _bytes(n, s, llk):
    return np.asarray(n, dtype=np.int64).tobytes() + np.asarray(s, dtype=np.float64).tobytes() + np.float64(llk).tobytes()


class _World:
    """The samples, and vb2_errstat_eval's answers, each computed once."""

    def __init__(self):
        self.samples = _build_samples()
        self._single = {}
        self._es = {}

    def single(self, j, table, p1, p2, alpha):
        key = (j, table.tobytes(), np.asarray(p1).tobytes(), np.asarray(p2).tobytes(), float(alpha))
        if key not in self._single:
            if j not in self._es:
                self._es[j] = vb.ErrStat(self.samples[j])
            self._single[key] = _bytes(*self._es[j].eval(table, p1, p2, alpha))
        return self._single[key]

    def close(self):
        for es in self._es.values():
            es.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _case(world, picks, shared_table=None):
    """Samples picks[i] (indices into world.samples), sample i with its own table i and point i."""
    ds = [world.samples[j] for j in picks]
    tables = [shared_table if shared_table is not None else _table(d, i) for i, d in enumerate(ds)]
    points = [_point(d, i) for i, d in enumerate(ds)]
    want = [world.single(j, tables[i], *points[i]) for i, j in enumerate(picks)]
    return ds, tables, points, want


def _eval(batch, tables, points, live=None):
    n, s, llk = batch.eval(np.array(tables), [p[0] for p in points], [p[1] for p in points], [p[2] for p in points], live=live)
    return [_bytes(n[i], s[i], llk[i]) for i in range(len(points))]


# ---- 1. the batch is the single E-step, bit for bit ----
@pytest.mark.parametrize("picks", [[5], [0, 3], [10, 7, 2, 12, 1], [j % 16 for j in range(64)]], ids=["S1", "S2", "S5", "S64"])
def test_batch_is_the_single_estep_bit_for_bit(world, picks):
    ds, tables, points, want = _case(world, picks)
    with vb.ErrStatBatch(ds) as b:
        got = _eval(b, tables, points)
        info = b.info()
    for i in range(len(picks)):
        assert got[i] == want[i], "sample %d (world %d: %d markers, k %d)" % (i, picks[i], ds[i].num_marker, ds[i].num_pc)
    assert info["num_sample"] == len(picks) and info["num_launch"] == 2 and info["num_eval"] == 1
    assert info["num_read"] == sum(d.num_read for d in ds) and info["num_pc"] == max(d.num_pc for d in ds)
    assert 1 <= info["last_grid"] <= 64 * len(picks)
    # something was counted, and the deep and the empty samples are what they are meant to be
    assert any(np.frombuffer(w[:94 * 8], dtype=np.int64).sum() > 0 for w in want)


def test_one_shared_table_with_entries_zero_and_one(world):
    picks = list(range(16))
    t = vb.nominal_err_table()
    t[20:41] = [min(1.0, 10.0 ** (-(q - 5) / 10.0)) for q in range(20, 41)]
    t[30], t[31], t[25] = 0.0, 1.0, 0.0
    ds, tables, points, want = _case(world, picks, shared_table=t)
    with vb.ErrStatBatch(ds) as b:
        n, s, llk = b.eval(t, [p[0] for p in points], [p[1] for p in points], [p[2] for p in points])     # [94]: one for all
        got = [_bytes(n[i], s[i], llk[i]) for i in range(len(picks))]
    assert got == want
    assert n[:, 30].sum() > 0 and n[:, 31].sum() > 0


def test_samples_without_a_job_read_zeros(world):
    """A sample without reads counts nothing; one switched off in `live`, one given as None and one of no markers take no
    workgroup: zeros and llk 0, and the others' bytes do not move."""
    picks = [4, 13, 6, 8, 2]
    ds, tables, points, want = _case(world, picks)
    zero = _bytes(np.zeros(94), np.zeros(94), 0.0)
    n13 = np.frombuffer(want[1][:94 * 8], dtype=np.int64)
    assert n13.sum() == 0 and want[1] == zero                    # (markers, but no read: every marker is skipped)
    empty = vb.PileupData(2, np.zeros((0, 2)), np.zeros(0), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint8),
                          np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
    with vb.ErrStatBatch(ds + [None, empty]) as b:
        tb = tables + [tables[0], tables[0]]
        pt = points + [(np.zeros(2), np.zeros(2), 0.03)] * 2
        got = _eval(b, tb, pt)
        assert got[:5] == want and got[5] == zero and got[6] == zero
        grid_all = b.info()["last_grid"]
        live = [1, 1, 0, 1, 0, 1, 1]
        got = _eval(b, tb, pt, live=live)
        assert [got[i] for i in (0, 1, 3)] == [want[i] for i in (0, 1, 3)] and got[2] == zero and got[4] == zero
        assert b.info()["last_grid"] < grid_all
        # what belongs to a sample that is not live is not read
        bad = [t.copy() for t in tb]
        bad[2][30] = 7.0
        pt2 = list(pt)
        pt2[4] = (pt[4][0], pt[4][1], float("nan"))
        assert _eval(b, bad, pt2, live=live) == got
        # nobody live: no launch at all
        launches = b.info()["num_launch"]
        assert _eval(b, tb, pt, live=[0] * 7) == [zero] * 7 and b.info()["num_launch"] == launches


def test_bits_do_not_depend_on_the_grid_the_call_or_the_order(world):
    picks = [5, 10, 11, 0, 8, 15, 3, 12]
    ds, tables, points, want = _case(world, picks)
    old = _abi.get_tunable("errstat_multi_groups")
    try:
        with vb.ErrStatBatch(ds) as b:
            grids = []
            for groups in (0, 0, 1, 3, 64, 1000, 0):
                _abi.set_tunable("errstat_multi_groups", groups)
                assert _eval(b, tables, points) == want, groups
                grids.append(b.info()["last_grid"])
            # one workgroup a sample; three where a sample has three groups; at most 64
            assert grids[2] == len(picks) and grids[3] == sum(min(3, -(-d.num_marker // 256)) for d in ds)
            assert grids[4] == grids[5] == sum(min(64, -(-d.num_marker // 256)) for d in ds)
        _abi.set_tunable("errstat_multi_groups", 0)
        order = np.random.default_rng(5).permutation(len(picks))
        with vb.ErrStatBatch([ds[i] for i in order]) as b:
            got = _eval(b, [tables[i] for i in order], [points[i] for i in order])
        assert got == [want[i] for i in order]
    finally:
        _abi.set_tunable("errstat_multi_groups", old)


def test_errors_and_the_shared_panel(world):
    d = world.samples[5]
    other = _make(3000, 4, 77)
    twin = vb.PileupData(4, d.ud, d.means, other.read_off, other.bases, other.quals, other.alt_base, None, 0.0, 0.0, True, {})
    t, (p1, p2, a) = _table(d, 0), _point(d, 0)
    with vb.ErrStatBatch([d, twin]) as shared, vb.ErrStatBatch([d, other]) as apart:
        assert shared.info()["num_panel"] == 1 and apart.info()["num_panel"] == 2
        assert apart.info()["device_bytes"] - shared.info()["device_bytes"] >= d.ud.nbytes
        n, s, llk = shared.eval(t, [p1, p1], [p2, p2], [a, a])
        assert _bytes(n[0], s[0], llk[0]) == world.single(5, t, p1, p2, a)
        with vb.ErrStat(twin) as es:
            assert _bytes(n[1], s[1], llk[1]) == _bytes(*es.eval(t, p1, p2, a))
        for bad in (-1e-9, 1.0000001, float("nan")):
            with pytest.raises(_abi.Vb2Error, match="alpha of sample 1 lies outside"):
                shared.eval(t, [p1, p1], [p2, p2], [a, bad])
        tt = np.array([t, t])
        tt[1, 30] = 1.5
        with pytest.raises(_abi.Vb2Error, match="quality 30"):
            shared.eval(tt, [p1, p1], [p2, p2], [a, a])
        with pytest.raises(_abi.Vb2Error):
            shared.eval(t, None, None, [a, a])
    with pytest.raises(_abi.Vb2Error, match="1..64 samples"):
        vb.ErrStatBatch([d] * 65)
    with pytest.raises(_abi.Vb2Error, match="1..64 samples"):
        vb.ErrStatBatch([])


# ---- 2. - 4. the cohort fit on the device ----
import errfit_cohort_ref as ecr  # noqa: E402
import errfit_ref as er  # noqa: E402

LLK_RTOL = 1e-12                  # tests/test_errfit_gpu.py's allowances for the device against the restatement:
ALPHA_ATOL, LLK1_RTOL = 1e-4, 1e-6      # s within LLK_RTOL s + n 2^-64; alpha 1e-4; llk 1e-6; evaluation counts equal
FIT_SAMPLES = [(11, 5), (12, 0), (13, 5), (14, 3)]      # (seed, planted shift): the second is calibrated


@pytest.fixture(scope="module")
def planted():
    """Four samples of 1 000 x 30 from errfit_ref.sample, their restatement evaluators and nominal estimates."""
    datas = [er.sample(1000, seed, shift=shift)[0] for seed, shift in FIT_SAMPLES]
    co = ecr.Cohort(datas)
    return datas, co, co.nominal_estimates()


def _fit_close(got, want):
    """test_the_fit_on_the_device_is_the_restatements' assertions, on one sample."""
    assert got["status"] == 0 and got["num_iter"] == want["num_iter"] and got["converged"] == want["converged"]
    assert got["iter_err"].tobytes() == want["iter_err"].tobytes()
    assert np.array_equal(got["err"], want["err"]) and np.array_equal(got["n"], want["n"])
    for q in np.nonzero(want["n"])[0]:
        assert abs(got["s"][q] - want["s"][q]) <= LLK_RTOL * want["s"][q] + float(want["n"][q]) * 2.0 ** -64
    assert np.allclose(got["iter_alpha"], want["iter_alpha"], rtol=0, atol=ALPHA_ATOL)
    assert np.allclose(got["iter_llk"], want["iter_llk"], rtol=LLK1_RTOL, atol=0)
    assert abs(got["estimate"]["llk1"] - want["estimate"]["llk1"]) <= LLK1_RTOL * abs(want["estimate"]["llk1"])
    assert got["num_step"] == want["num_step"] and got["estimate"]["num_eval"] == want["estimate"]["num_eval"]


def test_the_per_sample_cohort_fit_is_the_fit_alone(planted):
    datas, co, noms = planted
    fits, pool = vb.errfit_cohort(datas, noms)
    alone = [vb.errfit(d, nom) for d, nom in zip(datas, noms)]
    iters = [f["num_iter"] for f in fits]
    print("per sample: iterations %s, LRT %s" % (iters, [round(f["lrt"], 1) for f in fits]))
    for got, want in zip(fits, alone):
        # the tables, the counts and the course of the fit are equal; what a search returns, to the searches' agreement
        assert got["iter_err"].tobytes() == want["iter_err"].tobytes() and np.array_equal(got["err"], want["err"])
        assert np.array_equal(got["n"], want["n"]) and got["num_iter"] == want["num_iter"]
        assert got["converged"] and want["converged"] and got["num_bin"] == want["num_bin"] == 3
        _fit_close(got, want)
    # the samples leave at different iterations, so the lock-step thins out (on an MI355X: 9, 15, 9, 10 -- the calibrated
    # sample, whose rates barely move, is the LAST to meet the relative stop rule, not the first)
    assert min(iters) < max(iters)
    assert pool["num_iter"] == max(iters) and pool["num_estep"] == max(iters) + 1 and pool["num_fitted"] == 4
    assert pool["device_bytes"] > sum(2 * d.num_read for d in datas)


def test_the_pooled_fit_on_the_device_is_the_restatements(planted):
    datas, co, noms = planted
    want, wpool = co.pooled_fit(noms)
    # no seeded M-step value sits on a float32 rounding boundary: the device's s differs from the restatement's by about
    # 1e-13 relative, the distance to the nearest boundary is asked to be a thousand times that
    for u in wpool["unrounded"]:
        f = u.astype(np.float32)
        lo, hi = np.nextafter(f, np.float32(0)).astype(np.float64), np.nextafter(f, np.float32(2)).astype(np.float64)
        mid = np.minimum(np.abs(u - (f + lo) / 2), np.abs(u - (f + hi) / 2))
        assert np.all(mid > 1e-10 * u), (u, mid)
    got, gpool = vb.errfit_cohort(datas, noms, pooled=True)
    print("pooled: %d iterations, summed LRT %.1f, FREEMIX %s -> %s" % (gpool["num_iter"], gpool["lrt_sum"],
          [round(n["alpha"], 5) for n in noms], [round(f["alpha_fit"], 5) for f in got]))
    assert gpool["iter_err"].tobytes() == wpool["iter_err"].tobytes() and np.array_equal(gpool["err"], wpool["err"])
    assert np.array_equal(gpool["n"], wpool["n"]) and gpool["num_iter"] == wpool["num_iter"] and gpool["converged"]
    for q in np.nonzero(wpool["n"])[0]:
        assert abs(gpool["s"][q] - wpool["s"][q]) <= LLK_RTOL * wpool["s"][q] + float(wpool["n"][q]) * 2.0 ** -64
    for g, w in zip(got, want):
        _fit_close(g, w)
    assert abs(gpool["lrt_sum"] - wpool["lrt_sum"]) <= 2 * LLK1_RTOL * sum(abs(w["llk_fit"]) + abs(w["llk_nominal"]) for w in want)
    assert gpool["num_bin"] == 3 and gpool["num_estep"] == wpool["num_estep"] and gpool["num_step"] == wpool["num_step"]


def test_a_sample_that_failed_its_own_run_is_absent_from_the_pool(planted):
    """Sample 2 is handed over as one whose own run ended VB2_ERR_SANITY (what too little depth gives a cohort's sample): it
    never enters, its row carries the code, and the others' results are those of a pool without it."""
    datas, co, noms = planted
    status = [0, 0, _abi.VB2_ERR_SANITY, 0]
    got, gpool = vb.errfit_cohort([datas[0], datas[1], None, datas[3]], [noms[0], noms[1], None, noms[3]], pooled=True,
                                  enter_status=status)
    keep = [0, 1, 3]
    want, wpool = vb.errfit_cohort([datas[i] for i in keep], [noms[i] for i in keep], pooled=True)
    assert got[2]["status"] == _abi.VB2_ERR_SANITY and got[2]["num_iter"] == 0 and not got[2]["n"].any() and np.isnan(got[2]["lrt"])
    assert gpool["num_entered"] == gpool["num_fitted"] == 3 and gpool["num_sample"] == 4
    for i, w in zip(keep, want):
        for key in ("iter_err", "err", "n", "s", "iter_llk", "iter_alpha"):
            assert np.asarray(got[i][key]).tobytes() == np.asarray(w[key]).tobytes(), key
        assert got[i]["status"] == 0 and got[i]["lrt"] == w["lrt"] and got[i]["num_step"] == w["num_step"]
    for key in ("n", "s", "err", "iter_err"):
        assert np.asarray(gpool[key]).tobytes() == np.asarray(wpool[key]).tobytes(), key
    assert gpool["lrt_sum"] == wpool["lrt_sum"]
    # a pool WITH it goes another way
    full, _ = vb.errfit_cohort(datas, noms, pooled=True)
    assert full[0]["iter_err"][0].tobytes() != got[0]["iter_err"][0].tobytes()


# ---- 4. - 5. through the cohort runner and the executable ----
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
FIT_HEADER = ["#SEQ_ID", "FREEMIX", "FREEMIX_FIT", "LRT", "NUM_BIN", "FREELK1_FIT", "FREELK1_NOMINAL", "ITERATIONS", "CONVERGED"]
RATES_HEADER = ["#Q_REPORTED", "READS", "EXPECTED_ERRORS", "ERROR_RATE", "Q_EMPIRICAL", "SE_BINOM"]
POOLED_HEADER = ["#SEQ_ID", "FREEMIX", "FREEMIX_FIT", "LRT", "FREELK1_FIT", "FREELK1_NOMINAL", "STATUS"]


def _write_list(tmp, failing=None, n=6, M=1500):
    """n samples on ONE panel (errfit_ref.sample's, without known allele frequencies), each with its own reads and the rates
    of q - 5 planted in the odd ones; `failing`: that sample covers 100 markers only and fails its own sanity check."""
    base, _ = er.sample(M, 50, known_af=False)
    prefix = vb.synth.write_files(base, str(tmp / "panel"))
    chrs, poss, _, _ = vb.synth.read_bed_rows(prefix + ".bed")
    piles, outs = [], []
    for i in range(n):
        d, _ = er.sample(M, 50, known_af=False, shift=5 if i % 2 else 0)       # the same panel (seed), then other reads:
        rng = np.random.default_rng(500 + i)
        perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(d.read_off[:-1], d.read_off[1:])])
        keep = rng.random(M) < 0.9                                                # and other markers covered
        off = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(np.where(keep, np.diff(d.read_off), 0), out=off[1:])
        take = np.concatenate([perm[d.read_off[m]:d.read_off[m + 1]] for m in np.nonzero(keep)[0]])
        if failing == i:
            off[101:] = off[100]
            take = take[:off[100]]
        p = str(tmp / ("s%d.pileup" % i))
        vb.synth.write_pileup_text(p, chrs, poss, base.meta["ref_base"], off, d.bases[take], d.quals[take])
        piles.append(p)
        outs.append(str(tmp / ("s%d" % i)))
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        for p, o in zip(piles, outs):
            f.write("%s\t%s\n" % (p, o))
    return prefix, piles, outs, lst


def _cli(prefix, extra, out):
    return subprocess.run([CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--Output", out] + extra, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=600)


def test_a_sample_that_fails_its_own_run_through_the_cohort_runner(tmp_path):
    """Sample 2 covers 100 markers and fails its own run (VB2_ERR_SANITY, as the failing sample of test_source_gpu.py): it is
    absent from the pool, the others' results equal a pool without it, and its row carries its status."""
    prefix, piles, outs, lst = _write_list(tmp_path, failing=2, n=4)
    res, fit = vb.run_cohort_files(prefix, piles, output_prefixes=outs, num_pc=2, cohort_fit_error=True, pooled_error=True,
                                   sources_prefix=str(tmp_path / "with"))
    assert [r["status"] for r in res] == [0, 0, _abi.VB2_ERR_SANITY, 0]
    keep = [0, 1, 3]
    res3, fit3 = vb.run_cohort_files(prefix, [piles[i] for i in keep], num_pc=2, cohort_fit_error=True, pooled_error=True)
    bad = fit["fits"][2]
    assert bad["status"] == _abi.VB2_ERR_SANITY and bad["num_iter"] == 0 and not bad["n"].any() and np.isnan(bad["lrt"])
    assert fit["pool"]["num_entered"] == fit["pool"]["num_fitted"] == 3 and fit["pool"]["num_sample"] == 4
    for key in ("n", "s", "err", "iter_err", "iter_change"):
        assert np.asarray(fit["pool"][key]).tobytes() == np.asarray(fit3["pool"][key]).tobytes(), key
    assert fit["pool"]["lrt_sum"] == fit3["pool"]["lrt_sum"]
    for i, w in zip(keep, fit3["fits"]):
        g = fit["fits"][i]
        for key in ("iter_err", "err", "n", "s", "iter_llk", "iter_alpha"):
            assert np.asarray(g[key]).tobytes() == np.asarray(w[key]).tobytes(), key
        assert g["status"] == 0 and g["lrt"] == w["lrt"]
    rows = [ln.split("\t") for ln in open(str(tmp_path / "with.PooledFit")).read().splitlines()]
    assert rows[0] == POOLED_HEADER and len(rows) == 5
    assert rows[3] == [piles[2], "NA", "NA", "NA", "NA", "NA", str(_abi.VB2_ERR_SANITY)]
    assert all(r[6] == "0" for i, r in enumerate(rows[1:]) if i != 2)
    assert not os.path.exists(outs[2] + ".ErrorFit") and not os.path.exists(outs[2] + ".selfSM")


def test_end_to_end_cohort_fit_error(tmp_path):
    prefix, piles, outs, lst = _write_list(tmp_path)
    out = str(tmp_path / "run")
    plain = _cli(prefix, ["--PileupList", lst], out)
    assert plain.returncode == 0, plain.stderr[-2000:]
    own = [o + ext for o in outs for ext in (".selfSM", ".Ancestry")]
    before = [open(p, "rb").read() for p in own]
    assert not any(os.path.exists(o + ".ErrorFit") for o in outs)
    # per sample: the files of six --FitError runs, byte for byte
    fitted = _cli(prefix, ["--PileupList", lst, "--CohortFitError"], out)
    assert fitted.returncode == 0, fitted.stderr[-2000:]
    assert fitted.stdout == plain.stdout and [open(p, "rb").read() for p in own] == before
    notices = [ln for ln in fitted.stderr.decode().splitlines() if "--CohortFitError" in ln]
    assert len(notices) == 1 and notices[0].startswith("NOTICE - --CohortFitError: the error rates of 6 of 6 samples"), notices
    assert not os.path.exists(out + ".PooledFit") and not os.path.exists(out + ".ErrorRates")
    for i, o in enumerate(outs):
        single = _cli(prefix, ["--PileupFile", piles[i], "--FitError"], str(tmp_path / ("one%d" % i)))
        assert single.returncode == 0, single.stderr[-2000:]
        for ext in (".ErrorFit", ".ErrorRates"):
            got, want = open(o + ext).read(), open(str(tmp_path / ("one%d" % i)) + ext).read()
            assert got == want, (i, ext, got, want)
        lines = open(o + ".ErrorFit").read().splitlines()
        assert len(lines) == 2 and lines[0].split("\t") == FIT_HEADER
        assert open(o + ".ErrorRates").read().splitlines()[0].split("\t") == RATES_HEADER
        os.remove(o + ".ErrorFit")
        os.remove(o + ".ErrorRates")
    # pooled: one table and one row per sample
    pooled = _cli(prefix, ["--PileupList", lst, "--CohortFitError", "--PooledError"], out)
    assert pooled.returncode == 0, pooled.stderr[-2000:]
    assert pooled.stdout == plain.stdout and [open(p, "rb").read() for p in own] == before
    assert not any(os.path.exists(o + ".ErrorFit") for o in outs)
    notices = [ln for ln in pooled.stderr.decode().splitlines() if "--PooledError" in ln]
    assert len(notices) == 1 and "one error table for 6 of 6 samples, 3 qualities fitted in" in notices[0] and "summed LRT" in notices[0]
    rates = [ln.split("\t") for ln in open(out + ".ErrorRates").read().splitlines()]
    assert rates[0] == RATES_HEADER and [r[0] for r in rates[1:]] == ["20", "30", "37"]
    rows = [ln.split("\t") for ln in open(out + ".PooledFit").read().splitlines()]
    assert rows[0] == POOLED_HEADER and len(rows) == 7 and all(r[6] == "0" for r in rows[1:])
    res, fit = vb.run_cohort_files(prefix, piles, num_pc=2, cohort_fit_error=True, pooled_error=True)
    g = lambda x: "%g" % x
    for r, rr, f in zip(rows[1:], res, fit["fits"]):
        assert r[1:6] == [g(min(rr["alpha"], 1 - rr["alpha"])), g(f["freemix_fit"]), g(f["lrt"]), g(f["llk_fit"]), g(f["llk_nominal"])]
    for r in rates[1:]:
        q, e, n = int(r[0]), fit["pool"]["err"][int(r[0])], fit["pool"]["n"][int(r[0])]
        assert r[1:] == [str(n), g(fit["pool"]["s"][q]), g(e), g(-10 * np.log10(e)), g(np.sqrt(e * (1 - e) / n))]
    # the odd samples carry the planted shift, the pooled table sits between the two kinds
    assert fit["pool"]["lrt_sum"] > 50 and fit["pool"]["converged"]
    # --ErrorTable <Output>.ErrorRates on one sample alone: its pooled FREEMIX_FIT to the digits printed, and its FREELK1_FIT
    def selfsm(prefix_):
        lines_ = open(prefix_ + ".selfSM").read().splitlines()
        return dict(zip(lines_[0].split("\t"), lines_[1].split("\t")))
    for i in (1, 4):
        one = str(tmp_path / ("table%d" % i))
        under = _cli(prefix, ["--PileupFile", piles[i], "--ErrorTable", out + ".ErrorRates"], one)
        assert under.returncode == 0, under.stderr[-2000:]
        cols = selfsm(one)
        print("sample %d under the pooled table: FREEMIX %s (pooled fit %s, nominal %s), FREELK1 %s (pooled fit %s)"
              % (i, cols["FREEMIX"], rows[1 + i][2], rows[1 + i][1], cols["FREELK1"], rows[1 + i][4]))
        assert cols["FREEMIX"] == rows[1 + i][2] and cols["FREELK1"] == rows[1 + i][4]
        assert cols["FREEMIX"] != rows[1 + i][1]                                   # (not the nominal estimate)
        notes = [ln for ln in under.stderr.decode().splitlines() if "--ErrorTable" in ln]
        assert notes == ["NOTICE - --ErrorTable: the error rates of 3 qualities taken from %s.ErrorRates, the others nominal" % out]
    # ... and on the whole list
    lst2 = str(tmp_path / "list2.txt")
    outs2 = [str(tmp_path / ("t%d" % i)) for i in range(len(piles))]
    open(lst2, "w").write("".join("%s\t%s\n" % (p, o) for p, o in zip(piles, outs2)))
    under = _cli(prefix, ["--PileupList", lst2, "--ErrorTable", out + ".ErrorRates"], out + "t")
    assert under.returncode == 0, under.stderr[-2000:]
    for i, o in enumerate(outs2):
        cols = selfsm(o)
        assert cols["FREEMIX"] == rows[1 + i][2] and cols["FREELK1"] == rows[1 + i][4], (i, cols, rows[1 + i])
    # without the flag nothing changes; a table that lists no quality is the nominal one, byte for byte
    header_only = str(tmp_path / "nominal.ErrorRates")
    open(header_only, "w").write("\t".join(RATES_HEADER) + "\n")
    a, b = str(tmp_path / "plain1"), str(tmp_path / "nominal1")
    p1, p2 = _cli(prefix, ["--PileupFile", piles[1]], a), _cli(prefix, ["--PileupFile", piles[1], "--ErrorTable", header_only], b)
    assert p1.returncode == 0 and p2.returncode == 0 and p1.stdout == p2.stdout
    assert open(a + ".selfSM", "rb").read() == open(outs[1] + ".selfSM", "rb").read()
    for ext in (".selfSM", ".Ancestry"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read()
    # --ErrorPrior reaches the fit
    heavy = _cli(prefix, ["--PileupList", lst, "--CohortFitError", "--PooledError", "--ErrorPrior", "1000000"], out + "h")
    assert heavy.returncode == 0
    assert float(open(out + "h.ErrorRates").read().splitlines()[1].split("\t")[3]) != float(rates[1][3])
