"""The error-rate fit on the GPU: contexts under an error table, the E-step
kernel, the fit on the device against the procedure over the float64 restatement, and the command line.

Evaluations and sums are held to the project's LLK_RTOL = 1e-12 against the 80-bit restatement (tests/errfit_ref.py), s[q]
with the fixed-point scheme's own bound n[q] 2^-64 added; n[q] is compared exactly.  The worst deviations are printed at the
module's end (pytest -s).  Measured on an MI355X:

    evaluation, layout 1 (probability domain)  2.2e-16  (1 x 2, entries of 0 and 1, alpha = 1e-6)
    evaluation, layout 0 (run words)           2.0e-16  (300 x 30 wide alphabet, entries of 0 and 1, alpha = 1)
    derivatives' and marginals' llk            0        (300 x 2, shifted table)
    vb2_errstat_eval  s[q] beyond n[q] 2^-64   2.0e-13  (17 x 600, alpha = 0.03, q 34)
    vb2_errstat_eval  llk                      1.1e-15  (17 x 600, alpha = 0.03)

The fit on the device (1 000 x 30, the rates of q - 5 planted, seed 11): FREEMIX 0.03596 -> 0.03046, LRT 255.1, 9 iterations,
every iteration's table the restatement's bit for bit.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errfit_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
LLK_RTOL = 1e-12                  # the project's evaluation tolerance (tests/test_gpu_parity.py)
ALPHAS = [0.0, 1e-6, 0.03, 0.5, 1.0]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for what in sorted(_WORST):
        print("\n%s: worst |kernel - restatement| / |restatement| = %.3g (%s)" % ((what,) + _WORST[what]))


def _close(got, want, what, label, extra=0.0):
    """test_conditioned_gpu._close; extra: an absolute bound added to the relative one."""
    want = float(want)
    over = max(0.0, abs(got - want) - extra)              # (what the absolute bound does not cover)
    rel = over / abs(want) if want != 0 else over
    if rel > _WORST.get(what, (-1.0, ""))[0]:
        _WORST[what] = (rel, label)
    assert abs(got - want) <= LLK_RTOL * abs(want) + extra, (label, got, want, rel)


@pytest.fixture
def layout(request):
    """pd = 1: the probability domain where the sample allows it; 0: run words."""
    old = _abi.get_tunable("pd")
    _abi.set_tunable("pd", request.param)
    yield request.param
    _abi.set_tunable("pd", old)


def _digest(ctx):
    v = C.c_ulonglong(0)
    _abi.check(_abi.lib().vb2_debug_layout_digest(ctx._h, C.byref(v)), "vb2_debug_layout_digest")
    return v.value


def _points(k, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, (len(ALPHAS), k)), rng.normal(0, scale, (len(ALPHAS), k)), np.array(ALPHAS)


def _shifted(d, by=5):
    """Every present quality's rate that of q - by (at most 1)."""
    t = vb.nominal_err_table()
    for q in np.unique(np.clip(d.quals.astype(np.int64) - 33, 0, 93)):
        t[q] = min(1.0, 10.0 ** (-(int(q) - by) / 10.0))
    return t


def _zero_one(d):
    """The two most frequent qualities at rates 0 and 1."""
    q = np.bincount(np.clip(d.quals.astype(np.int64) - 33, 0, 93), minlength=94).argsort()[::-1]
    t = vb.nominal_err_table()
    t[q[0]], t[q[1]] = 0.0, 1.0
    return t


def _make(M, k, seed=21, known_af=False, **kw):
    d = vb.synth.make_pileup(M, mean_depth=30 if M > 1 else 40, num_pc=k, alpha_true=0.05, seed=seed, **kw)
    if known_af:
        d.known_af = np.clip(d.means / 2.0 + np.random.default_rng(1).normal(0, 0.02, M), 0.0, 1.0)
    return d


# ---- 1. NULL and the nominal table are vb2_ctx_create ----
@pytest.mark.parametrize("layout", [1, 0], indirect=True)
def test_null_and_nominal_tables_are_the_plain_context(layout):
    d = _make(3000, 2)
    p1, p2, a = _points(2, 1)
    with vb.LikelihoodContext(d) as plain:
        want, digest, lay = plain.llk(p1, p2, a), _digest(plain), plain.info()["layout"]
    assert lay == layout
    h = C.c_void_p()
    inp, opt = d.as_input(), _abi.Options(-1, 0, None)
    _abi.check(_abi.lib().vb2_ctx_create_ex(C.byref(inp), C.byref(opt), None, C.byref(h)), "vb2_ctx_create_ex")
    null = vb.LikelihoodContext.__new__(vb.LikelihoodContext)
    null._lib, null.data, null.num_pc, null._h = _abi.lib(), d, 2, h
    with null, vb.LikelihoodContext(d, err_table=vb.nominal_err_table()) as nom:
        for ctx in (null, nom):
            assert _digest(ctx) == digest and ctx.info()["layout"] == lay
            assert ctx.llk(p1, p2, a).tobytes() == want.tobytes()


# ---- 2. evaluation under a table ----
def _check_ctx(d, table, label, seed=3):
    c80 = er.Counts(d, np.longdouble)
    t80 = table.astype(np.longdouble)
    p1, p2, a = _points(d.num_pc, seed)
    with vb.LikelihoodContext(d, err_table=table) as ctx:
        lay = ctx.info()["layout"]
        got = ctx.llk(p1, p2, a)
        for i in range(len(a)):
            _close(got[i], er.llk(c80, t80, p1[i], p2[i], a[i]), "eval layout %d" % lay, "%s alpha %g" % (label, a[i]))
    return lay


@pytest.mark.parametrize("M,k,layout", [(1, 2, 1), (17, 1, 0), (17, 4, 1), (300, 4, 0), (300, 1, 1), (3000, 2, 0), (3000, 2, 1)],
                         indirect=["layout"])
def test_eval_under_a_table_matches_the_restatement(M, k, layout):
    d = _make(M, k)
    assert _check_ctx(d, _shifted(d), "shifted %d x %d" % (M, k)) == layout
    # (a rate of 1 costs the (het, het) term log2 6 bits per read: the probability-domain bound follows the table, and a
    # sample may take run words under it)
    assert _check_ctx(d, _zero_one(d), "zero-one %d x %d" % (M, k)) in (0, layout)


@pytest.mark.parametrize("layout", [1, 0], indirect=True)
def test_eval_under_a_table_known_af_filter_and_wide_alphabet(layout):
    d = _make(300, 2, known_af=True)
    _check_ctx(d, _shifted(d), "known AF")
    d = vb.synth.with_sanity_stats(_make(300, 2, seed=22, missing_frac=0.1))
    _check_ctx(d, _shifted(d), "missing + depth filter")
    d = _make(300, 2, seed=5, q_lo=2, q_hi=60)
    _check_ctx(d, _shifted(d), "wide alphabet")
    _check_ctx(d, _zero_one(d), "wide alphabet zero-one")


@pytest.mark.parametrize("layout", [1, 0], indirect=True)
def test_per_marker_units_follow_the_table(layout):
    import deriv_ref as dr
    d = _make(300, 2)
    table = _shifted(d)
    c80 = er.Counts(d, np.longdouble)
    p1, p2, a = _points(2, 4)
    i = 2
    want = er.llk(c80, table.astype(np.longdouble), p1[i], p2[i], a[i])
    with vb.LikelihoodContext(d, err_table=table) as ctx, vb.LikelihoodContext(d) as plain:
        llk, grad, _ = ctx.derivatives(p1[i], p2[i], a[i])
        _close(llk[0], want, "derivs", "shifted 300 x 2")
        logl = ctx.marginals(p1[i], p2[i], a[i])[2]
        _close(float(np.sum(logl.astype(np.longdouble))), want, "marginals", "shifted 300 x 2")
        # the alpha derivative is the table's too: a central difference of the restatement under the table
        h = 1e-5
        fd = (er.llk(c80, table.astype(np.longdouble), p1[i], p2[i], a[i] + h) -
              er.llk(c80, table.astype(np.longdouble), p1[i], p2[i], a[i] - h)) / (2 * h)
        assert abs(grad[0][4] - float(fd)) <= 1e-5 * abs(float(fd))
        assert abs(plain.derivatives(p1[i], p2[i], a[i])[1][0][4] - float(fd)) > 1e-2 * abs(float(fd))
    del dr


# ---- 3. - 5. the E-step ----
def _check_stats(d, table, alphas, label, seed=6, es=None):
    c80 = er.Counts(d, np.longdouble)
    t80 = table.astype(np.longdouble)
    p1, p2, _ = _points(d.num_pc, seed)
    own = es is None
    es = es or vb.ErrStat(d)
    try:
        for i, alpha in enumerate(alphas):
            n, s, llk = es.eval(table, p1[i], p2[i], alpha)
            n80, s80 = er.stats(c80, t80, p1[i], p2[i], alpha)
            assert np.array_equal(n, n80), (label, alpha)
            for q in np.nonzero(n80)[0]:
                _close(s[q], s80[q], "errstat s", "%s alpha %g q %d" % (label, alpha, q), extra=float(n80[q]) * 2.0 ** -64)
            assert np.all(s[n80 == 0] == 0)
            _close(llk, er.llk(c80, t80, p1[i], p2[i], alpha), "errstat llk", "%s alpha %g" % (label, alpha))
    finally:
        if own:
            es.close()


@pytest.mark.parametrize("M,k,known_af", [(1, 1, False), (257, 4, False), (300, 1, True), (300, 4, False), (3000, 4, False),
                                          (3000, 1, True)])
def test_errstat_matches_the_restatement(M, k, known_af):
    d = _make(M, k, known_af=known_af)
    _check_stats(d, _shifted(d), [0.0, 0.03, 1.0], "%d x %d%s" % (M, k, " known AF" if known_af else ""))
    if M == 300:
        _check_stats(d, _zero_one(d), [0.0, 0.03, 1.0], "zero-one %d x %d" % (M, k))


def _edges():
    """17 x 600 deep: marker 3 has 1 200 reads (its L underflows); the first and the last marker are empty; marker 5 holds
    class-other reads only; the qualities run past 93."""
    d = vb.synth.make_pileup(17, mean_depth=600, num_pc=4, alpha_true=0.05, seed=9, q_lo=20, q_hi=40)
    depth = np.diff(d.read_off)
    depth[0] = depth[16] = 0
    depth[3] = 1200
    depth[5] = 12                     # (600 class-other reads would underflow as well)
    rng = np.random.default_rng(4)
    off = np.zeros(18, dtype=np.int64)
    np.cumsum(depth, out=off[1:])
    R = int(off[-1])
    bases = np.empty(R, dtype=np.uint8)
    quals = np.empty(R, dtype=np.uint8)
    for m in range(17):
        lo, hi, olo = int(off[m]), int(off[m + 1]), int(d.read_off[m])
        take = (olo + np.arange(hi - lo) % max(1, int(d.read_off[m + 1]) - olo)) if hi > lo else np.zeros(0, dtype=np.int64)
        bases[lo:hi] = d.bases[take]
        quals[lo:hi] = d.quals[take]
    # marker 3: half ref, half alt at high quality under both homozygous-leaning frequencies -- and deep enough to underflow
    lo, hi = int(off[3]), int(off[4])
    bases[lo:hi] = np.where(np.arange(hi - lo) % 3 == 0, ord("."), d.alt_base[3])
    other = [b for b in b"ACGT" if b != d.alt_base[5] and b != d.meta["ref_base"][5]][0]
    bases[int(off[5]):int(off[6])] = other
    # qualities above 93 (characters up to 255) on marker 7, quality 0 and below on marker 8
    quals[int(off[7]):int(off[8])] = rng.integers(33 + 90, 256, size=int(off[8] - off[7])).astype(np.uint8)
    quals[int(off[8]):int(off[9]):7] = 30
    return vb.PileupData(4, d.ud, d.means, off, bases, quals, d.alt_base, None, float(R) / 15, 0.0, True, dict(d.meta))


def test_errstat_edges():
    d = _edges()
    table = _shifted(d)
    c = er.Counts(d)
    z = np.zeros(4)
    live = er._markers(c, table, z, z, 0.03)[1]
    assert not live[c.pos[3]] and live[c.pos[5]] and c.pos[0] < 0 and c.pos[16] < 0      # the deep marker underflows
    _check_stats(d, table, [0.0, 0.03, 1.0], "edges 17 x 600")
    with vb.ErrStat(d) as es:
        n = es.eval(table, z, z, 0.03)[0]
        assert n.sum() == d.num_read - 1200 and n[93] > 0 and n[94 - 1] == er.stats(c, table, z, z, 0.03)[0][93]
        for bad in (-1e-9, 1.0000001, float("nan")):
            with pytest.raises(_abi.Vb2Error, match="alpha lies outside"):
                es.eval(table, z, z, bad)
        t = table.copy()
        t[30] = 1.5
        with pytest.raises(_abi.Vb2Error, match="quality 30"):
            es.eval(t, z, z, 0.03)
        assert es.info()["num_launch"] == 2 and es.info()["num_read"] == d.num_read and es.info()["device_bytes"] > 2 * d.num_read
    # all reads at one quality
    one = _make(300, 2, q_lo=30, q_hi=30)
    _check_stats(one, _shifted(one), [0.03], "one quality")
    # the depth filter
    f = vb.synth.with_sanity_stats(_make(300, 2, seed=22, missing_frac=0.1))
    _check_stats(f, _shifted(f), [0.03], "depth filter")


def test_errstat_llk_is_the_contexts():
    d = _make(3000, 2)
    table = _shifted(d)
    p1, p2, a = _points(2, 8)
    with vb.ErrStat(d) as es, vb.LikelihoodContext(d, err_table=table) as ctx:
        want = ctx.llk(p1, p2, a)
        for i in range(len(a)):
            got = es.eval(table, p1[i], p2[i], a[i])[2]
            assert abs(got - want[i]) <= LLK_RTOL * abs(want[i]), (a[i], got, want[i])


def test_errstat_bits_do_not_depend_on_the_grid_or_the_call():
    d = _make(3000, 4)
    table = _shifted(d)
    p1, p2, _ = _points(4, 9)
    old = _abi.get_tunable("errstat_groups")
    try:
        with vb.ErrStat(d) as es:
            got = []
            for groups in (0, 0, 1, 3, 0):
                _abi.set_tunable("errstat_groups", groups)
                n, s, llk = es.eval(table, p1[2], p2[2], 0.03)
                got.append(n.tobytes() + s.tobytes() + np.float64(llk).tobytes())
            assert len(set(got)) == 1 and n.sum() > 0
    finally:
        _abi.set_tunable("errstat_groups", old)


# ---- 6. the fit on the device is the restatement's ----
FIT_SEED = 11


def test_the_fit_on_the_device_is_the_restatements():
    d, planted = er.sample(1000, FIT_SEED)
    ev = er.Evaluator(d)
    want, nom = ev.fit(2, True)
    with vb.LikelihoodContext(d) as ctx:
        dev_nom = ctx.optimize()
    assert abs(dev_nom["alpha"] - nom["alpha"]) <= 1e-4 and dev_nom["num_eval"] == nom["num_eval"]
    got = vb.errfit(d, nom)
    print("1 000 x 30 planted q - 5: FREEMIX %.5f -> %.5f, LRT %.1f, %d iterations" % (nom["alpha"], got["alpha_fit"], got["lrt"],
                                                                                       got["num_iter"]))
    # no seeded value may sit on a float32 rounding boundary: the unrounded M-step values of the restatement
    assert got["num_iter"] == want["num_iter"] and got["converged"] and want["converged"]
    assert got["iter_err"].tobytes() == want["iter_err"].tobytes()
    assert np.array_equal(got["err"], want["err"]) and np.array_equal(got["n"], want["n"])
    for q in np.nonzero(want["n"])[0]:
        assert abs(got["s"][q] - want["s"][q]) <= LLK_RTOL * want["s"][q] + float(want["n"][q]) * 2.0 ** -64
    # alpha and llk1 with the refit tests' own allowances (test_refbias_gpu): the searches stop within about 1e-8 |llk|
    assert np.allclose(got["iter_alpha"], want["iter_alpha"], rtol=0, atol=1e-4)
    assert np.allclose(got["iter_llk"], want["iter_llk"], rtol=1e-6, atol=0)
    assert abs(got["estimate"]["llk1"] - want["estimate"]["llk1"]) <= 1e-6 * abs(want["estimate"]["llk1"])
    assert got["num_step"] == want["num_step"] and got["estimate"]["num_eval"] == want["estimate"]["num_eval"]
    assert got["lrt"] > 100 and got["num_bin"] == 3


# ---- 7. the command line ----
FIT_HEADER = ["#SEQ_ID", "FREEMIX", "FREEMIX_FIT", "LRT", "NUM_BIN", "FREELK1_FIT", "FREELK1_NOMINAL", "ITERATIONS", "CONVERGED"]
RATES_HEADER = ["#Q_REPORTED", "READS", "EXPECTED_ERRORS", "ERROR_RATE", "Q_EMPIRICAL", "SE_BINOM"]


def _run_cli(prefix, out, extra):
    return subprocess.run([CLI, "--SVDPrefix", prefix, "--Reference", "none.fa", "--PileupFile", prefix + ".pileup", "--Output", out,
                           "--DisableSanityCheck"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_end_to_end_fit_error(tmp_path):
    d, _ = er.sample(1000, FIT_SEED, known_af=False)
    prefix = vb.synth.write_files(d, str(tmp_path / "planted"))
    out = str(tmp_path / "run")
    plain = _run_cli(prefix, out, [])
    assert plain.returncode == 0, plain.stderr[-2000:]
    others = [out + ext for ext in (".selfSM", ".Ancestry")]
    before = [open(p, "rb").read() for p in others]
    assert not os.path.exists(out + ".ErrorFit") and not os.path.exists(out + ".ErrorRates")
    fitted = _run_cli(prefix, out, ["--FitError"])
    assert fitted.returncode == 0, fitted.stderr[-2000:]
    assert fitted.stdout == plain.stdout
    assert [open(p, "rb").read() for p in others] == before
    notices = [ln for ln in fitted.stderr.decode().splitlines() if "error rates" in ln]
    assert len(notices) == 1 and notices[0].startswith("NOTICE - FREEMIX "), notices
    assert len(fitted.stderr.splitlines()) == len(plain.stderr.splitlines()) + 1
    res = vb.run_files(prefix, prefix + ".pileup", None, num_pc=2, disable_sanity=True, fit_error=True)
    f = res["error_fit"]
    g = lambda x: "%g" % x
    lines = open(out + ".ErrorFit").read().splitlines()
    assert len(lines) == 2 and lines[0].split("\t") == FIT_HEADER
    selfsm = open(out + ".selfSM").read().splitlines()
    cols = dict(zip(selfsm[0].split("\t"), selfsm[1].split("\t")))
    assert lines[1].split("\t") == [cols["#SEQ_ID"], cols["FREEMIX"], g(f["freemix_fit"]), g(f["lrt"]), "3", g(f["llk_fit"]),
                                    g(f["llk_nominal"]), str(f["num_iter"]), "1"]
    assert f["alpha_nominal"] == res["alpha"] and f["llk_nominal"] == -res["llk1"]
    rows = [ln.split("\t") for ln in open(out + ".ErrorRates").read().splitlines()]
    assert rows[0] == RATES_HEADER and [r[0] for r in rows[1:]] == ["20", "30", "37"]
    for r in rows[1:]:
        q = int(r[0])
        e = f["err"][q]
        assert r[1:] == [str(f["n"][q]), g(f["s"][q]), g(e), g(-10 * np.log10(e)), g(np.sqrt(e * (1 - e) / f["n"][q]))]
    print("end to end: " + "  ".join("%s %s" % (h, v) for h, v in zip(FIT_HEADER, lines[1].split("\t"))))
    assert f["lrt"] > 100 and f["freemix_fit"] < min(res["alpha"], 1 - res["alpha"])
    # --ErrorPrior reaches the fit
    heavy = _run_cli(prefix, out + "h", ["--FitError", "--ErrorPrior", "100000"])
    assert heavy.returncode == 0
    assert float(open(out + "h.ErrorFit").read().splitlines()[1].split("\t")[3]) < f["lrt"]


def test_fit_error_from_bam_input(golden_dir, tmp_path):
    """expected/result.Pileup turned into a BAM, as test_bam_gpu does: both files are written, FREEMIX is .selfSM's."""
    from test_bam_gpu import _cli, _golden_bam
    bam, _ = _golden_bam(golden_dir, str(tmp_path), os.path.join("expected", "result.Pileup"))
    out = str(tmp_path / "r")
    _cli(golden_dir, out, ["--BamFile", bam, "--FitError"])
    lines = open(out + ".ErrorFit").read().splitlines()
    assert len(lines) == 2 and lines[0].split("\t") == FIT_HEADER
    selfsm = open(out + ".selfSM").read().splitlines()
    cols = dict(zip(selfsm[0].split("\t"), selfsm[1].split("\t")))
    row = lines[1].split("\t")
    assert row[0] == cols["#SEQ_ID"] and row[1] == cols["FREEMIX"]
    rates = open(out + ".ErrorRates").read().splitlines()
    assert rates[0].split("\t") == RATES_HEADER and len(rates) - 1 == int(row[4]) > 0
    assert open(out + ".selfSM").read() == open(os.path.join(golden_dir, "expected", "result.selfSM")).read()
