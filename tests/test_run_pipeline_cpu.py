"""The file flow of one sample without a device: what the panel loader and the single-sample load report when files are
broken, pinned on both loaders (vb2_flat_load of a text pileup, and the cohort's: vb2_cohort_run with a one-line list,
which reads its panel before it touches a device).

* The panel files' errors come in the reference's reading order -- .bed, AF file, .UD, .mu -- whatever thread met them
  first; a pileup's error comes after all of them.
* A .UD with more rows than the .bed is VB2_ERR_INVALID ".UD has more rows than .mu/.bed".
* A failing load leaves no helper thread behind: 200 failing loads of every kind in one process, then a good load whose
  arrays are those of a fresh process (a joinable thread that were left behind would have ended the process).

The AF reader takes any text (ContaminationEstimator.cpp:461-487 reads what `>>` gives it): the one error it reports is a
file that cannot be opened, so that is how the AF file is broken here.
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, K = 50, 2
INVALID, IO = _abi.VB2_ERR_INVALID, _abi.VB2_ERR_IO


def write_panel(pre, broken=(), ud_rows=M):
    """A 50-marker, 2-PC panel and a pileup of its first ten markers at <pre>.*; broken: which files are left out (bed,
    mu), cut to one column (ud) or given a line no reader takes (pileup)."""
    if "bed" not in broken:
        with open(pre + ".bed", "w") as f:
            f.write("".join("1\t%d\t%d\tA\tC\n" % (100 * i + 99, 100 * i + 100) for i in range(M)))
    with open(pre + ".UD", "w") as f:
        f.write("".join(("%r\n" % (0.01 * i) if "ud" in broken else "%r\t%r\n" % (0.01 * i, -0.02 * i)) for i in range(ud_rows)))
    if "mu" not in broken:
        with open(pre + ".mu", "w") as f:
            f.write("".join("1:%d_A/C %r\n" % (100 * i + 100, 0.5 + 0.01 * i) for i in range(M)))
    with open(pre + ".pileup", "w") as f:
        f.write("".join("1\t%d\tA\t3\t.,c\tIJK\n" % (100 * i + 100) for i in range(10)))
        if "pileup" in broken:
            f.write("1\t1100\t.\t2\t..\tII\n")
    return pre


def message(kind, pre):
    return {"bed": "Open file:%s.bed\t failed" % pre, "af": "Open file:%s.af\t failed" % pre,
            "ud": "--NumPC should be less than or equal to the number of PCs in SVD files provided by --SVDPrefix! "
                  "(Expected:2 vs Observed:1)",
            "mu": "Open file:%s.mu\t failed" % pre, "rows": ".UD has more rows than .mu/.bed",
            "pileup": "Pileup format error: cannot find ref allele, exit!"}[kind]


def flat_load(pre, af=False):
    """(return code, vb2_last_error) of vb2_flat_load; a loaded sample is freed."""
    L = _abi.lib()
    args, keep = vb.api._run_args(pre, pre + ".pileup", K, True, pre + ".af" if af else None, None)
    h = C.c_void_p()
    rc = L.vb2_flat_load(C.byref(args), C.byref(h))
    err = L.vb2_last_error().decode()
    if h:
        L.vb2_flat_free(h)
    return rc, err


def cohort_load(pre, af=False):
    """(return code, vb2_last_error) of vb2_cohort_run over a list of one line."""
    L = _abi.lib()
    args, keep = vb.api._run_args(pre, pre + ".pileup", K, True, pre + ".af" if af else None, None)
    ca = _abi.CohortArgs()
    ca.base = args
    ca.num_sample = 1
    piles = (C.c_char_p * 1)((pre + ".pileup").encode())
    ca.pileup_paths = piles
    res, status = (_abi.RunResult * 1)(), (C.c_int32 * 1)()
    rc = L.vb2_cohort_run(C.byref(ca), res, status)
    return rc, L.vb2_last_error().decode()


# (what is broken, with an AF file named, whose message and code come out)
ORDER = [(("bed", "ud", "mu"), False, "bed", IO), (("bed", "ud", "mu"), True, "bed", IO),
         (("ud", "mu"), True, "af", IO), (("ud", "mu"), False, "ud", INVALID), (("mu",), False, "mu", IO)]


@pytest.mark.parametrize("load", [flat_load, cohort_load], ids=["flat", "cohort"])
@pytest.mark.parametrize("broken,af,first,code", ORDER, ids=["bed+ud+mu", "bed+af+ud+mu", "af+ud+mu", "ud+mu", "mu"])
def test_panel_errors_come_in_the_references_reading_order(tmp_path, load, broken, af, first, code):
    pre = write_panel(str(tmp_path / "p"), broken)
    assert load(pre, af) == (code, message(first, pre))


def test_ud_with_more_rows_than_the_bed(tmp_path):
    pre = write_panel(str(tmp_path / "p"), ud_rows=M + 1)
    assert flat_load(pre) == (INVALID, message("rows", pre))


def test_a_pileup_error_is_reported_after_the_panels(tmp_path):
    pre = write_panel(str(tmp_path / "p"), ("mu", "pileup"))
    assert flat_load(pre) == (IO, message("mu", pre))
    pre = write_panel(str(tmp_path / "q"), ("pileup",))
    assert flat_load(pre) == (INVALID, message("pileup", pre))
    pre = write_panel(str(tmp_path / "r"))
    assert flat_load(pre)[0] == _abi.VB2_OK


def digest(pre):
    d = vb.PileupData.from_files(pre, pre + ".pileup", K)
    h = hashlib.sha256()
    for a in (d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base):
        h.update(a.tobytes())
    return "%d %d %s" % (d.num_marker, d.num_read, h.hexdigest())


def failing_loads_then_a_good_one(tmp, turns):
    kinds = [(("bed", "ud", "mu"), False, M, "bed", IO), (("ud", "mu"), True, M, "af", IO), (("ud", "mu"), False, M, "ud", INVALID),
             (("mu",), False, M, "mu", IO), ((), False, M + 1, "rows", INVALID), (("pileup",), False, M, "pileup", INVALID)]
    for n, (broken, af, rows, first, code) in enumerate(kinds):
        pre = write_panel(os.path.join(tmp, "k%d" % n), broken, rows)
        for _ in range(turns):
            assert flat_load(pre, af) == (code, message(first, pre)), first
    return digest(write_panel(os.path.join(tmp, "good")))


def test_failing_loads_leave_no_thread_behind(tmp_path):
    def child(what):
        code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_run_pipeline_cpu as t; print(%s)" % (
            ROOT, os.path.join(ROOT, "tests"), what)
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.splitlines()[-1]
    after = child("t.failing_loads_then_a_good_one(%r, 200)" % str(tmp_path))
    fresh = child("t.digest(%r)" % str(tmp_path / "good"))
    assert after == fresh and after.startswith("%d 30 " % M)
