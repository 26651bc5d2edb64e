"""The single-sample file flow end to end on the MI355X, per entry point: vb2_run, vb2_run_interval, vb2_run_replicates,
vb2_run_refbias, and vb2_run over two marker shards of one device, on the bundled golden pileup with the hapmap panel at
--NumPC 2 (what test_cli_reproduces_reference_ctest reads).

* Every entry in a child process with notices on: stdout and the NOTICE lines of stderr, in order, against
  tests/golden/run_notices.json -- the seconds of every `[... seconds ...]` bracket and the device's name after "upload to"
  masked --, and every file the run writes by its sha256 in the same fixture.
* A stage that cannot open its file ends the run with VB2_ERR_IO and the text the fixture holds (no .Pileup asked for:
  the stage's file is the first the run opens), and a vb2_run in the same process afterwards writes the golden files.
* A sample that fails its sanity check: VB2_ERR_SANITY, <prefix>.Pileup written, <prefix>.selfSM not.

The fixture was recorded on the parent of the commit that moved the file flow out of abi.cpp into run.cpp:
tests/golden/make_run_notices.py on a machine with the device.
"""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "run_notices.json")
PANEL = os.path.join(GOLDEN_DIR, "hapmap", "hapmap_3.3.b37.dat")
PILEUP = os.path.join(GOLDEN_DIR, "expected", "result.Pileup")

pytestmark = pytest.mark.gpu

CASES = {
    "run": dict(entry="run", files={"run.Ancestry", "run.selfSM", "run.Pileup"}),
    "interval": dict(entry="interval", files={"run.Ancestry", "run.selfSM", "run.Pileup", "run.CI"}),
    "replicates": dict(entry="replicates", files={"run.Ancestry", "run.selfSM", "run.Pileup", "run.Chrom", "run.Boot"}),
    "refbias": dict(entry="refbias", files={"run.Ancestry", "run.selfSM", "run.Pileup", "run.RefBias"}),
    "shards": dict(entry="run", devices=[0, 0], files={"run.Ancestry", "run.selfSM", "run.Pileup"}),
}


def call(entry, prefix, notices=True, disable_sanity=True, devices=None, output_pileup=True):
    """(return code, vb2_last_error, vb2_run_result) of one entry point on the golden input."""
    L = _abi.lib()
    args, keep = vb.api._run_args(PANEL, PILEUP, 2, disable_sanity, None, prefix, output_pileup=output_pileup, devices=devices)
    args.model.notices = int(notices)
    res = _abi.RunResult()
    if entry == "run":
        rc = L.vb2_run(C.byref(args), C.byref(res))
    elif entry == "interval":
        ci = _abi.Interval()
        rc = L.vb2_run_interval(C.byref(args), C.byref(res), C.byref(ci))
    elif entry == "replicates":
        summary = _abi.ReplicateSummary()
        rc = L.vb2_run_replicates(C.byref(args), 1, 4, C.byref(res), C.byref(summary))
    else:
        fit = _abi.RefBiasFit()
        rc = L.vb2_run_refbias(C.byref(args), C.byref(res), C.byref(fit))
    del keep
    return rc, L.vb2_last_error().decode(), res


def mask(text):
    text = re.sub(r"[-+.0-9eE]+ seconds", "T seconds", text)
    return re.sub(r"(upload to )(?!\d+ devices \().*?(  \[)", r"\1<DEVICE>\2", text)


def sha_files(d):
    return {f: hashlib.sha256(open(os.path.join(str(d), f), "rb").read()).hexdigest() for f in sorted(os.listdir(str(d)))}


def run_case(name, d):
    """Case `name` in a child process whose working directory is d (the prefix is relative: no line names a directory)."""
    case = CASES[name]
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_run_pipeline_gpu as t; "
            "rc, err, _ = t.call(%r, 'run', devices=%r); assert rc == 0, (rc, err)"
            % (ROOT, os.path.join(ROOT, "tests"), case["entry"], case.get("devices")))
    p = subprocess.run([sys.executable, "-c", code], cwd=str(d), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    notices = [ln for ln in mask(p.stderr).splitlines() if ln.startswith("NOTICE")]
    return dict(stdout=mask(p.stdout).splitlines(), notices=notices, files=sha_files(d))


def record(tmp):
    """What tests/golden/run_notices.json holds (tests/golden/make_run_notices.py)."""
    out = {}
    for name in sorted(CASES):
        d = os.path.join(str(tmp), name)
        os.mkdir(d)
        out[name] = run_case(name, d)
    for entry in ("refbias", "replicates"):
        rc, err, _ = call(entry, "no_such_directory/run", notices=False, output_pileup=False)
        out["fails." + entry] = dict(rc=rc, error=err)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_runs_text_and_files_are_the_recorded_ones(golden, tmp_path, name):
    got, want = run_case(name, tmp_path), golden[name]
    assert set(got["files"]) == CASES[name]["files"]
    assert got["stdout"] == want["stdout"]
    assert got["notices"] == want["notices"]
    assert got["files"] == want["files"]


def test_a_stage_that_fails_ends_the_run_cleanly(golden, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for entry in ("refbias", "replicates"):
        rc, err, _ = call(entry, "no_such_directory/run", notices=False, output_pileup=False)
        assert rc == _abi.VB2_ERR_IO
        assert (rc, err) == (golden["fails." + entry]["rc"], golden["fails." + entry]["error"])
        assert err.startswith("Open file no_such_directory/run.") and err.endswith(" failed!")
    assert golden["fails.refbias"]["error"] == "Open file no_such_directory/run.RefBias failed!"
    assert golden["fails.replicates"]["error"] == "Open file no_such_directory/run.Chrom failed!"
    rc, err, res = call("run", "run", notices=False)
    assert rc == _abi.VB2_OK, err
    assert sha_files(tmp_path) == golden["run"]["files"]
    with open(os.path.join(GOLDEN_DIR, "expected", "result.Ancestry"), "rb") as f:
        assert open("run.Ancestry", "rb").read() == f.read()
    with open(os.path.join(GOLDEN_DIR, "expected", "result.selfSM")) as f:
        want = f.read().splitlines()[1].split("\t")
    got = open("run.selfSM").read().splitlines()[1].split("\t")
    assert got[6:9] == want[6:9]                              # FREEMIX, FREELK1, FREELK0 of the reference's own run


def test_the_sanity_failure_path_keeps_its_side_effects(tmp_path, monkeypatch):
    """The golden pileup covers 15 markers: with the sanity check on the load fails, after the .Pileup is written."""
    monkeypatch.chdir(tmp_path)
    rc, err, _ = call("run", "run", notices=False, disable_sanity=False)
    assert rc == _abi.VB2_ERR_SANITY
    assert err == "Insufficient Available markers, check input bam depth distribution in output pileup file after specifying --OutputPileup"
    assert sorted(os.listdir(str(tmp_path))) == ["run.Pileup"]
    with open(PILEUP, "rb") as f:
        assert open("run.Pileup", "rb").read() == f.read()
