"""The cohort runner's after-run stages end to end on the MI355X, in both pipeline modes (VB2_COHORT_STREAM 1 and 0): what
the existing suites of the six flags leave open.

* Every flag set of FLAGS through the command line, on test_paired_gpu's cohort (six samples of 3 000 markers x 30, k = 2,
  and a seventh that fails its sanity check): the notices on stderr against tests/golden/cohort_stages_notices.json --
  `[... seconds]` and the directory masked; every line as a sorted multiset (reader, device and releaser threads write their
  lines in whatever order they run), and the lines of the after-run stages, which one thread writes, in sequence.
* Every file two runs of the table both write is byte for byte the same file, for ALL pairs of the table, and so is stdout.
* In process, three slots or groups of three: an entry point that is given no result arrays but prefixes writes the files
  of one that is given them ("borrow the caller's arrays or make room").
* A pair whose normal fails: the run is VB2_OK and a second identical run in the same process writes identical files (a
  tumour's parked context that were never released would still hold its slab and its streams).

The golden text was recorded on the parent of the commit that split cohort.cpp into the pipeline and its stages:
`PYTHONPATH=. python tests/test_cohort_stages_gpu.py <out.json>` on a machine with the device.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paired_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cohort_stages_notices.json")

pytestmark = pytest.mark.gpu

FLAGS = {
    "plain": [],
    "source": ["--FindSource"],
    "source_interval": ["--FindSource", "--CohortInterval"],
    "source_refit": ["--FindSource", "--RefitSource"],
    "related": ["--FindRelated"],
    "related_source": ["--FindRelated", "--FindSource"],
    "paired": ["--MatchedNormal", "PAIRS"],
    "paired_interval": ["--MatchedNormal", "PAIRS", "--PairInterval"],
}
MODES = {"stream": "1", "groups": "0"}
# written by the calling thread after the pipeline's threads are joined: their sequence is part of the contract
STAGE_LINE = re.compile(r"phase: (Refit|Intervals) given|--RefitSource: |--MatchedNormal: (pair|the contexts)|--PairInterval: |"
                        r"--FindRelated: sample \d+ failed|cohort of \d+ samples")


def normalise(stderr, tmp):
    text = stderr.decode().replace(str(tmp), "<TMP>")
    return re.sub(r"\[[-+.0-9eE]+ seconds\]", "[T seconds]", text).splitlines()


class Cohort:
    """The cohort's files, written once, and the command-line runs of the table, each made when first asked for in a
    directory of its own with relative prefixes -- so that two runs' files of one name are comparable byte for byte."""

    def __init__(self, tmp):
        from test_paired_gpu import _write_cohort
        self.tmp = tmp
        self.data, self.prefix, self.piles, self.outs, _ = _write_cohort(tmp, extra_failing=True)
        self.bad = len(self.piles) - 1
        self.pairs = str(tmp / "pairs.txt")
        with open(self.pairs, "w") as f:                     # the second tumour's normal is the sample that fails
            f.write("%s\t%s\n%s\t%s\n" % (self.piles[0], self.piles[1], self.piles[2], self.piles[self.bad]))
        self.lst = str(tmp / "relative.txt")
        with open(self.lst, "w") as f:
            for p, o in zip(self.piles, self.outs):
                f.write("%s\t%s\n" % (p, os.path.basename(o)))
        self.runs = {}

    def run(self, name, mode):
        if (name, mode) not in self.runs:
            d = self.tmp / ("%s.%s" % (name, mode))
            d.mkdir()
            args = [CLI, "--SVDPrefix", self.prefix, "--Reference", "none.fa", "--PileupList", self.lst, "--Output", "run"]
            args += [self.pairs if a == "PAIRS" else a for a in FLAGS[name]]
            p = subprocess.run(args, env=dict(os.environ, VB2_COHORT_STREAM=MODES[mode]), cwd=str(d), stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=120)
            # (the sample that fails its sanity check makes the command line end with EXIT_FAILURE after a complete run)
            assert p.returncode == 1 and b"FATAL" not in p.stderr, p.stderr[-2000:]
            files = {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}
            self.runs[(name, mode)] = dict(stdout=p.stdout, lines=normalise(p.stderr, self.tmp), files=files)
        return self.runs[(name, mode)]


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    return Cohort(tmp_path_factory.mktemp("cohort_stages"))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(FLAGS))
def test_notices_are_the_recorded_ones(cohort, name, mode):
    want = json.load(open(GOLDEN))["%s.%s" % (name, mode)]
    got = cohort.run(name, mode)["lines"]
    assert sorted(got) == sorted(want)
    assert [ln for ln in got if STAGE_LINE.search(ln)] == [ln for ln in want if STAGE_LINE.search(ln)]


EXPECTED_FILES = {"plain": set(), "source": {"run.Sources"}, "source_interval": {"run.Sources", "CI"},
                  "source_refit": {"run.Sources", "run.SourceFit"}, "related": {"run.Related"},
                  "related_source": {"run.Related", "run.Sources"}, "paired": {"run.PairFit"},
                  "paired_interval": {"run.PairFit", "run.PairCI"}}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_file_two_runs_share_is_the_same_file(cohort, mode):
    runs = {name: cohort.run(name, mode) for name in sorted(FLAGS)}
    good = [os.path.basename(o) for i, o in enumerate(cohort.outs) if i != cohort.bad]
    for name, r in runs.items():
        want = {g + ext for g in good for ext in (".selfSM", ".Ancestry")} | (EXPECTED_FILES[name] - {"CI"})
        if "CI" in EXPECTED_FILES[name]:
            want |= {g + ".CI" for g in good}
        assert set(r["files"]) == want, name
        assert all(len(b) > 0 for b in r["files"].values()), name
    names = sorted(runs)
    compared = 0
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert runs[a]["stdout"] == runs[b]["stdout"], (a, b)
            for f in set(runs[a]["files"]) & set(runs[b]["files"]):
                assert runs[a]["files"][f] == runs[b]["files"][f], (a, b, f)
                compared += 1
    assert compared >= 28 * 12


# ---- in process: no result arrays, but prefixes ----

def _bare_call(kind, cohort, outs, prefix, pairs):
    """Entry point `kind` with every optional result array null."""
    S = len(cohort.piles)
    args, keep = vb.api._run_args(cohort.prefix, cohort.piles[0], 2, False, None, prefix)
    ca = _abi.CohortArgs()
    ca.base = args
    ca.num_sample = S
    piles = (C.c_char_p * S)(*[p.encode() for p in cohort.piles])
    prefs = (C.c_char_p * S)(*[o.encode() for o in outs])
    ca.pileup_paths, ca.output_prefixes, ca.group_size = piles, prefs, 3
    res, status = (_abi.RunResult * S)(), (C.c_int32 * S)()
    L = _abi.lib()
    tum = np.array([p[0] for p in pairs], dtype=np.int32)
    nrm = np.array([p[1] for p in pairs], dtype=np.int32)
    pt = lambda x: x.ctypes.data_as(C.c_void_p)
    if kind == "source":
        rc = L.vb2_cohort_run_sources(C.byref(ca), 3, res, status, None, None)
    elif kind == "source_interval":
        rc = L.vb2_cohort_run_intervals(C.byref(ca), 3, res, status, None)
    elif kind == "source_refit":
        rc = L.vb2_cohort_run_source_fits(C.byref(ca), 3, res, status, None, None, None)
    elif kind == "related":
        rc = L.vb2_cohort_run_related(C.byref(ca), 3, 0, res, status, None, None)
    elif kind == "paired":
        rc = L.vb2_cohort_run_paired(C.byref(ca), len(pairs), pt(tum), pt(nrm), 0.99, res, status, None)
    else:
        rc = L.vb2_cohort_run_paired_intervals(C.byref(ca), len(pairs), pt(tum), pt(nrm), 0.99, res, status, None, None)
    del keep
    return rc, [int(s) for s in status]


KW = {"source": dict(find_source=True), "source_interval": dict(find_source=True, confidence_interval=True),
      "source_refit": dict(find_source=True, refit_source=True), "related": dict(find_related=True),
      "paired": dict(), "paired_interval": dict(pair_interval=True)}


def _files(d):
    return {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}


@pytest.mark.parametrize("stream", [1, 0])
@pytest.mark.parametrize("kind", sorted(KW))
def test_a_caller_without_result_arrays_gets_the_same_files(cohort, tmp_path, tunable, kind, stream):
    tunable("cohort_stream", stream)
    pairs = [(0, 1), (2, cohort.bad)]
    cwd = os.getcwd()
    got = {}
    for who in ("arrays", "bare"):
        d = tmp_path / who
        d.mkdir()
        os.chdir(str(d))                                      # (relative prefixes: the files name them)
        try:
            outs = [os.path.basename(o) for o in cohort.outs]
            if who == "bare":
                rc, status = _bare_call(kind, cohort, outs, "run", pairs)
                assert rc == _abi.VB2_OK
            else:
                kw = dict(KW[kind], matched_normal=pairs) if kind.startswith("paired") else KW[kind]
                res = vb.run_cohort_files(cohort.prefix, cohort.piles, outs, num_pc=2, group_size=3, sources_prefix="run", **kw)
                status = [r["status"] for r in (res[0] if isinstance(res, tuple) else res)]
        finally:
            os.chdir(cwd)
        assert status == [_abi.VB2_ERR_SANITY if s == cohort.bad else 0 for s in range(len(cohort.piles))]
        got[who] = _files(d)
    assert set(got["bare"]) == set(got["arrays"]) and len(got["bare"]) >= 13
    for f in got["arrays"]:
        assert got["bare"][f] == got["arrays"][f], f


@pytest.mark.parametrize("stream", [1, 0])
@pytest.mark.parametrize("interval", [False, True])
def test_a_tumour_whose_normal_fails_is_released(cohort, tmp_path, tunable, stream, interval):
    tunable("cohort_stream", stream)
    got = []
    for turn in range(2):
        d = tmp_path / ("turn%d" % turn)
        d.mkdir()
        outs = [str(d / os.path.basename(o)) for o in cohort.outs]
        res, fits = vb.run_cohort_files(cohort.prefix, cohort.piles, outs, num_pc=2, group_size=3, sources_prefix=str(d / "run"),
                                        matched_normal=[(0, 1), (2, cohort.bad)], pair_interval=interval)      # VB2_OK, or it raises
        assert res[cohort.bad]["status"] == _abi.VB2_ERR_SANITY and res[2]["status"] == 0
        assert fits[0]["status"] == 0 and fits[1]["status"] == _abi.VB2_PAIR_FIT_NONE
        got.append({f: b.replace(str(d).encode(), b"<DIR>") for f, b in _files(d).items()})
    assert got[0] == got[1] and ("run.PairCI" in got[0]) == interval and "run.PairFit" in got[0]


if __name__ == "__main__":                                    # record the golden notices (see the module's docstring)
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        c = Cohort(pathlib.Path(t))
        out = {"%s.%s" % (n, m): c.run(n, m)["lines"] for n in sorted(FLAGS) for m in sorted(MODES)}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
