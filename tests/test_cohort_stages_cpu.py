"""The seven cohort entry points' refusals, without a GPU: every one of them comes before a device or a file is touched, so
the exact vb2_last_error text, the return code and the ORDER of the checks are pinned here on arguments that name no
existing file (vb2_cohort_run, _sources, _related, _source_fits, _intervals, _paired, _paired_intervals)."""
import ctypes as C

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

INVALID = _abi.VB2_ERR_INVALID
ONE_DEVICE = {
    "sources": "--FindSource takes one device: a source set is not spread over several --Devices",
    "related": "--FindRelated takes one device: a set of samples is not spread over several --Devices",
    "source_fits": "--RefitSource takes one device: a source set and the refits given it are not spread over several --Devices",
    "intervals": "--CohortInterval takes one device: the intervals of a cohort are not spread over several --Devices",
    "paired": "--MatchedNormal takes one device: the normals' rows and the refits given them are not spread over several --Devices",
    "paired_intervals": "--MatchedNormal takes one device: the normals' rows and the refits given them are not spread over several --Devices",
}
FIX_ALPHA = {
    "source_fits": "--RefitSource cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate",
    "paired": "--MatchedNormal cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate",
    "paired_intervals": "--MatchedNormal cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate",
}
HOM_MIN = "--NormalHomMin takes a probability within [0, 1]"
ENTRIES = ["run"] + sorted(ONE_DEVICE)
PAIRED = ("paired", "paired_intervals")
TOPS = {"sources": ("top",), "related": ("top", "top2"), "source_fits": ("top",), "intervals": ("top",)}


def _invalid(name):
    # (the two paired entry points share their check, and its message names the first)
    return "vb2_cohort_run_%s: invalid argument" % ("paired" if name in PAIRED else name) if name != "run" \
        else "vb2_cohort_run: invalid argument"


class Args:
    """vb2_cohort_args for three samples whose files do not exist, and everything the arrays must outlive."""

    def __init__(self, tmp, num_pc=2, devices=None, num_sample=3, **model_kw):
        self.base, self.keep = vb.api._run_args(str(tmp / "nopanel"), str(tmp / "s.pileup"), 2, True, None, None,
                                                devices=devices, **model_kw)
        self.base.num_pc = num_pc
        self.ca = _abi.CohortArgs()
        self.ca.base = self.base
        self.ca.num_sample = num_sample
        self.piles = (C.c_char_p * 3)(*[str(tmp / ("s%d.pileup" % i)).encode() for i in range(3)])
        self.ca.pileup_paths = self.piles
        self.res, self.status = (_abi.RunResult * 3)(), (C.c_int32 * 3)()


def _call(name, a, ca=True, out=True, status=True, top=0, top2=0, num_pair=1, tumour=(0,), normal=(1,), hom_min=0.99):
    """(return code, vb2_last_error) of entry point `name`; the optional result arrays are all null."""
    L = _abi.lib()
    ca = C.byref(a.ca) if ca else None
    out = a.res if out else None
    status = a.status if status else None
    t = None if tumour is None else np.asarray(tumour, dtype=np.int32)
    n = None if normal is None else np.asarray(normal, dtype=np.int32)
    pt = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    if name == "run":
        rc = L.vb2_cohort_run(ca, out, status)
    elif name == "sources":
        rc = L.vb2_cohort_run_sources(ca, top, out, status, None, None)
    elif name == "related":
        rc = L.vb2_cohort_run_related(ca, top, top2, out, status, None, None)
    elif name == "source_fits":
        rc = L.vb2_cohort_run_source_fits(ca, top, out, status, None, None, None)
    elif name == "intervals":
        rc = L.vb2_cohort_run_intervals(ca, top, out, status, None)
    elif name == "paired":
        rc = L.vb2_cohort_run_paired(ca, num_pair, pt(t), pt(n), hom_min, out, status, None)
    else:
        rc = L.vb2_cohort_run_paired_intervals(ca, num_pair, pt(t), pt(n), hom_min, out, status, None, None)
    return rc, L.vb2_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_null_and_out_of_range_arguments(tmp_path, name):
    want = (INVALID, _invalid(name))
    for null in ("ca", "out", "status"):
        assert _call(name, Args(tmp_path), **{null: False}) == want, null
    for field in ("ud_path", "mean_path", "bed_path"):
        a = Args(tmp_path)
        setattr(a.ca.base, field, None)
        assert _call(name, a) == want, field
    a = Args(tmp_path)
    a.ca.pileup_paths = None
    assert _call(name, a) == want
    for num_sample in (0, -1):
        assert _call(name, Args(tmp_path, num_sample=num_sample)) == want
    for num_pc in (0, -1, _abi.VB2_MAX_PC + 1):
        assert _call(name, Args(tmp_path, num_pc=num_pc)) == want, num_pc
    for key in TOPS.get(name, ()):
        assert _call(name, Args(tmp_path), **{key: -1}) == want, key
    if name in PAIRED:
        assert _call(name, Args(tmp_path), tumour=None) == want
        assert _call(name, Args(tmp_path), normal=None) == want
        assert _call(name, Args(tmp_path), num_pair=0) == want
        assert _call(name, Args(tmp_path), num_pair=-1) == want


@pytest.mark.parametrize("name", sorted(ONE_DEVICE))
def test_one_device_functions_refuse_two_devices(tmp_path, name):
    want = (INVALID, ONE_DEVICE[name])
    assert _call(name, Args(tmp_path, devices=[0, 1])) == want
    a = Args(tmp_path)
    a.ca.base.num_device = -1                      # (for these a negative count is the same refusal)
    assert _call(name, a) == want
    # an invalid argument is reported before the device count
    assert _call(name, Args(tmp_path, devices=[0, 1], num_pc=0)) == (INVALID, _invalid(name))
    assert _call(name, Args(tmp_path, devices=[0, 1]), status=False) == (INVALID, _invalid(name))


@pytest.mark.parametrize("name", sorted(FIX_ALPHA))
def test_fix_alpha_is_refused_after_the_device_count(tmp_path, name):
    assert _call(name, Args(tmp_path, fix_alpha=0.01)) == (INVALID, FIX_ALPHA[name])
    assert _call(name, Args(tmp_path, devices=[0, 1], fix_alpha=0.01)) == (INVALID, ONE_DEVICE[name])
    assert _call(name, Args(tmp_path, fix_alpha=0.01), top=-1, num_pair=0) == (INVALID, _invalid(name))


@pytest.mark.parametrize("name", PAIRED)
def test_hom_min_and_the_pairs_come_last_in_that_order(tmp_path, name):
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert _call(name, Args(tmp_path), hom_min=bad) == (INVALID, HOM_MIN), bad
    assert _call(name, Args(tmp_path, fix_alpha=0.01), hom_min=2.0) == (INVALID, FIX_ALPHA[name])
    assert _call(name, Args(tmp_path, devices=[0, 1]), hom_min=2.0) == (INVALID, ONE_DEVICE[name])
    # the pair list is looked at after hom_min, and its messages name vb2_cohort_run_paired from either entry point
    self_pair = "vb2_cohort_run_paired: pair 1: a sample is paired with itself"
    assert _call(name, Args(tmp_path), tumour=(1,), normal=(1,), hom_min=2.0) == (INVALID, HOM_MIN)
    assert _call(name, Args(tmp_path), tumour=(1,), normal=(1,)) == (INVALID, self_pair)
    assert _call(name, Args(tmp_path), tumour=(3,), normal=(1,)) == \
        (INVALID, "vb2_cohort_run_paired: pair 1: a sample index outside the cohort")
    assert _call(name, Args(tmp_path), num_pair=2, tumour=(0, 0), normal=(1, 2)) == \
        (INVALID, "vb2_cohort_run_paired: pair 2: the tumour is listed twice")
    assert _call(name, Args(tmp_path, fix_alpha=0.01), tumour=(1,), normal=(1,)) == (INVALID, FIX_ALPHA[name])


def test_the_plain_run_takes_64_devices_and_no_device_twice(tmp_path):
    invalid = (INVALID, "vb2_cohort_run: invalid argument")
    twice = (INVALID, "vb2_cohort_run: a device is listed twice")
    assert _call("run", Args(tmp_path, devices=list(range(65)))) == invalid
    a = Args(tmp_path)
    a.ca.base.num_device = -1
    assert _call("run", a) == invalid
    assert _call("run", Args(tmp_path, devices=[0, 1, 0])) == twice
    assert _call("run", Args(tmp_path, devices=[3, 3])) == twice
    # 64 devices pass the count and reach the check for a device listed twice; 65 do not get that far
    assert _call("run", Args(tmp_path, devices=list(range(63)) + [0])) == twice
    assert _call("run", Args(tmp_path, devices=list(range(64)) + [0])) == invalid
    # a fixed alpha is the plain run's business: nothing here refuses it (an invalid argument still comes first)
    assert _call("run", Args(tmp_path, devices=[0, 0], fix_alpha=0.01)) == twice
    assert _call("run", Args(tmp_path, devices=[0, 0], fix_alpha=0.01, num_pc=0)) == invalid
