"""--RefVCF's FP64 half at its stage edges, verified a posteriori (tests/panel_ref.py): the projection's column passes
(16 columns of V each), its sample stages (128 samples each), one thread per marker around 256, chunks whose last one is
partly padding, and degenerate spectra (M < N, C = 0, a duplicated sample, N = 1).  Every case is one build through
build_panel_from_genotypes plus check_panel: mu, row_sum and gram exactly, the projection against an 80-bit evaluation
with the builder's own V within (N + 2) u cond and 32 u cond, the eigenpairs by residual, orthonormality, trace and
spectrum against the exact centred Gram, within 32 x what a float64 numpy restatement of the same G leaves."""
import json
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if _abi.lib().vb2_device_count() < 1:
        pytest.fail("no gfx950 device visible: the panel builder runs on the GPU only")


def _checked(G, num_svd_pcs, label, **kw):
    """Build, check, print the record of ratios, fail on the first quantity outside its allowance."""
    r = vb.build_panel_from_genotypes(G, num_svd_pcs=num_svd_pcs, **kw)
    rec = pr.check_panel(G, r, num_svd_pcs)
    print("PANELREC %s %s" % (label, json.dumps(dict(
        M=rec["M"], N=rec["N"], k=rec["k"], ratio={n: rec[n] for n in pr.RATIOS},
        ref_ratio={n: (rec["ref"][n] / rec["allow"][n]) for n in pr.RATIOS if rec["ref"][n] is not None},
        resid_over_s=rec["value"]["resid"] / rec["scale"]["s"], ortho_over_u=rec["value"]["ortho"] / pr.U,
        ref_resid_over_s=rec["ref"]["resid"] / rec["scale"]["s"], ref_ortho_over_u=rec["ref"]["ortho"] / pr.U))))
    pr.assert_inside(rec)
    return r, rec


@pytest.fixture(scope="module")
def wide():
    return pr.structured_geno(300, 80, seed=31)


# ---- column passes of project_kernel (col0 = 0, 16, 32, ...; a partial last pass)

@pytest.mark.parametrize("num_svd_pcs", [1, 15, 16, 17, 32, 33, 0])
def test_column_passes(wide, num_svd_pcs):
    r, rec = _checked(wide, num_svd_pcs, "cols_300x80_k%d" % num_svd_pcs)
    assert rec["k"] == (num_svd_pcs or 80)


def test_column_passes_fewer_markers_than_samples():
    G = pr.structured_geno(50, 80, seed=32)
    r, rec = _checked(G, 0, "cols_50x80_all")
    assert rec["k"] == 50 and r["v"].shape == (80, 50)


# ---- sample stages (kProjRows = 128; the Gram's 64-row tiles; N = 1 and 2)

@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 256, 257])
def test_sample_stages(N):
    G = pr.random_geno(300, N, seed=1000 + N)
    _checked(G, min(17, N), "samples_300x%d" % N)


def test_sample_stages_largest():
    G = pr.structured_geno(1000, 257, seed=33)
    _checked(G, 17, "samples_1000x257")


# ---- marker edges (one thread per marker, 256 per workgroup) and chunks

@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_marker_edges(M):
    G = pr.random_geno(M, 129, seed=2000 + M)
    _checked(G, min(M, 17), "markers_%dx129" % M)


@pytest.mark.parametrize("M", [300, 256, 129])      # the last chunk: 44 markers plus padding, full, one marker
def test_chunks(M):
    G = pr.structured_geno(M, 80, seed=3000 + M)
    one, _ = _checked(G, 17, "chunks_%dx80_one" % M)
    many, _ = _checked(G, 17, "chunks_%dx80_of128" % M, chunk_markers=128)
    # the integer half and mu do not depend on the chunking (c and tau are summed per chunk: v and ud may differ)
    assert np.array_equal(one["gram"], many["gram"]) and np.array_equal(one["row_sum"], many["row_sum"])
    assert np.array_equal(one["mu"].view(np.uint64), many["mu"].view(np.uint64))


# ---- degenerate inputs

@pytest.mark.parametrize("value", [1, -1])
def test_constant_matrix(value):
    G = np.full((300, 80), value, dtype=np.int8)
    r, rec = _checked(G, 17, "constant_%d" % value)
    assert np.array_equal(r["mu"], np.full(300, float(value)))
    assert np.array_equal(r["sigma"], np.zeros(80)), r["sigma"][:4]             # C = 0 exactly
    assert np.isfinite(r["v"]).all() and np.isfinite(r["ud"]).all()
    assert rec["allow"]["resid"] == rec["scale"]["s"] and rec["allow"]["ortho"] == 80 * pr.U     # the floors decide


def test_all_missing_rows(wide):
    G = wide.copy()
    G[:100, :] = -1
    r, rec = _checked(G, 17, "missing_rows")
    assert np.array_equal(r["mu"][:100], np.full(100, -1.0))
    # (g - mu) = 0 in every entry of those rows: ud is 0 up to the rounding of sum_j -V_jq + vsum_q
    _, cond = pr.projection_reference(G[:100], r["mu"][:100], r["v"])
    assert (np.abs(r["ud"][:100]) <= pr.MARGIN * pr.U * cond).all()


def test_duplicated_sample(wide):
    G = wide.copy()
    G[:, 70] = G[:, 5]
    r, rec = _checked(G, 0, "duplicated_sample")
    # C (e_5 - e_70) = 0 exactly: the smallest eigenvalue is rounding noise (the centring's own direction, 1, is not
    # quite null: mu is a binary32 mean)
    assert r["sigma"][79] ** 2 <= rec["allow"]["spec"], r["sigma"][78:]


def test_clamped_eigenvalues():
    G = pr.structured_geno(50, 80, seed=32)
    r, rec = _checked(G, 0, "clamped_50x80")
    tail = r["sigma"][50:]
    assert tail.shape == (30,) and np.isfinite(tail).all() and (tail >= 0).all()
    assert (tail < np.sqrt(rec["allow"]["spec"])).all(), (tail.max(), np.sqrt(rec["allow"]["spec"]))
