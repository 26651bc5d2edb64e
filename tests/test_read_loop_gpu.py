"""The branches of the probability-domain row walk (eval_body: walk_pd and the loops around it), which go wrong by KIND of row and
not by size: a tile without rows, a first row that is ref-ref, ref-alt or alt-alt, an odd or even count of ref rows, the mixed
row, odd and even alt tails.  Small, shallow samples reach them all -- at a mean depth of 0.5 most markers have no read and
many have alt reads only.  The order in which a row's table reads and multiplies are issued (READS_AHEAD) may not move a
bit: each launch is compared with the pass-per-group kernel, with the plain 8-point launches, with the oracle, and with
the bytes the commit before that change computed (tests/golden/read_loop, tools/make_read_loop_golden.py)."""
import json
import os
import sys

import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_read_loop_golden as gold  # noqa: E402

pytestmark = pytest.mark.gpu

LLK_RTOL = 1e-12
GOLDEN = os.path.join(ROOT, "tests", "golden", "read_loop")


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def marker_classes(d):
    """(markers without a read, markers all of whose reads are the upper-case alt base)"""
    depth = np.diff(d.read_off)
    none = int((depth == 0).sum())
    mk = np.repeat(np.arange(d.num_marker), depth)
    not_alt = np.bincount(mk, weights=(d.bases != d.alt_base[mk]), minlength=d.num_marker)
    return none, int(((depth > 0) & (not_alt == 0)).sum())


@pytest.fixture(scope="module")
def golden():
    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    llk = np.load(os.path.join(GOLDEN, "llk.npy"))
    assert [tuple(c) for c in meta["cases"]] == [tuple(c) for c in gold.CASES] and tuple(meta["sizes"]) == gold.SIZES
    assert llk.shape == (len(gold.CASES), sum(gold.SIZES)) and len(meta["parent_commit"]) == 40
    return meta, llk


@pytest.mark.parametrize("case", gold.CASES, ids=lambda c: "depth%s-k%d-q%d..%d%s" % (c[0], c[1], c[2], c[3], "-knownAF" if c[4] else ""))
def test_every_kind_of_row_gives_the_bits_of_the_other_kernels_and_of_the_parent_commit(case, tunable, golden):
    from conftest import fixture_input_must_match
    meta, want_all = golden
    ci = gold.CASES.index(case)
    depth, k = case[0], case[1]
    d = gold.make_case(case)
    pc1, pc2, al = gold.points(case)
    fixture_input_must_match(gold.input_sha(d, (pc1, pc2, al)), meta["input_sha256"][ci], "read_loop case %r" % (case,))
    none, alt_only = marker_classes(d)
    print("depth %s: %d markers without a read, %d with upper-case alt reads only" % (depth, none, alt_only))
    if depth in (0.5, 3):
        assert none > 0 and alt_only > 0
    od = oracle_data(d)
    ref = np.array([od.llk(pc1[i], pc2[i], al[i], num_thread=1) for i in range(max(gold.SIZES))])      # (1 500 markers: a thread pool costs more than the sum)
    off = 0
    with vb.LikelihoodContext(d) as ctx:
        assert ctx.info()["layout"] == 1
        for B in gold.SIZES:
            p1, p2, a = pc1[:B], pc2[:B], al[:B]
            tunable("split", 1)
            got = ctx.llk(p1, p2, a)
            assert np.all(np.isfinite(got)) and np.all(got < 0), B
            tunable("split", 0)
            assert np.array_equal(ctx.llk(p1, p2, a), got), B                                   # (a)
            tunable("split", 1)
            plain = np.concatenate([ctx.llk(p1[i:i + 8], p2[i:i + 8], a[i:i + 8]) for i in range(0, B, 8)])
            assert np.array_equal(plain, got), B                                                # (b)
            err = rel_err(got, ref[:B])             # (the smaller launch takes the first points of the larger one)
            print("B = %d: max rel err against the oracle %.2e" % (B, err))
            assert err <= LLK_RTOL, B                                                           # (c)
            want = want_all[ci, off:off + B]
            assert got.tobytes() == want.tobytes(), (B, int(np.sum(got != want)))               # (d)
            off += B
