"""What the three row sets on a context (Replicates, Conditioned, Paired) share and where they differ, on the MI355X: the
refusals of eval and create with each class's own text, what a refused eval leaves behind (num_step; the stage drained),
and the device memory of a set.  One context of 17 markers x 6, k = 1, two rows per set; every row is the anonymous
model (all-ones weights, all-zero priors), so that each set's values are ctx.llk's.

device_bytes: with the slab cache off a set holds exactly what it asks for; the three literals are what the sets of this
shape reported before the three classes were given one base."""
import ctypes as C

import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi
from verifybamid_amd.api import _p

pytestmark = pytest.mark.gpu

M, K, ROWS = 17, 1, 2
LLK_RTOL = 1e-12                  # the project's evaluation tolerance (tests/test_gpu_parity.py)
DEVICE_BYTES = {"replicates": 1664, "conditioned": 2176, "paired": 2944}
NOUN = {"replicates": "a replicate's", "conditioned": "a hypothesis's", "paired": "a hypothesis's"}
RANGE = {"replicates": "(1..65535 replicates)", "conditioned": "(1..65535 hypotheses)", "paired": "(1..65535 hypotheses)"}
NAMES = sorted(NOUN)


def _payload(name, rows):
    return {"replicates": np.ones((rows, M), dtype=np.uint8), "conditioned": np.zeros((rows, M, 3), dtype=np.float32),
            "paired": np.zeros((rows, M, 6), dtype=np.float32)}[name]


@pytest.fixture(scope="module")
def case():
    d = vb.synth.make_pileup(M, mean_depth=6, num_pc=K, alpha_true=0.05, seed=11)
    before = _abi.get_tunable("slab_cache")
    with vb.LikelihoodContext(d) as ctx:
        _abi.set_tunable("slab_cache", 0)
        try:
            sets = {"replicates": vb.Replicates(ctx, _payload("replicates", ROWS)),
                    "conditioned": vb.Conditioned(ctx, _payload("conditioned", ROWS)),
                    "paired": vb.Paired(ctx, _payload("paired", ROWS))}
            created = {name: s.info()["device_bytes"] for name, s in sets.items()}
        finally:
            _abi.set_tunable("slab_cache", before)
        yield ctx, sets, created
        for s in sets.values():
            s.close()


def _raw_eval(name, s, num_point, pc1, pc2, alpha, out):
    fn = getattr(_abi.lib(), "vb2_%s_eval" % name)
    npt = np.ascontiguousarray(num_point, dtype=np.int32)
    return fn(s._h, _p(npt), _p(pc1), _p(pc2), _p(alpha), _p(out))


def _error():
    return _abi.lib().vb2_last_error().decode()


POINTS = (np.array([[0.01], [-0.02], [0.005]]), np.array([[0.02], [0.0], [-0.01]]), np.array([0.03, 0.2, 0.0]))


@pytest.mark.parametrize("name", NAMES)
def test_a_count_outside_the_slots_is_refused_in_the_classs_words(case, name):
    _, sets, _ = case
    s = sets[name]
    step = s.info()["num_step"]
    pc = np.zeros((9, K))
    assert _raw_eval(name, s, [9, 0], pc, pc, np.zeros(9), np.zeros(9)) == _abi.VB2_ERR_INVALID
    assert _error() == "vb2_%s_eval: %s point count outside 0..VB2_BATCH_SLOTS" % (name, NOUN[name])
    assert s.info()["num_step"] == step


@pytest.mark.parametrize("name", NAMES)
def test_a_step_without_points_is_ok_and_is_no_step(case, name):
    _, sets, _ = case
    s = sets[name]
    step = s.info()["num_step"]
    assert _raw_eval(name, s, [0, 0], None, None, None, None) == _abi.VB2_OK
    assert s.eval([0, 0], np.zeros((0, K)), np.zeros((0, K)), np.zeros(0)).shape == (0,)
    assert s.info()["num_step"] == step


@pytest.mark.parametrize("name", NAMES)
def test_points_without_a_place_for_the_values(case, name):
    """All three refuse; Replicates before anything reaches the stream, Conditioned and Paired after the launch, which
    they drain: one step more, and the next evaluation is right."""
    ctx, sets, _ = case
    s = sets[name]
    pc1, pc2, alpha = POINTS
    want = ctx.llk(pc1, pc2, alpha)
    first = s.eval([2, 1], pc1, pc2, alpha)
    step = s.info()["num_step"]
    assert _raw_eval(name, s, [2, 1], pc1, pc2, alpha, None) == _abi.VB2_ERR_INVALID
    assert _error() == "vb2_%s_eval: invalid argument" % name
    assert s.info()["num_step"] == step + (0 if name == "replicates" else 1)
    again = s.eval([2, 1], pc1, pc2, alpha)
    assert np.array_equal(again, first)
    assert np.all(np.abs(again - want) <= LLK_RTOL * np.abs(want)), (again, want)
    assert s.info()["num_step"] == step + (1 if name == "replicates" else 2)


@pytest.mark.parametrize("name", NAMES)
def test_a_set_of_no_rows_is_refused(case, name):
    ctx, _, _ = case
    h = C.c_void_p()
    create = getattr(_abi.lib(), "vb2_%s_create" % name)
    assert create(ctx._h, 0, _p(_payload(name, 1)), C.byref(h)) == _abi.VB2_ERR_INVALID
    assert _error() == "vb2_%s_create: invalid argument %s" % (name, RANGE[name])
    assert not h.value


def test_the_device_memory_of_a_set(case):
    _, _, created = case
    print("device_bytes with the slab cache off: %r" % created)
    assert created == DEVICE_BYTES
