"""What differs between the three row-set refit drivers (replicates, conditioned, paired), without a device: the message
of an empty row, whether a fixed alpha is refused and under whose name, and which side of a point is held.  A closed-form
evaluator stands in for the likelihood (k = 1, 3 rows), so that every difference is the driver's own.

tests/test_conditioned_cpu.py::test_the_driver_fixes_pc1_at_every_call_and_an_empty_hypothesis_fails_alone and its twin
in tests/test_paired_cpu.py already assert the held side and the lone status of the conditioned and the paired driver on
the restatements; here they are checked only through the one evaluator all three share, beside what those leave out:
the replicates' side of each, and the texts."""
import numpy as np
import pytest

import verifybamid_amd as vb
from verifybamid_amd import _abi

K, ROWS = 1, 3
FIXED = np.array([[0.011], [0.02], [-0.01]])
DRIVERS = {
    "replicates": (lambda ev, **kw: vb.replicates_with_evaluator(ev, ROWS, K, **kw),
                   "vb2_replicates_optimize_llk: a replicate's weights select no counted marker"),
    "conditioned": (lambda ev, **kw: vb.conditioned_with_evaluator(ev, ROWS, K, FIXED, **kw),
                    "vb2_conditioned_optimize_llk: the sample counts no marker under a hypothesis"),
    "paired": (lambda ev, **kw: vb.paired_with_evaluator(ev, ROWS, K, FIXED, **kw),
               "vb2_paired_optimize_llk: a hypothesis leaves the sample no marker"),
}


class Quadratic:
    """llk of row r at a point: a concave quadratic with its maximum at alpha = 0.05 + 0.03 r, pc1 = 0.01, pc2 = -0.02,
    always negative; a row in `empty` gives exactly 0.0.  Keeps what it was called with."""

    def __init__(self, empty=()):
        self.empty, self.calls = set(empty), []

    def __call__(self, num_point, pc1, pc2, alpha):
        self.calls.append((num_point.copy(), pc1.copy(), pc2.copy(), alpha.copy()))
        rows = np.repeat(np.arange(len(num_point)), num_point)
        out = -10.0 - 1000.0 * (alpha - (0.05 + 0.03 * rows)) ** 2 - 50.0 * (pc1[:, 0] - 0.01) ** 2 - 50.0 * (pc2[:, 0] + 0.02) ** 2
        out[np.isin(rows, list(self.empty))] = 0.0
        return out


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_an_empty_row_fails_alone_with_the_drivers_own_message(name):
    run, message = DRIVERS[name]
    ev = Quadratic(empty=[1])
    est = run(ev)
    assert [e["status"] for e in est] == [0, _abi.VB2_ERR_INVALID, 0]
    assert _abi.lib().vb2_last_error().decode() == message
    assert ev.calls[0][0].tolist() == [1, 1, 1]
    assert all(c[0][1] == 0 for c in ev.calls[1:])                            # the empty row leaves after its first value
    for r in (0, 2):                                                          # the others finish, at their own maximum
        assert abs(est[r]["alpha"] - (0.05 + 0.03 * r)) < 1e-3, est[r]


def test_a_fixed_alpha_is_refused_by_the_refits_under_their_own_name_and_not_by_the_replicates():
    for name in ("conditioned", "paired"):
        with pytest.raises(_abi.Vb2Error) as exc:
            DRIVERS[name][0](Quadratic(), fix_alpha=0.02)
        assert ("vb2_%s_optimize_llk: a fixed alpha leaves the refit nothing to estimate (--FixAlpha)" % name) in str(exc.value)
    ev = Quadratic()
    est = DRIVERS["replicates"][0](ev, fix_alpha=0.02)
    assert [e["status"] for e in est] == [0, 0, 0]
    assert all(e["alpha"] == 0.02 for e in est)
    assert all(np.all(c[3] == 0.02) or np.all(c[3] == 0.0) for c in ev.calls)  # (llk0 is taken at alpha = 0)


def test_the_held_side():
    def sides(name):
        ev = Quadratic()
        est = DRIVERS[name][0](ev)
        assert [e["status"] for e in est] == [0, 0, 0]
        assert np.all(ev.calls[-1][3] == 0.0)                                 # the llk0 call is among them
        rows = [np.repeat(np.arange(ROWS), c[0]) for c in ev.calls]
        return ev.calls, rows

    calls, rows = sides("conditioned")
    assert all(np.array_equal(c[1], FIXED[r]) for c, r in zip(calls, rows))
    assert any(not np.array_equal(c[2], FIXED[r]) for c, r in zip(calls, rows))
    calls, rows = sides("paired")
    assert all(np.array_equal(c[2], FIXED[r]) for c, r in zip(calls, rows))
    assert any(not np.array_equal(c[1], FIXED[r]) for c, r in zip(calls, rows))
    # the replicates hold neither side and keep the model's two sets of PCs: both move, and apart from each other
    calls, rows = sides("replicates")
    for side in (1, 2):
        assert len({float(v) for c in calls for v in c[side][:, 0]}) > 3
    assert any(not np.array_equal(c[1], c[2]) for c in calls)
