"""CPU tests of the closed-loop BC driver (gd_bc_rollout, gpudrive_lab_amd.bc_rollout): the surface, the argument checks, the
byte count, and the per-row rule (csrc/bc_rollout_rule.hpp, as a host program) against the numpy restatement of the
reference's script (tests/bc_rollout_reference.py) on scripted sequences, bit for bit."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import bc_rollout_reference as REF
from tests.conftest import ROOT


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert ("int gd_bc_rollout(gd_sim *sim, const gd_bc_policy *policy, const gd_bc_rollout_buffers *buffers, int32_t n_steps);"
            in header)
    assert "gd_bc_rollout" in _capi.SYMBOLS
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "gd_bc_rollout" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    at = L.gd_bc_rollout.argtypes
    assert len(at) == 4 and at[1]._type_ is _capi.GdBCPolicy and at[2]._type_ is _capi.GdBCRolloutBuffers
    B = _capi.GdBCRolloutBuffers
    names = [f[0] for f in B._fields_]
    assert names == ["row_slot", "row_of_slot", "n_rows", "deterministic", "u", "z", "window", "partner_mask", "road_mask",
                     "partner_value", "row_actions", "dead", "goal_achieved", "off_road", "veh_collision", "goal_step",
                     "off_road_step", "init_goal_dist", "goal_dist", "any_alive", "summary", "actions", "dead_mask",
                     "ego_global_pos", "ego_global_rot"]
    # the C struct's layout: two pointers, two int32, 21 pointers -- and the header's fields in the same order
    assert B.n_rows.offset == 16 and B.deterministic.offset == 20 and B.u.offset == 24 and ctypes.sizeof(B) == 24 * 8
    body = header[header.index("typedef struct gd_bc_rollout_buffers {"):header.index("} gd_bc_rollout_buffers;")]
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[ *](\w+)[,;]", code)
    assert declared == names, "the header declares other fields, or in another order"
    from gpudrive_lab_amd import bc_rollout
    assert bc_rollout.SUMMARY_NAMES == REF.SUMMARY_NAMES


def test_exported_from_the_package():
    import gpudrive_lab_amd
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC, ClosedLoopEpisode
    assert gpudrive_lab_amd.ClosedLoopBC is ClosedLoopBC and gpudrive_lab_amd.ClosedLoopEpisode is ClosedLoopEpisode


class _StubSim:
    """Stands in for a SimManager where the checks must fire before the simulator is touched."""

    def __init__(self, model, W=3, A=64):
        self.__dict__.update(_params=types.SimpleNamespace(dynamicsModel=model), _W=W, _A=A)

    def __getattr__(self, name):
        raise AssertionError("the simulator was touched (%s) before the arguments were checked" % name)


def _stub_policy(max_agents=64, num_stack=5):
    """A DeviceBCPolicy that owns nothing on a device: the checks read its sizes only."""
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    p = object.__new__(DeviceBCPolicy)
    p.max_agents, p.num_stack = max_agents, num_stack
    return p


def test_refuses_the_state_model_before_any_device_call():
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    with pytest.raises(ValueError, match="State"):
        ClosedLoopBC(_StubSim(3), _stub_policy())
    with pytest.raises(ValueError, match="State"):
        ClosedLoopBC.nbytes(_StubSim(3), _stub_policy())


@pytest.mark.parametrize("mask", [torch.zeros(3, 63, dtype=torch.bool), torch.zeros(2, 64, dtype=torch.bool),
                                  torch.zeros(3 * 64, dtype=torch.bool), torch.zeros(3, 64), np.zeros((3, 64), bool)])
def test_refuses_a_bad_mask_before_any_device_call(mask):
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    with pytest.raises(ValueError, match="mask"):
        ClosedLoopBC(_StubSim(2), _stub_policy(), mask=mask)
    with pytest.raises(ValueError, match="mask"):
        ClosedLoopBC.nbytes(_StubSim(2), _stub_policy(), mask=mask)


def test_refuses_a_bad_policy_before_any_device_call():
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    good = torch.zeros(3, 64, dtype=torch.bool)
    for policy in (None, object(), torch.nn.Linear(2, 2), {"max_agents": 64}):
        with pytest.raises(ValueError, match="DeviceBCPolicy"):
            ClosedLoopBC(_StubSim(2), policy, mask=good)
    with pytest.raises(ValueError, match="max_agents"):
        ClosedLoopBC(_StubSim(2), _stub_policy(max_agents=128), mask=good)
    with pytest.raises(ValueError, match="max_agents"):
        ClosedLoopBC.nbytes(_StubSim(2, A=128), _stub_policy(max_agents=64))


@pytest.mark.parametrize("n_steps", [0, 92, -1, 5.0, "7", True, None])
def test_run_refuses_bad_steps_before_any_device_call(n_steps):
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    loop = object.__new__(ClosedLoopBC)  # (no simulator, no policy: anything run() touched would raise AttributeError)
    with pytest.raises(ValueError, match="n_steps"):
        loop.run(n_steps=n_steps)


def test_run_refuses_a_draw_without_a_generator_before_any_device_call():
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    loop = object.__new__(ClosedLoopBC)
    with pytest.raises(ValueError, match="generator"):
        loop.run(deterministic=False)
    with pytest.raises(ValueError, match="generator"):
        loop.run(deterministic=False, generator=1234)


def test_nbytes_is_the_sum_of_the_arrays():
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    for A, R in ((64, 5), (128, 5), (64, 1)):
        D = 6 + (A - 1) * 6 + 200 * 13
        row = (R * D * 4            # window
               + R * (A - 1) + R * 200   # the forward's masks
               + (A - 1)            # partner_value
               + 3 * 4              # row_actions
               + 1 + 3 * 4 + 2 * 4 + 2 * 4)  # dead, accumulators, step indices, distances
        assert ClosedLoopBC.row_nbytes(A, R) == row
        assert ClosedLoopBC.row_nbytes(A, R, record=True) == row + 91 * (3 * 4 + 1 + 2 * 4 + 4)

    class Counted(_StubSim):
        def controlled_state_tensor(self):
            t = torch.zeros(3, 64, 1, dtype=torch.int32)
            t[0, :5] = 1
            t[2, 7] = 1
            return types.SimpleNamespace(to_torch=lambda: t)

    sim = Counted(2)
    pol = _stub_policy(64, 5)
    assert ClosedLoopBC.nbytes(sim, pol) == 6 * ClosedLoopBC.row_nbytes(64, 5) + 92 * 4 + 8 * 4
    assert ClosedLoopBC.nbytes(sim, pol, record=True) == 6 * ClosedLoopBC.row_nbytes(64, 5, True) + 92 * 4 + 8 * 4
    mask = torch.zeros(3, 64, dtype=torch.bool)
    mask[1, 3:5] = True
    assert (ClosedLoopBC.nbytes(sim, pol, mask=mask, stochastic=True)
            == 2 * ClosedLoopBC.row_nbytes(64, 5) + 92 * 4 + 8 * 4 + 91 * 2 * 4 * 4)


# ---- the rule against the restatement of simulation.py on scripted sequences
N_ROWS, N_STEPS = 8, 12


def _script(rows=range(N_ROWS), steps=N_STEPS):
    """8 rows x 12 steps; state 0 is the reset state, state t + 1 what is read after step t."""
    S = N_STEPS + 1
    rng = np.random.default_rng(7)
    done = np.zeros((S, N_ROWS), np.int32)
    info = np.zeros((S, N_ROWS, 5), np.int32)
    xy = rng.uniform(-1, 1, (S, N_ROWS, 2)).astype(np.float32)
    info[..., 4] = 7  # the agent type column: never read
    # row 0: done in the reset state (never read: the loop reads done after a step only), then alive until step 5 ends it
    done[0, 0] = 1
    done[6:, 0] = 1
    info[6, 0, 3] = 1
    # row 1: goal and off-road on the same step, and done with it
    info[4, 1, 3] = info[4, 1, 0] = 1
    done[4:, 1] = 1
    # row 2: off road after step 1 and again after step 5: the step index must not move; a done flag that does not stay set
    info[2, 2, 0] = 1
    info[6, 2, 0] = 1
    done[9, 2] = 1
    # row 3: info columns 1 and 2 both set in one step (2, clamped to 1), twice
    info[5, 3, 1] = info[5, 3, 2] = 1
    info[7, 3, 1] = info[7, 3, 2] = 1
    done[8:, 3] = 1
    # row 4: never dies; reaches its goal in the last state (counted by the accumulator, too late for the step index)
    info[N_STEPS, 4, 3] = 1
    # row 5: a zero initial goal distance, goal achieved: the 0 / 0 ratio is replaced by 0
    xy[0, 5] = 0
    xy[3:, 5] = 0
    info[3, 5, 3] = 1
    done[3:, 5] = 1
    # row 6: a zero initial goal distance, no goal: x / 0 = inf, progress -inf
    xy[0, 6] = 0
    done[7:, 6] = 1
    # row 7: flags already in the reset state (the accumulators start from them), dies in step 0; info keeps arriving
    info[0, 7, 0] = 1
    info[0, 7, 1] = info[0, 7, 2] = 1
    done[1:, 7] = 1
    info[10, 7, 3] = 1
    rows = list(rows)
    return done[:steps + 1, rows], info[:steps + 1, rows], xy[:steps + 1, rows]


CASES = {
    "all-rows": _script(),                               # row 4 never dies: all 12 iterations
    "finite": _script(rows=[0, 1, 2, 3, 4, 5, 7]),       # without the -inf row: a finite goal_progress
    "break": _script(rows=[0, 1, 2, 3, 5, 6, 7]),        # without the survivor: the loop breaks after step 8
    "one-step": _script(rows=[4, 7], steps=1),
    "prefix": _script(steps=5),
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_same(got, want, what):
    for k in ("dead", "goal_achieved", "off_road", "veh_collision", "goal_step", "off_road_step", "init_goal_dist", "goal_dist",
              "summary"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, got[k], want[k])
    assert got["iterations"] == want["iterations"], (what, got["iterations"], want["iterations"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_rule_host_program_equals_the_restatement_bit_for_bit(case):
    done, info, xy = CASES[case]
    want = REF.metrics(done, info, xy)
    got = REF.run_rule_host(done, info, xy)
    _assert_same(got, want, case)
    assert got["summary"][7] == want["iterations"] and got["summary"][6] == done.shape[1]


def test_the_script_exercises_what_it_claims():
    done, info, xy = CASES["all-rows"]
    r = REF.metrics(done, info, xy)
    assert r["iterations"] == 12 and r["dead"].tolist() == [True, True, True, True, False, True, True, True]
    assert r["goal_step"].tolist() == [6, 4, -1, -1, -1, 3, -1, 10] and r["off_road_step"].tolist() == [-1, 4, 2, -1, -1, -1, -1, 0]
    assert r["goal_achieved"].tolist() == [1, 1, 0, 0, 1, 1, 0, 1] and r["off_road"].tolist() == [0, 1, 1, 0, 0, 0, 0, 1]
    assert r["veh_collision"].tolist() == [0, 0, 0, 1, 0, 0, 0, 1]
    assert r["init_goal_dist"][5] == 0 and r["init_goal_dist"][6] == 0 and r["goal_dist"][6] > 0
    s = dict(zip(REF.SUMMARY_NAMES, r["summary"].tolist()))
    assert s["goal_progress"] == -np.inf and s["goal_count"] == 5 and s["n_rows"] == 8 and s["iterations"] == 12
    assert s["collision_rate"] == np.float32(np.float32(3 / 8) + np.float32(2 / 8))
    f = REF.metrics(*CASES["finite"])
    assert np.isfinite(f["summary"]).all() and 0 < abs(f["summary"][4]) < 10
    b = REF.metrics(*CASES["break"])
    assert b["iterations"] == 9 and b["dead"].all()  # row 2's done after step 8 ends the loop; later states are never read
    assert b["goal_step"].tolist()[-1] == -1         # row 7's goal in state 10 is behind the break
    assert REF.metrics(*CASES["prefix"])["iterations"] == 5


def test_rule_host_program_under_the_sanitizers():
    """The same scripts through a stand-alone executable built with -fsanitize=address,undefined: it must exit cleanly and
    give the same bits."""
    for case in sorted(CASES):
        done, info, xy = CASES[case]
        _assert_same(REF.run_rule_host(done, info, xy, sanitize=True), REF.metrics(done, info, xy), case + " (sanitized)")


def test_ordered_sum_is_the_lane_order():
    v = np.random.default_rng(3).uniform(-1, 1, 1000).astype(np.float32)
    lanes = [np.float32(0)] * 256
    for i, x in enumerate(v):
        lanes[i % 256] = np.float32(lanes[i % 256] + x)
    total = np.float32(0)
    for s in lanes:
        total = np.float32(total + s)
    assert REF.ordered_sum(v) == total
