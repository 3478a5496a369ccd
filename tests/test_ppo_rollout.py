"""CPU tests of the closed-loop PPO evaluator (gd_policy_rollout, gpudrive_lab_amd.ppo_rollout): the surface, the argument
checks, the byte count, and the rule (csrc/policy_rollout_rule.hpp, as a host program) against the numpy restatement of the
reference's rollout (tests/ppo_rollout_reference.py) on scripted sequences, bit for bit."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import ppo_rollout_reference as REF
from tests.conftest import ROOT


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert ("int gd_policy_rollout(gd_sim *sim, const gd_policy *policy, const gd_policy_rollout_buffers *buffers, "
            "int32_t n_steps);" in header)
    assert "gd_policy_rollout" in _capi.SYMBOLS
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "gd_policy_rollout" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    at = L.gd_policy_rollout.argtypes
    assert len(at) == 4 and at[1]._type_ is _capi.GdPolicy and at[2]._type_ is _capi.GdPolicyRolloutBuffers
    B = _capi.GdPolicyRolloutBuffers
    names = [f[0] for f in B._fields_]
    assert names == ["n_rows", "deterministic", "u", "table", "n_actions", "reserved", "actions", "logprob", "entropy", "value",
                     "live", "goal_achieved", "collided", "off_road", "world_active", "episode_lengths", "bad_indices",
                     "any_active", "goal_achieved_count", "frac_goal_achieved", "collided_count", "frac_collided",
                     "off_road_count", "frac_off_road", "other_count", "frac_other", "controlled_per_scene", "summary",
                     "actions_idx", "live_mask", "agent_positions"]
    # the C struct's layout: two int32, two pointers, two int32, 25 pointers -- and the header's fields in the same order
    assert B.n_rows.offset == 0 and B.deterministic.offset == 4 and B.u.offset == 8 and B.table.offset == 16
    assert B.n_actions.offset == 24 and B.reserved.offset == 28 and B.actions.offset == 32
    assert B.summary.offset == 32 + 21 * 8 and B.agent_positions.offset == 32 + 24 * 8 and ctypes.sizeof(B) == 32 + 25 * 8
    body = header[header.index("typedef struct gd_policy_rollout_buffers {"):header.index("} gd_policy_rollout_buffers;")]
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[ *](\w+)[,;]", code)
    assert declared == names, "the header declares other fields, or in another order"
    from gpudrive_lab_amd import ppo_rollout
    assert ppo_rollout.SUMMARY_NAMES == REF.SUMMARY_NAMES
    assert ppo_rollout.WORLD_RESULTS == REF.WORLD_NAMES


def test_the_rule_header_states_the_summary_order():
    hdr = open(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "policy_rollout_rule.hpp")).read()
    enum = re.search(r"enum \{ (S_GOAL_ACHIEVED.*?) \};", hdr).group(1)
    assert [n.strip()[2:].lower() for n in enum.split(",")] == list(REF.SUMMARY_NAMES)


def test_exported_from_the_package():
    import gpudrive_lab_amd
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO, PolicyEpisode
    assert gpudrive_lab_amd.ClosedLoopPPO is ClosedLoopPPO and gpudrive_lab_amd.PolicyEpisode is PolicyEpisode


class _StubSim:
    """Stands in for a SimManager where the checks must fire before the simulator is touched."""

    def __init__(self, model, W=3, A=64):
        self.__dict__.update(_params=types.SimpleNamespace(dynamicsModel=model), _W=W, _A=A)

    def __getattr__(self, name):
        raise AssertionError("the simulator was touched (%s) before the arguments were checked" % name)


def _stub_policy(max_agents=64, ego_width=6, n_actions=91):
    """A DevicePolicy that owns nothing on a device: the checks read its sizes only."""
    from gpudrive_lab_amd.policy import DevicePolicy
    p = object.__new__(DevicePolicy)
    p.max_agents, p.ego_width, p.n_actions = max_agents, ego_width, n_actions
    return p


GOOD = dict(mask=torch.zeros(3, 64, dtype=torch.bool))


def test_refuses_the_state_model_before_any_device_call():
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    with pytest.raises(ValueError, match="State"):
        ClosedLoopPPO(_StubSim(3), _stub_policy())
    with pytest.raises(ValueError, match="State"):
        ClosedLoopPPO.nbytes(_StubSim(3), _stub_policy())


@pytest.mark.parametrize("mask", [torch.zeros(3, 63, dtype=torch.bool), torch.zeros(2, 64, dtype=torch.bool),
                                  torch.zeros(3 * 64, dtype=torch.bool), torch.zeros(3, 64), np.zeros((3, 64), bool)])
def test_refuses_a_bad_mask_before_any_device_call(mask):
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    with pytest.raises(ValueError, match="mask"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(), mask=mask)
    with pytest.raises(ValueError, match="mask"):
        ClosedLoopPPO.nbytes(_StubSim(0), _stub_policy(), mask=mask)


def test_refuses_a_bad_policy_before_any_device_call():
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    for policy in (None, object(), torch.nn.Linear(2, 2), {"max_agents": 64}, object.__new__(DeviceBCPolicy)):
        with pytest.raises(ValueError, match="DevicePolicy"):
            ClosedLoopPPO(_StubSim(0), policy, **GOOD)
    with pytest.raises(ValueError, match="max_agents"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(max_agents=128), **GOOD)
    with pytest.raises(ValueError, match="max_agents"):
        ClosedLoopPPO.nbytes(_StubSim(0, A=128), _stub_policy(max_agents=64))


def test_refuses_reward_weights_that_do_not_fit_the_policy():
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    good = torch.zeros(3, 64, 3)
    with pytest.raises(ValueError, match="reward_weights"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(ego_width=9), **GOOD)  # required
    for wt in (torch.zeros(3, 64, 2), torch.zeros(3, 64, 3, dtype=torch.float64), np.zeros((3, 64, 3), np.float32), 1.0):
        with pytest.raises(ValueError, match="reward_weights"):
            ClosedLoopPPO(_StubSim(0), _stub_policy(ego_width=9), reward_weights=wt, **GOOD)
    with pytest.raises(ValueError, match="reward_weights"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(ego_width=6), reward_weights=good, **GOOD)  # refused


def test_refuses_a_table_that_does_not_fit_the_policy():
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    for table in (torch.zeros(91, 2), torch.zeros(91), np.zeros((91, 3), np.float32), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="action_table"):
            ClosedLoopPPO(_StubSim(0), _stub_policy(), action_table=table, **GOOD)
    with pytest.raises(ValueError, match="n_actions"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(), action_table=torch.zeros(7, 3), **GOOD)
    with pytest.raises(ValueError, match="n_actions"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(n_actions=7), **GOOD)  # the default table of classic has 91 rows
    with pytest.raises(ValueError, match="delta_local"):
        ClosedLoopPPO(_StubSim(2), _stub_policy(), **GOOD)  # the default table of delta_local has 8000


@pytest.mark.parametrize("init_steps", [-1, 91, 5.0, "7", True, None])
def test_refuses_bad_init_steps_before_any_device_call(init_steps):
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    with pytest.raises(ValueError, match="init_steps"):
        ClosedLoopPPO(_StubSim(0), _stub_policy(), init_steps=init_steps, **GOOD)


@pytest.mark.parametrize("n_steps", [0, 92, -1, 5.0, "7", True, None])
def test_run_refuses_bad_steps_before_any_device_call(n_steps):
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    loop = object.__new__(ClosedLoopPPO)  # (no simulator, no policy: anything run() touched would raise AttributeError)
    with pytest.raises(ValueError, match="n_steps"):
        loop.run(n_steps=n_steps, deterministic=True)


def test_run_refuses_a_draw_without_a_generator_before_any_device_call():
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    loop = object.__new__(ClosedLoopPPO)
    with pytest.raises(ValueError, match="generator"):
        loop.run()
    with pytest.raises(ValueError, match="generator"):
        loop.run(deterministic=False, generator=1234)


def test_nbytes_is_the_sum_of_the_arrays():
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    row = 8 + 3 * 4 + 1 + 3 * 4            # actions, logprob / entropy / value, live, the three sums
    world = 1 + 4 + 4 + 9 * 4              # world_active, episode_lengths, bad_indices, the nine results
    assert ClosedLoopPPO.row_nbytes() == row and ClosedLoopPPO.row_nbytes(record=True) == row + 91 * (8 + 1)
    for A in (64, 128):
        assert ClosedLoopPPO.world_nbytes(A) == world and ClosedLoopPPO.world_nbytes(A, record=True) == world + A * 91 * 2 * 4

    class Counted(_StubSim):
        def controlled_state_tensor(self):
            t = torch.zeros(3, 64, 1, dtype=torch.int32)
            t[0, :5] = 1
            t[2, 7] = 1
            return types.SimpleNamespace(to_torch=lambda: t)

    sim = Counted(0)
    pol = _stub_policy()
    fixed = 92 * 4 + 8 * 4
    assert ClosedLoopPPO.nbytes(sim, pol) == 6 * row + 3 * world + fixed
    assert ClosedLoopPPO.nbytes(sim, pol, record=True) == 6 * (row + 91 * 9) + 3 * (world + 64 * 91 * 8) + fixed
    mask = torch.zeros(3, 64, dtype=torch.bool)
    mask[1, 3:5] = True
    assert ClosedLoopPPO.nbytes(sim, pol, mask=mask, stochastic=True) == 2 * row + 3 * world + fixed + 91 * 2 * 4


# ---- the rule against the restatement of eval_utils.rollout() on scripted sequences
W_S, A_S = 6, 8


def _script(steps=91):
    """6 worlds x 8 slots; entry t is what is read after step t."""
    mask = np.zeros((W_S, A_S), bool)
    done = np.zeros((91, W_S, A_S), np.int32)
    info = np.zeros((91, W_S, A_S, 5), np.int32)
    info[..., 4] = 7  # the agent type column: never read
    # world 0: no rows (NaN fractions, length 0); its slots carry flags and done flags all the same
    done[3:, 0, 2] = 1
    info[3, 0, 2, 3] = 1
    # world 1: one row, which finishes in step 0 with its goal
    mask[1, 4] = True
    done[0:, 1, 4] = 1
    info[0, 1, 4, 3] = 1
    # world 2: three rows, nothing before the end of the episode: finishes at t = 90; row 1 collects nothing at all (other),
    # row 0 goes off road twice (a raw sum of 2) and collides with both kinds in one step (2), row 5 reaches the goal at the end
    mask[2, [0, 1, 5]] = True
    done[90, 2, :] = 1
    info[10, 2, 0, 0] = info[11, 2, 0, 0] = 1
    info[40, 2, 0, 1] = info[40, 2, 0, 2] = 1
    info[90, 2, 5, 3] = 1
    # world 3: a done flag on a slot outside the mask must not count: the world finishes when rows 1 and 2 are both done (t = 7)
    mask[3, [1, 2]] = True
    done[2:, 3, 6] = 1
    done[4:, 3, 1] = 1
    info[4, 3, 1, 0] = 1
    info[6, 3, 1, 3] = 1   # after the row died: not counted
    done[7:, 3, 2] = 1
    info[7, 3, 2, 1] = 1
    # world 4: a done flag that does not stay set: row 0 is done after step 5 only, row 3 from step 9 on; never both at once
    # before step 20, where both are
    mask[4, [0, 3]] = True
    done[5, 4, 0] = 1
    done[9:, 4, 3] = 1
    done[20:, 4, 0] = 1
    info[12, 4, 0, 0] = 1   # row 0 died at step 5: not counted
    info[9, 4, 3, 3] = info[9, 4, 3, 0] = 1  # two flags on one row
    # world 5: every slot is a row; all finish at t = 30 but one, which the world waits for until t = 60
    mask[5, :] = True
    done[30:, 5, :7] = 1
    done[60:, 5, 7] = 1
    info[30, 5, :4, 3] = 1
    info[45, 5, 7, 2] = 1
    return mask, done[:steps], info[:steps]


def _worlds(script, worlds):
    mask, done, info = script
    return mask[worlds], done[:, worlds], info[:, worlds]


CASES = {
    "all-worlds": _script(),                              # world 2 runs to the end: all 91 iterations
    "break": _worlds(_script(), [0, 1, 3, 4, 5]),         # without it: the loop breaks after step 60
    "one-step": _worlds(_script(steps=1), [0, 1, 2]),
    "prefix": _script(steps=7),
    "no-rows-only": _worlds(_script(), [0]),              # every world is done at t = 0
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_same(got, want, what):
    for k in ("live", "goal_achieved", "collided", "off_road", "world_active", "episode_lengths", "any_active", "summary") + REF.WORLD_NAMES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:  # NaN as NaN (IEEE leaves the sign and payload of 0 / 0 open), everything else by its bits
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan) and np.array_equal(_bits(g)[~nan], _bits(w)[~nan]), (what, k, g, w)
        else:
            assert np.array_equal(g, w), (what, k, g, w)
    assert got["iterations"] == want["iterations"], (what, got["iterations"], want["iterations"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_rule_host_program_equals_the_restatement_bit_for_bit(case):
    mask, done, info = CASES[case]
    want = REF.metrics(mask, done, info)
    got = REF.run_rule_host(mask, done, info)
    _assert_same(got, want, case)
    assert got["summary"][6] == want["iterations"] and got["summary"][4] == mask.sum()


def test_the_script_exercises_what_it_claims():
    r = REF.metrics(*CASES["all-worlds"])
    assert r["iterations"] == 91 and r["episode_lengths"].tolist() == [0, 0, 90, 7, 20, 60]
    assert np.isnan(r["frac_goal_achieved"][0]) and np.isnan(r["frac_other"][0]) and r["controlled_per_scene"][0] == 0
    assert r["goal_achieved_count"].tolist() == [0, 1, 1, 0, 1, 4] and r["collided_count"].tolist() == [0, 0, 1, 1, 0, 1]
    assert r["off_road_count"].tolist() == [0, 0, 1, 1, 1, 0] and r["other_count"].tolist() == [0, 0, 1, 0, 1, 3]
    assert r["off_road"][2, 0] == 2 and r["collided"][2, 0] == 2, "the sums are raw, not clamped"
    assert r["goal_achieved"][3, 1] == 0 and r["off_road"][4, 0] == 0, "a dead row collected a flag"
    assert r["goal_achieved"][0].sum() == 0 and not r["live"].any()
    assert r["goal_achieved"][4, 3] == 1 and r["off_road"][4, 3] == 1, "a row collects two flags"
    assert r["frac_other"].tolist()[1:] == [0, np.float32(1 / 3), 0, 0.5, np.float32(3 / 8)]
    s = dict(zip(REF.SUMMARY_NAMES, r["summary"].tolist()))
    assert s == dict(goal_achieved=7, collided=3, off_road=3, other=5, n_rows=16, worlds_with_rows=5, iterations=91,
                     mean_episode_length=float(np.float32(177) / np.float32(6)))
    b = REF.metrics(*CASES["break"])
    assert b["iterations"] == 61 and b["any_active"][:62].tolist() == [1] * 61 + [0] and not b["world_active"].any()
    p = REF.metrics(*CASES["prefix"])
    assert p["iterations"] == 7 and p["episode_lengths"].tolist() == [0, 0, 0, 0, 0, 0] and p["world_active"].tolist() == [
        False, False, True, True, True, True] and p["any_active"][7] == 1
    n = REF.metrics(*CASES["no-rows-only"])
    assert n["iterations"] == 1 and np.isnan(n["frac_collided"]).all() and n["summary"][5] == 0


def test_rule_host_program_under_the_sanitizers():
    """The same scripts through a stand-alone executable built with -fsanitize=address,undefined: it must exit cleanly and
    give the same bits."""
    for case in sorted(CASES):
        mask, done, info = CASES[case]
        _assert_same(REF.run_rule_host(mask, done, info, sanitize=True), REF.metrics(mask, done, info), case + " (sanitized)")
