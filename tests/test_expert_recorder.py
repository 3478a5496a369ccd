"""CPU tests of the expert trajectory recorder (gd_record_expert, gpudrive_lab_amd.recorder) and of its yardstick, the
reference's save_trajectory restated on the harness (tests/il_reference.py): what can be checked without a device."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd.harness import TorchCallSequence
from tests import il_reference
from tests.conftest import ROOT
from tests.test_harness import FakeSim, _T


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "int gd_record_expert(gd_sim *sim, const gd_record_buffers *buffers, int32_t n_steps);" in header
    assert "gd_record_expert" in _capi.SYMBOLS
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "gd_record_expert" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_record_expert.argtypes) == 3 and L.gd_record_expert.argtypes[1]._type_ is _capi.GdRecordBuffers
    B = _capi.GdRecordBuffers
    assert [f[0] for f in B._fields_] == ["row_slot", "n_rows", "obs", "actions", "dead_mask", "partner_mask", "road_mask",
                                          "ego_global_pos", "ego_global_rot", "dead", "goal_achieved", "off_road",
                                          "veh_collision", "any_alive", "kernel_ms"]
    assert B.obs.offset == 16 and B.kernel_ms.offset == 14 * 8 and ctypes.sizeof(B) == 15 * 8  # the C struct's layout


class _StubSim:
    """Stands in for a SimManager where the checks must fire before the simulator is touched: it knows its shape and its
    parameters and nothing else."""

    def __init__(self, model, W=3, A=64):
        self.__dict__.update(_params=types.SimpleNamespace(dynamicsModel=model), _W=W, _A=A)

    def __getattr__(self, name):
        raise AssertionError("the simulator was touched (%s) before the arguments were checked" % name)


def test_recorder_refuses_the_state_model_before_any_device_call():
    from gpudrive_lab_amd.recorder import ExpertRecorder
    with pytest.raises(ValueError, match="State"):
        ExpertRecorder(_StubSim(3))
    with pytest.raises(ValueError, match="State"):
        ExpertRecorder(_StubSim(3), mask=torch.zeros(3, 64, dtype=torch.bool))


@pytest.mark.parametrize("mask", [torch.zeros(3, 63, dtype=torch.bool), torch.zeros(2, 64, dtype=torch.bool),
                                  torch.zeros(3 * 64, dtype=torch.bool), torch.zeros(3, 64), np.zeros((3, 64), bool)])
def test_recorder_refuses_a_bad_mask_before_any_device_call(mask):
    from gpudrive_lab_amd.recorder import ExpertRecorder
    with pytest.raises(ValueError, match="mask"):
        ExpertRecorder(_StubSim(2), mask=mask)
    with pytest.raises(ValueError, match="mask"):
        ExpertRecorder.nbytes(_StubSim(2), mask)


def test_row_nbytes_is_the_sum_of_the_arrays():
    from gpudrive_lab_amd.recorder import ExpertRecorder, packed_width
    assert packed_width(64) == 2984 and packed_width(128) == 3368
    for A in (64, 128):
        per_step = packed_width(A) * 4 + 3 * 4 + 1 + (A - 1) + 200 + 2 * 4 + 4
        assert ExpertRecorder.row_nbytes(A) == 91 * per_step + 1 + 3 * 4


# ---- the yardstick on a scripted simulator ----
class ScriptedSim(FakeSim):
    """FakeSim whose step k makes the listed slots done and writes the listed info rows; the absolute pose's x counts the
    steps, the self observation's speed is 10 * (step + 1) + slot."""

    def __init__(self, script, W=1, A=64, controlled=(0, 1, 2)):
        super().__init__(W=W, A=A)
        self.t["abs"] = torch.zeros(W, A, 14)
        self.t["controlled"][0, list(controlled), 0] = 1
        self.t["roadmap"][..., 7] = -1.0       # every road row is padding ...
        self.t["roadmap"][0, :, :5, 7] = 3.0   # ... but the first five
        self.t["partner"][..., 8] = -2.0       # nobody ...
        self.t["partner"][0, :, :4, 8] = 1.0   # ... but four partners,
        self.t["partner"][0, :, :4, 0] = 5.0   # which move,
        self.t["resp"][0, 1, 0] = 2            # and slot 1 is Static (partner 0 of ego 0, partner 1 of ego 2)
        self.t["traj"][0, :, 6 * 91:] = torch.arange(64 * 910, dtype=torch.float32).view(64, 910) * 1e-4
        self.script = script
        self._observe()

    absolute_self_observation_tensor = lambda self: _T(self.t["abs"])

    def _observe(self):
        self.t["abs"][0, :, 0] = float(self.steps)
        self.t["abs"][0, :, 1] = torch.arange(64, dtype=torch.float32)
        self.t["abs"][0, :, 7] = 0.25 * self.steps
        self.t["self_obs"][0, :, 0] = 10.0 * (self.steps + 1) + torch.arange(64, dtype=torch.float32)

    def reset(self, worlds):
        super().reset(worlds)
        self.steps = 0
        self.t["done"].zero_()
        self.t["info"].zero_()
        self._observe()

    def step(self):
        done, info = self.script.get(self.steps, ({}, {}))
        self.t["done"].zero_()   # (the simulator keeps done set; the loop must not depend on that)
        self.t["info"].zero_()
        for a in done:
            self.t["done"][0, a, 0] = 1
        for a, row in info.items():
            self.t["info"][0, a] = torch.tensor(row, dtype=torch.int32)
        super().step()
        self._observe()


SCRIPT = {
    1: ({}, {1: [0, 1, 1, 0, 0], 2: [1, 0, 0, 0, 0]}),   # slot 1: both collision columns in one step (2 -> clamped to 1)
    2: ({0}, {0: [0, 0, 0, 1, 0], 2: [1, 0, 0, 0, 0]}),  # slot 0 reaches its goal and is done; slot 2 off road again
    3: ({}, {0: [0, 0, 0, 1, 0]}),                       # a done agent's info still counts while the loop runs
    4: ({1, 2}, {}),                                     # the last two are done: the loop breaks after this step
    5: ({}, {1: [1, 0, 0, 0, 0]}),                       # never reached
}


def test_reference_loop_defaults_dead_mask_clamps_and_break():
    sim = ScriptedSim(SCRIPT)
    h = TorchCallSequence(sim, dynamics_model="delta_local")
    r = il_reference.save_trajectory(h)
    D = 6 + 63 * 6 + 200 * 13
    assert r["iterations"] == 5 and sim.steps == 5  # the early break: steps 0..4 ran, step 5 never did
    assert tuple(r["obs"].shape) == (3, 91, D) and tuple(r["actions"].shape) == (3, 91, 3)
    assert tuple(r["partner_mask"].shape) == (3, 91, 63) and r["partner_mask"].dtype == torch.int64
    assert tuple(r["road_mask"].shape) == (3, 91, 200) and r["road_mask"].dtype == torch.bool
    assert tuple(r["ego_global_pos"].shape) == (3, 91, 2) and tuple(r["ego_global_rot"].shape) == (3, 91, 1)
    # dead_mask[t] is the state BEFORE step t: slot 0 is done by step 2, so t = 2 is still recorded and t = 3 is not
    dm = r["dead_mask"]
    assert dm.dtype == torch.bool
    assert not dm[0, :3].any() and dm[0, 3:].all()
    assert not dm[1, :5].any() and dm[1, 5:].all() and torch.equal(dm[1], dm[2])
    # what a live (row, step) holds: the observation before step t, the action of step t, the pose, the masks
    assert r["obs"][0, 2, 0].item() == pytest.approx((10.0 * 3 + 0) / 100) and r["obs"][2, 4, 0].item() == pytest.approx(0.52)
    assert r["ego_global_pos"][1, 4].tolist() == [4.0, 1.0] and r["ego_global_rot"][1, 4].item() == 1.0
    exp = h.get_expert_actions()[0]
    assert torch.equal(r["actions"][2, :5], exp[0, 2, :5]) and torch.equal(r["actions"][0, :3], exp[0, 0, :3])
    assert r["partner_mask"][0, 0, :5].tolist() == [1, 0, 0, 0, 2]  # ego 0: partner 0 is slot 1, the Static one
    assert r["partner_mask"][2, 0, :5].tolist() == [0, 1, 0, 0, 2]  # ego 2: partner 1 is slot 1
    assert not r["road_mask"][1, 0, :5].any() and r["road_mask"][1, 0, 5:].all()
    # the defaults everywhere else (storage.py:29-35)
    for n, t0 in ((0, 3), (1, 5), (2, 5)):
        assert not r["obs"][n, t0:].any() and not r["actions"][n, t0:].any()
        assert (r["partner_mask"][n, t0:] == 2).all() and r["road_mask"][n, t0:].all()
        assert not r["ego_global_pos"][n, t0:].any() and not r["ego_global_rot"][n, t0:].any()
    # the clamps: slot 0's goal twice, slot 1's two collision columns at once, slot 2 off road twice
    assert r["goal_achieved"].tolist() == [1.0, 0.0, 0.0]
    assert r["veh_collision"].tolist() == [0.0, 1.0, 0.0]
    assert r["off_road"].tolist() == [0.0, 0.0, 1.0]  # (step 5's off_road of slot 1 is behind the break)
    assert r["collision"].tolist() == [False, True, True]


def test_reference_loop_partner_order():
    """Partner j of ego a is slot j for j < a and j + 1 otherwise: with slot 1 Static, it is partner 0 of ego 0 and partner 1
    of ego 2."""
    sim = ScriptedSim(SCRIPT)
    h = TorchCallSequence(sim, dynamics_model="delta_local")
    h.get_obs()
    pm = h.get_partner_mask()
    assert pm[0, 0, :5].tolist() == [1, 0, 0, 0, 2] and pm[0, 2, :5].tolist() == [0, 1, 0, 0, 2]
    assert pm[0, 1, :5].tolist() == [0, 0, 0, 0, 2]


def test_reference_loop_runs_all_91_iterations_without_an_early_break():
    sim = ScriptedSim({90: ({0, 1, 2}, {})})
    h = TorchCallSequence(sim, dynamics_model="classic")
    r = il_reference.save_trajectory(h)
    assert r["iterations"] == 91 and sim.steps == 91
    assert not r["dead_mask"].any() and r["collision"].tolist() == [False, False, False]


def test_reference_loop_with_an_explicit_mask_and_another_observation_source():
    sim = ScriptedSim(SCRIPT)
    h = TorchCallSequence(sim, dynamics_model="delta_local")
    mask = torch.zeros(1, 64, dtype=torch.bool)
    mask[0, 0] = True
    calls = []

    def source():
        calls.append(sim.steps)
        return h.get_obs() + 0.0

    r = il_reference.save_trajectory(h, mask=mask, get_obs=source)
    assert r["iterations"] == 3 and calls == [0, 1, 2, 3]  # one row, done by step 2
    assert tuple(r["obs"].shape) == (1, 91, 6 + 63 * 6 + 200 * 13) and r["goal_achieved"].tolist() == [1.0]
    assert r["partner_mask"][0, 0, :5].tolist() == [1, 0, 0, 0, 2]


# ---- ExpertEpisode.save ----
def test_episode_save_writes_the_reference_files():
    from gpudrive_lab_amd.recorder import ExpertEpisode
    N, T, A = 3, 91, 64
    D = 6 + (A - 1) * 6 + 200 * 13
    g = torch.Generator().manual_seed(0)
    ep = ExpertEpisode(
        obs=torch.rand(N, T, D, generator=g), actions=torch.rand(N, T, 3, generator=g),
        dead_mask=torch.rand(N, T, generator=g) < 0.5,
        partner_mask=torch.randint(0, 3, (N, T, A - 1), generator=g).to(torch.uint8),
        road_mask=torch.rand(N, T, 200, generator=g) < 0.5, ego_global_pos=torch.rand(N, T, 2, generator=g),
        ego_global_rot=torch.rand(N, T, 1, generator=g), goal_achieved=torch.tensor([1.0, 1.0, 0.0]),
        off_road=torch.tensor([0.0, 1.0, 0.0]), veh_collision=torch.tensor([0.0, 0.0, 0.0]), steps=torch.tensor(91))
    assert ep.keep.tolist() == [True, False, True]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        main, glob = ep.save(d, 300)
        assert main == os.path.join(d, "trajectory_300.npz") and glob == os.path.join(d, "global", "global_trajectory_300.npz")
        assert sorted(os.listdir(d)) == ["global", "trajectory_300.npz"]
        assert os.listdir(os.path.join(d, "global")) == ["global_trajectory_300.npz"]
        with np.load(main) as z:  # what baselines/il/il.py:71-82 reads
            assert sorted(z.files) == ["actions", "dead_mask", "obs", "partner_mask", "road_mask"]
            want = dict(obs=((2, T, D), np.float32), actions=((2, T, 3), np.float32), dead_mask=((2, T), np.bool_),
                        partner_mask=((2, T, A - 1), np.int64), road_mask=((2, T, 200), np.bool_))
            for k, (shape, dt) in want.items():
                assert z[k].shape == shape and z[k].dtype == dt, k
            keep = ep.keep
            assert np.array_equal(z["obs"], ep.obs[keep].numpy()) and np.array_equal(z["actions"], ep.actions[keep].numpy())
            assert np.array_equal(z["dead_mask"], ep.dead_mask[keep].numpy())
            assert np.array_equal(z["partner_mask"], ep.partner_mask[keep].numpy().astype(np.int64))
            assert np.array_equal(z["road_mask"], ep.road_mask[keep].numpy())
        with np.load(glob) as z:
            assert sorted(z.files) == ["ego_global_pos", "ego_global_rot"]
            assert z["ego_global_pos"].shape == (2, T, 2) and z["ego_global_pos"].dtype == np.float32
            assert z["ego_global_rot"].shape == (2, T, 1) and z["ego_global_rot"].dtype == np.float32
            assert np.array_equal(z["ego_global_pos"], ep.ego_global_pos[ep.keep].numpy())


# ---- the yardstick on the CPU oracle: the committed scenes meet the conditions the GPU suite relies on ----
class _OracleAsSim:
    """The oracle's numpy views behind the `.to_torch()` surface the harness drives."""

    def __init__(self, orc):
        self._orc = orc

    def __getattr__(self, name):
        f = getattr(self._orc, name)
        if name.endswith("_tensor"):
            return lambda: _T(torch.from_numpy(f()))
        return f


@pytest.mark.parametrize("model,static,iterations,first,last,dropped,goals", [
    ("delta_local", 0, 89, 6, 88, 0, 13),  # every agent reaches its goal; all are dead by t = 88: the break path
    ("delta_local", 1, 89, 0, 88, 2, 41),
    ("classic", 0, 91, 8, 90, 2, 8),       # the loop runs all 91 iterations; both values of keep occur
    ("classic", 1, 91, 0, 90, 3, 37),
])
def test_reference_loop_on_the_oracle_meets_the_conditions(oracle_mod, model, static, iterations, first, last, dropped, goals):
    from tests.conftest import SCENE_4, SCENE_407, TEST_JSON
    O = oracle_mod
    kw = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0,
              dynamicsModel={"classic": 0, "delta_local": 2}[model], isStaticAgentControlled=static,
              initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1, roadObservationAlgorithm=1, collisionBehaviour=1)
    orc = O.OracleSim([TEST_JSON, SCENE_407, SCENE_4], O.default_params(**kw), max_agents=64)
    try:
        h = TorchCallSequence(_OracleAsSim(orc), dynamics_model=model)
        assert h.cont_agent_mask.sum(1).tolist() == ([16, 8, 19] if static else [2, 3, 8])
        r = il_reference.save_trajectory(h)
        dm = r["dead_mask"]
        death = [int(x.to(torch.int32).argmax()) - 1 if x.any() else 90 for x in dm]  # the step that ended each row
        assert r["iterations"] == iterations and (min(death), max(death)) == (first, last)
        assert int(r["collision"].sum()) == dropped and int(r["goal_achieved"].sum()) == goals
        assert bool(dm[:, :90].any()) and bool((~dm[:, 50:]).any())
        if not static:
            assert bool((r["partner_mask"][~dm] == 1).any())
    finally:
        orc.close()
