"""GPU suite: learner rows -- the packed observation written per controlled agent, discrete actions decoded on the device and
the flat episode outputs (gd_set_learner_rows, gd_attach_packed_rows, gd_set_discrete_actions, gd_episode_buffers.*_rows,
gpudrive_lab_amd.learner.DeviceLearnerEnv).

Everything here is held to the path the engine already had, bit for bit: twin simulators on the same scenes and the same
actions, one with the full [W, A, D] direct pack and torch's boolean indexing, the other with the learner rows."""
import numpy as np
import pytest
import torch

from tests import parity as P
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

# classic dynamics, parked cars Static (what the reference's PPO baselines construct)
BASE = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0, dynamicsModel=0,
            isStaticAgentControlled=0, initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1)

ROADS = {  # (knn_order, roadObservationAlgorithm, environment), as in tests/test_gpu_step_outputs.py
    "ref_order": (0, 0, {"GPUDRIVE_RANK_MIN_ROADS": "200"}),
    "set_order_fused": (1, 0, {"GPUDRIVE_SET_FUSED_ROWS": "1"}),
    "set_order_row_kernel": (1, 0, {"GPUDRIVE_SET_FUSED_ROWS": "0"}),
    "linear": (0, 1, {}),
}
STEPS = 36
WARM = 86          # log playback before the first compared step: the 91-step episode ends inside the compared steps
CANARY = 1 << 18   # floats of the guard region behind the row buffer (1 MB)
CANARY_BITS = 0x7FC0DEAD  # a NaN payload no kernel writes


def _bits(t):
    return t.contiguous().view(torch.int32)


def _equal_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    if not torch.equal(_bits(a), _bits(b)):
        bad = (_bits(a) != _bits(b)).nonzero()
        raise AssertionError("%s: %d elements differ, first at %s" % (what, bad.shape[0], bad[0].tolist()))


def _actions(gen, W, A, dev):
    a = torch.zeros(W, A, 10)
    a[..., 0] = torch.rand(W, A, generator=gen) * 5.0 - 3.0
    a[..., 1] = torch.rand(W, A, generator=gen) * 1.4 - 0.7
    return a.to(dev)


def _mask(kind, sim, seed=7):
    W, A = sim._W, sim._A
    dev = sim._device
    if kind == "controlled":
        return sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
    if kind == "random":  # padding and Static slots included
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(W, A, generator=g) < 0.4).to(dev)
    if kind == "all":
        return torch.ones(W, A, dtype=torch.bool, device=dev)
    return torch.zeros(W, A, dtype=torch.bool, device=dev)


class _Guarded:
    """A NaN-filled row buffer with a canary tail."""

    def __init__(self, n, D, dev):
        self.n, self.D = n, D
        self.buf = torch.full((n * D + CANARY,), float("nan"), dtype=torch.float32, device=dev)
        self.buf.view(torch.int32)[n * D:] = CANARY_BITS

    def check(self, what):
        rows = self.buf[:self.n * self.D]
        assert not bool(torch.isnan(rows).any()), "%s: a learner row was not written" % what
        assert bool((self.buf.view(torch.int32)[self.n * self.D:] == CANARY_BITS).all()), "%s: write past the row buffer" % what


def _attach_rows(sim, mask_kind, only):
    mask = _mask(mask_kind, sim)
    n = sim.set_learner_rows(mask)
    assert n == int(mask.sum())
    D = 6 + (sim._A - 1) * 6 + 200 * 13
    g = _Guarded(n, D, sim._device)
    rows = sim.direct_pack_rows(only=only, out=g.buf)
    assert tuple(rows.shape) == (n, D)
    return mask, g, rows


def _run_twins(monkeypatch, tmp_path, roads, cb, slots, only, mask_kind):
    knn_order, algo, env = ROADS[roads]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scenes = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    kw = dict(BASE, roadObservationAlgorithm=algo, collisionBehaviour=cb)
    from gpudrive_lab_amd.episode import EpisodeTracker
    full = P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, **kw)
    rsim = P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, **kw)
    try:
        assert full.direct_pack(only=only)
        mask, guard, rows = _attach_rows(rsim, mask_kind, only)
        torch.cuda.synchronize()
        guard.check("attach")
        _equal_bits(rows, full.packed_observations()[mask], "attach")
        for s in (full, rsim):
            s.advance_log_playback(WARM)
        tf, tr = EpisodeTracker(full), EpisodeTracker(rsim)
        gen = torch.Generator().manual_seed(11)
        W = len(scenes)
        resets = 0
        for k in range(STEPS):
            a = _actions(gen, W, slots, full._device)
            full.action_tensor().to_torch().copy_(a)
            rsim.action_tensor().to_torch().copy_(a)
            tf.step()
            tr.step()
            resets += int(tf.done_worlds.sum())
            if k == 12:
                for s in (full, rsim):
                    s.reset([0, W - 1])
            if k == 18:
                for s in (full, rsim):
                    s.deleteAgents({1: [0]})
            if k == 26:  # new scenes: the rows are set (and attached) again, as the caller must
                for s in (full, rsim):
                    s.set_maps(scenes[1:] + scenes[:1])
                mask, guard, rows = _attach_rows(rsim, mask_kind, only)
                tf, tr = EpisodeTracker(full), EpisodeTracker(rsim)
            torch.cuda.synchronize()
            guard.check("step %d" % k)
            _equal_bits(rows, full.packed_observations()[mask], "step %d" % k)
            if not only:  # the raw rows are still written for every slot
                for name in ("partner_observations_tensor", "agent_roadmap_tensor", "self_observation_tensor"):
                    _equal_bits(getattr(rsim, name)().to_torch(), getattr(full, name)().to_torch(), "%s step %d" % (name, k))
        assert resets > 0, "no world was reset by the tracker"
        if only:
            with pytest.raises(NotImplementedError):
                rsim.packed_observations()
        print("LEARNER_ROWS %s cb%d A=%d only=%d mask=%s rows=%d resets=%d" % (roads, cb, slots, only, mask_kind, guard.n, resets))
    finally:
        full.close()
        rsim.close()


MATRIX = ([("linear", cb, A, only, "controlled") for cb in (0, 1, 2) for A in (64, 128) for only in (0, 1)] +
          [(r, 1, 64, only, "controlled") for r in ("set_order_fused", "set_order_row_kernel") for only in (0, 1)] +
          [("ref_order", 1, A, only, "controlled") for A in (64, 128) for only in (0, 1)] +
          [("linear", 1, 64, 1, m) for m in ("random", "all", "none")] +
          [("ref_order", 1, 128, 0, m) for m in ("random", "all", "none")] +
          [("set_order_fused", 2, 64, 1, "random")])


@pytest.mark.parametrize("roads,cb,slots,only,mask_kind", MATRIX, ids=["%s-cb%d-%d-only%d-%s" % c for c in MATRIX])
def test_row_pack_equals_the_full_pack_indexed(monkeypatch, tmp_path, roads, cb, slots, only, mask_kind):
    _run_twins(monkeypatch, tmp_path, roads, cb, slots, only, mask_kind)


def test_all_true_rows_are_the_whole_full_tensor(tmp_path):
    scenes = [TEST_JSON, SCENE_407, P.parked_car_scene(tmp_path)]
    kw = dict(BASE, roadObservationAlgorithm=1, collisionBehaviour=1)
    full = P.make_gpu_sim(scenes, max_agents=64, **kw)
    rsim = P.make_gpu_sim(scenes, max_agents=64, **kw)
    try:
        assert full.direct_pack(only=True)
        _, g, rows = _attach_rows(rsim, "all", True)
        gen = torch.Generator().manual_seed(3)
        for k in range(5):
            a = _actions(gen, len(scenes), 64, full._device)
            full.action_tensor().to_torch().copy_(a)
            rsim.action_tensor().to_torch().copy_(a)
            full.step()
            rsim.step()
        torch.cuda.synchronize()
        g.check("all-true")
        _equal_bits(rows, full.packed_observations().view(-1, rows.shape[1]), "all-true rows vs the whole tensor")
    finally:
        full.close()
        rsim.close()


@pytest.fixture
def side_stream():
    """The step graph is captured and replayed on a stream of torch's own (the legacy null stream cannot be captured)."""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        yield st


def _discrete_twins(tmp_path, dynamics=0):
    scenes = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    kw = dict(BASE, roadObservationAlgorithm=1, collisionBehaviour=1, dynamicsModel=dynamics)
    return scenes, P.make_gpu_sim(scenes, max_agents=64, **kw), P.make_gpu_sim(scenes, max_agents=64, **kw)


OUTPUTS = ("action_tensor", "reward_tensor", "done_tensor", "info_tensor", "self_observation_tensor",
           "absolute_self_observation_tensor", "partner_observations_tensor", "agent_roadmap_tensor", "steps_remaining_tensor")


@pytest.mark.parametrize("model", ["classic", "delta_local"])
def test_discrete_actions_equal_the_torch_path(tmp_path, model, side_stream):
    from gpudrive_lab_amd.learner import action_table
    dyn = {"classic": 0, "delta_local": 2}[model]
    scenes, dev_sim, ref_sim = _discrete_twins(tmp_path, dyn)
    try:
        n = dev_sim.set_learner_rows()
        mask = ref_sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        assert n == int(mask.sum()) and n > 2
        table = action_table(model).cuda()
        gen = torch.Generator().manual_seed(5)
        # other slots hold values of their own: they must be left as they are
        junk = torch.rand(len(scenes), 64, 10, generator=gen).cuda()
        dev_sim.action_tensor().to_torch().copy_(junk)
        ref_sim.action_tensor().to_torch().copy_(junk)
        stat0 = dev_sim.stat(0)
        for k in range(12):
            idx = torch.randint(0, table.shape[0], (n,), generator=gen).cuda()
            before = dev_sim.action_tensor().to_torch().clone()
            dev_sim.set_discrete_actions(idx, table)
            act = ref_sim.action_tensor().to_torch()
            act[:, :, :3][mask] = table[idx]
            torch.cuda.synchronize()
            after = dev_sim.action_tensor().to_torch()
            _equal_bits(after[mask][:, :3], table[idx], "decoded rows")
            _equal_bits(after[~mask], before[~mask], "other slots")
            _equal_bits(after[mask][:, 3:], before[mask][:, 3:], "columns 3..9")
            dev_sim.step()
            ref_sim.step()
            torch.cuda.synchronize()
            for name in OUTPUTS:
                _equal_bits(getattr(dev_sim, name)().to_torch(), getattr(ref_sim, name)().to_torch(), "%s step %d" % (name, k))
        assert dev_sim.stat(0) - stat0 >= 11, "set_discrete_actions broke the graph replay"
        # indices outside the table: counted, their rows left alone, the others decoded
        bad0 = dev_sim.stat(45)
        idx = torch.randint(0, table.shape[0], (n,), generator=gen)
        idx[0], idx[n - 1] = -1, table.shape[0]
        idx = idx.cuda()
        before = dev_sim.action_tensor().to_torch().clone()
        dev_sim.set_discrete_actions(idx, table)
        torch.cuda.synchronize()
        after = dev_sim.action_tensor().to_torch()
        assert dev_sim.stat(45) - bad0 == 2
        _equal_bits(after[mask][[0, n - 1]], before[mask][[0, n - 1]], "rows with indices outside the table")
        _equal_bits(after[mask][1:n - 1, :3], table[idx[1:n - 1]], "rows with valid indices")
    finally:
        dev_sim.close()
        ref_sim.close()


def test_discrete_actions_refused_for_state_and_without_rows(tmp_path):
    from gpudrive_lab_amd.learner import action_table
    scenes = [TEST_JSON]
    sim = P.make_gpu_sim(scenes, max_agents=64, **dict(BASE, dynamicsModel=3))
    try:
        sim.set_learner_rows()
        idx = torch.zeros(sim._n_rows, dtype=torch.int64, device="cuda")
        with pytest.raises(NotImplementedError):
            sim.set_discrete_actions(idx, action_table("classic").cuda())
    finally:
        sim.close()
    sim = P.make_gpu_sim(scenes, max_agents=64, **BASE)
    try:
        n = sim.set_learner_rows()
        sim.clear_learner_rows()
        with pytest.raises(ValueError):
            sim.set_discrete_actions(torch.zeros(n, dtype=torch.int64, device="cuda"), action_table("classic").cuda())
        # the C entry itself, without rows
        from gpudrive_lab_amd import _capi
        t = action_table("classic").cuda()
        i = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
        assert sim._L.gd_set_discrete_actions(sim._h, i.data_ptr(), t.data_ptr(), t.shape[0]) == _capi.GD_ERR_INVALID
        # a wrong row count is refused and leaves no rows
        m = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        mu8 = m.to(torch.uint8).contiguous()
        assert sim._L.gd_set_learner_rows(sim._h, mu8.data_ptr(), int(m.sum()) + 1) == _capi.GD_ERR_INVALID
    finally:
        sim.close()


@pytest.mark.parametrize("reward_type", ["weighted_combination", "sparse_on_goal_achieved", "distance_to_logs"])
def test_flat_episode_outputs_equal_the_indexed_ones(tmp_path, reward_type):
    from gpudrive_lab_amd.episode import EpisodeTracker
    scenes = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    sim = P.make_gpu_sim(scenes, max_agents=64, **dict(BASE, roadObservationAlgorithm=1, collisionBehaviour=1))
    try:
        tr = EpisodeTracker(sim, reward_type=reward_type)
        mask = tr.controlled_agent_mask
        n = sim.set_learner_rows(mask)
        flat = dict(reward_rows=torch.full((n,), float("nan"), device="cuda"),
                    terminal_rows=torch.full((n,), 7, dtype=torch.uint8, device="cuda"),
                    truncated_rows=torch.full((n,), 7, dtype=torch.uint8, device="cuda"),
                    mask_rows=torch.full((n,), 7, dtype=torch.uint8, device="cuda"))
        for k, v in flat.items():
            setattr(tr._bufs, k, v.data_ptr())
        gen = torch.Generator().manual_seed(9)
        ends = 0
        for k in range(100):
            sim.action_tensor().to_torch().copy_(_actions(gen, len(scenes), 64, sim._device))
            r, t, u, m = tr.step()
            ends += int(tr.done_worlds.sum())
            torch.cuda.synchronize()
            _equal_bits(flat["reward_rows"], r[mask], "reward step %d" % k)
            for key, full in (("terminal_rows", t), ("truncated_rows", u), ("mask_rows", m)):
                assert torch.equal(flat[key], full[mask].to(torch.uint8)), "%s step %d" % (key, k)
        assert ends > 0
    finally:
        sim.close()


def test_device_learner_env_equals_the_reference_shaped_loop(tmp_path, side_stream):
    from gpudrive_lab_amd.episode import EpisodeTracker
    from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table
    scenes = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    kw = dict(BASE, roadObservationAlgorithm=1, collisionBehaviour=2)
    a_sim = P.make_gpu_sim(scenes, max_agents=128, **kw)
    b_sim = P.make_gpu_sim(scenes, max_agents=128, **kw)
    try:
        env = DeviceLearnerEnv(a_sim)
        table = action_table("classic").cuda()
        assert b_sim.direct_pack(only=True)

        def reference_setup():
            tr = EpisodeTracker(b_sim)
            return tr, tr.controlled_agent_mask

        tr, mask = reference_setup()
        obs = env.reset()
        _equal_bits(obs, b_sim.packed_observations()[mask], "reset")
        gen = torch.Generator().manual_seed(21)

        def run(steps, tag):
            nonlocal tr, mask
            s0 = a_sim.stat(0)
            for k in range(steps):
                idx = torch.randint(0, table.shape[0], (env.num_agents,), generator=gen).cuda()
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
                try:
                    out = env.step(idx)
                finally:
                    torch.cuda.set_sync_debug_mode(0)
                act = b_sim.action_tensor().to_torch()
                act[:, :, :3][mask] = table[idx]
                r, t, u, m = tr.step()
                ref = (b_sim.packed_observations()[mask], r[mask], t[mask], u[mask], m[mask])
                torch.cuda.synchronize()
                for name, x, y in zip(("obs", "rewards", "terminals", "truncations", "masks"), out, ref):
                    _equal_bits(x.to(torch.float32) if x.dtype == torch.bool else x,
                                y.to(torch.float32) if y.dtype == torch.bool else y, "%s %s step %d" % (tag, name, k))
            assert a_sim.stat(0) - s0 == steps, "every learner step is a graph replay"

        run(120, "first")
        s_a, s_b = env.pop_stats(), tr.pop_stats()
        assert s_a and s_a.keys() == s_b.keys(), (s_a, s_b)
        for key in s_a:  # (running sums of float atomics: the order of the worlds' additions may differ)
            assert s_a[key] == pytest.approx(s_b[key], rel=1e-5), key
        new = scenes[2:] + scenes[:2]
        obs = env.resample(new)
        b_sim.set_maps(new)
        tr, mask = reference_setup()
        _equal_bits(obs, b_sim.packed_observations()[mask], "resample")
        run(20, "resampled")
    finally:
        a_sim.close()
        b_sim.close()
