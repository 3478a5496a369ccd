"""GPU suite: conditioned learner rows -- the reward-conditioned policy's [N, D + 3] rows (ego 6 | the slot's 3 reward weights |
partners | road points) written in place by the step's kernels (gd_attach_packed_rows_conditioned,
SimManager.direct_pack_rows(reward_weights=...), gpudrive_lab_amd.learner.ConditionedLearnerEnv).

Everything is held bit for bit to the paths the engine already had: `packed_observations(reward_weights=w)[mask]` of the
same simulator (only = 0) or of a twin on the same scenes and actions (only = 1), whose tracker has the same seed; and the
[N, D] learner rows of a twin, which must equal the conditioned rows outside the three weight columns."""
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
D_ROW = lambda A: 6 + (A - 1) * 6 + 200 * 13
PLAIN_COLS = lambda A: torch.cat([torch.arange(6), torch.arange(9, D_ROW(A) + 3)])  # the conditioned columns outside the weights


def _bits(t):
    t = t.contiguous()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int32)


def _equal_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    x, y = _bits(a), _bits(b)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        raise AssertionError("%s: %d elements differ, first at %s" % (what, bad.shape[0], bad[0].tolist()))


def _actions(gen, W, A, dev):
    a = torch.zeros(W, A, 10)
    a[..., 0] = torch.rand(W, A, generator=gen) * 5.0 - 3.0
    a[..., 1] = torch.rand(W, A, generator=gen) * 1.4 - 0.7
    return a.to(dev)


def _mask(kind, sim, seed=7):
    W, A = sim._W, sim._A
    dev = sim._device
    cont = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
    if kind == "controlled":
        return cont
    if kind == "random":  # padding and Static slots included
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(W, A, generator=g) < 0.4).to(dev)
    if kind == "all":
        return torch.ones(W, A, dtype=torch.bool, device=dev)
    if kind.startswith("first"):  # n rows: the last one ends against the canary at each 16-byte phase
        n = int(kind[5:])
        m = torch.zeros(W * A, dtype=torch.bool, device=dev)
        m[cont.view(-1).nonzero().view(-1)[:n]] = True
        return m.view(W, A)
    return torch.zeros(W, A, dtype=torch.bool, device=dev)


class _Guarded:
    """A NaN-filled row buffer with a canary tail."""

    def __init__(self, n, R, dev):
        self.n, self.R = n, R
        self.buf = torch.full((n * R + CANARY,), float("nan"), dtype=torch.float32, device=dev)
        self.buf.view(torch.int32)[n * R:] = CANARY_BITS

    def check(self, what):
        rows = self.buf[:self.n * self.R]
        assert not bool(torch.isnan(rows).any()), "%s: a learner row was not written" % what
        assert bool((self.buf.view(torch.int32)[self.n * self.R:] == CANARY_BITS).all()), "%s: write past the row buffer" % what


def _tracker(sim):
    from gpudrive_lab_amd.episode import EpisodeTracker
    return EpisodeTracker(sim, reward_type="reward_conditioned", condition_mode="random", seed=5)


def _attach(csim, psim, mask_kind, only, tc):
    """Conditioned rows on csim (weights: its tracker's), [N, D] rows with only = 0 on the twin psim, same mask."""
    mask = _mask(mask_kind, csim)
    n = csim.set_learner_rows(mask)
    assert n == int(mask.sum()) and psim.set_learner_rows(mask) == n
    A = csim._A
    g = _Guarded(n, D_ROW(A) + 3, csim._device)
    rows = csim.direct_pack_rows(only=only, out=g.buf, reward_weights=tc.reward_weights_tensor)
    assert tuple(rows.shape) == (n, D_ROW(A) + 3)
    plain = psim.direct_pack_rows(only=False)
    assert tuple(plain.shape) == (n, D_ROW(A))
    return mask, g, rows, plain


def _compare(csim, psim, tc, tp, mask, g, rows, plain, only, what):
    torch.cuda.synchronize()
    g.check(what)
    ref_sim, ref_tr = (psim, tp) if only else (csim, tc)
    _equal_bits(tc.reward_weights_tensor, tp.reward_weights_tensor, "%s: weights of the twins" % what)
    _equal_bits(rows, ref_sim.packed_observations(reward_weights=ref_tr.reward_weights_tensor)[mask], what)
    _equal_bits(rows[:, PLAIN_COLS(csim._A).to(rows.device)], plain, "%s: the [N, D] rows" % what)


def _run_twins(monkeypatch, tmp_path, roads, cb, slots, only, mask_kind):
    knn_order, algo, env = ROADS[roads]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scenes = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    kw = dict(BASE, roadObservationAlgorithm=algo, collisionBehaviour=cb)
    csim = P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, **kw)
    psim = P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, **kw)
    try:
        tc, tp = _tracker(csim), _tracker(psim)
        mask, g, rows, plain = _attach(csim, psim, mask_kind, only, tc)
        _compare(csim, psim, tc, tp, mask, g, rows, plain, only, "attach")
        for s in (csim, psim):
            s.advance_log_playback(WARM)
        _compare(csim, psim, tc, tp, mask, g, rows, plain, only, "log playback")
        gen = torch.Generator().manual_seed(11)
        W = len(scenes)
        resets = 0
        for k in range(STEPS):
            a = _actions(gen, W, slots, csim._device)
            csim.action_tensor().to_torch().copy_(a)
            psim.action_tensor().to_torch().copy_(a)
            tc.step()
            tp.step()
            resets += int(tc.done_worlds.sum())
            if k == 8:  # host redraws of some worlds, between steps
                for t in (tc, tp):
                    t.set_reward_weights([1, 2], condition_mode="preset", agent_type="cautious")
                _compare(csim, psim, tc, tp, mask, g, rows, plain, only, "preset redraw")
            if k == 12:
                for s in (csim, psim):
                    s.reset([0, W - 1])
            if k == 16:
                for t in (tc, tp):
                    t.set_reward_weights([0, W - 1], condition_mode="fixed", agent_type=torch.tensor([-0.25, 1.5, -0.75]))
                _compare(csim, psim, tc, tp, mask, g, rows, plain, only, "fixed redraw")
            if k == 18:
                for s in (csim, psim):
                    s.deleteAgents({1: [0]})
            if k == 22:
                for t in (tc, tp):
                    t.set_reward_weights(None, condition_mode="random")
            if k == 26:  # new scenes: trackers and rows set (and attached) again, as the caller must
                for s in (csim, psim):
                    s.set_maps(scenes[1:] + scenes[:1])
                tc, tp = _tracker(csim), _tracker(psim)
                mask, g, rows, plain = _attach(csim, psim, mask_kind, only, tc)
            _compare(csim, psim, tc, tp, mask, g, rows, plain, only, "step %d" % k)
        assert resets > 0, "no world was reset by the tracker"
        if only:
            with pytest.raises(NotImplementedError):
                csim.packed_observations(reward_weights=tc.reward_weights_tensor)
        print("COND_ROWS %s cb%d A=%d only=%d mask=%s rows=%d resets=%d" % (roads, cb, slots, only, mask_kind, g.n, resets))
    finally:
        csim.close()
        psim.close()


MATRIX = ([("linear", cb, A, only, "controlled") for cb in (0, 1, 2) for A in (64, 128) for only in (0, 1)] +
          [(r, 1, 64, only, "controlled") for r in ("set_order_fused", "set_order_row_kernel") for only in (0, 1)] +
          [("set_order_fused", 1, 128, 1, "controlled"), ("set_order_row_kernel", 1, 128, 0, "controlled")] +
          [("ref_order", 1, A, only, "controlled") for A in (64, 128) for only in (0, 1)] +
          [("linear", 1, 64, 1, m) for m in ("random", "all", "none")] +
          [("ref_order", 1, 128, 0, m) for m in ("random", "all", "none")] +
          [("set_order_fused", 2, 64, 1, "random"), ("set_order_row_kernel", 0, 128, 1, "random")] +
          [("linear", 1, 64, 1, "first%d" % n) for n in (1, 2, 3)] +
          [("linear", 1, 128, 0, "first%d" % n) for n in (1, 2, 3)] +
          [("set_order_fused", 1, 64, 1, "first3"), ("ref_order", 1, 64, 1, "first1")])


@pytest.mark.parametrize("roads,cb,slots,only,mask_kind", MATRIX, ids=["%s-cb%d-%d-only%d-%s" % c for c in MATRIX])
def test_conditioned_rows_equal_the_conditioned_pack_indexed(monkeypatch, tmp_path, roads, cb, slots, only, mask_kind):
    _run_twins(monkeypatch, tmp_path, roads, cb, slots, only, mask_kind)


def test_conditioned_attach_checks(tmp_path):
    from gpudrive_lab_amd import _capi
    sim = P.make_gpu_sim([TEST_JSON, SCENE_407], max_agents=64, **dict(BASE, roadObservationAlgorithm=1))
    try:
        tr = _tracker(sim)
        out = torch.empty(64 * 2 * (D_ROW(64) + 3), device="cuda")
        w = tr.reward_weights_tensor
        # without learner rows, with a NULL weights pointer, with a buffer one float short
        assert sim._L.gd_attach_packed_rows_conditioned(sim._h, out.data_ptr(), out.numel() * 4, 1, w.data_ptr()) == _capi.GD_ERR_INVALID
        n = sim.set_learner_rows()
        assert sim._L.gd_attach_packed_rows_conditioned(sim._h, out.data_ptr(), out.numel() * 4, 1, None) == _capi.GD_ERR_INVALID
        short = (n * (D_ROW(64) + 3) - 1) * 4
        assert sim._L.gd_attach_packed_rows_conditioned(sim._h, out.data_ptr(), short, 1, w.data_ptr()) == _capi.GD_ERR_INVALID
        rows = sim.direct_pack_rows(only=False, reward_weights=w)
        assert tuple(rows.shape) == (n, D_ROW(64) + 3)
        sim.step()
        torch.cuda.synchronize()
        _equal_bits(rows, sim.packed_observations(reward_weights=w)[sim._learner_mask], "attached")
        # gd_attach_packed(NULL) detaches either kind; an [N, D] attachment replaces it
        sim.direct_pack_off()
        plain = sim.direct_pack_rows(only=False)
        sim.step()
        torch.cuda.synchronize()
        assert tuple(plain.shape) == (n, D_ROW(64))
        _equal_bits(plain, sim.packed_observations()[sim._learner_mask], "the [N, D] rows that replaced them")
    finally:
        sim.close()


@pytest.fixture
def side_stream():
    """The step graph is captured and replayed on a stream of torch's own (the legacy null stream cannot be captured)."""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        yield st


ENV_CASES = [(k, mode) for k in (0, 11) for mode in ("random", "preset", "fixed")]


@pytest.mark.parametrize("init_steps,mode", ENV_CASES, ids=["k%d-%s" % c for c in ENV_CASES])
def test_conditioned_learner_env_equals_the_reference_shaped_loop(tmp_path, side_stream, init_steps, mode):
    """ConditionedLearnerEnv against tracker + full conditioned pack + [mask] on a twin, and its rows outside the weight
    columns against DeviceLearnerEnv on a third simulator, over 120 steps, a resample and 20 more steps."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    from gpudrive_lab_amd.learner import ConditionedLearnerEnv, DeviceLearnerEnv, action_table
    agent_type = {"random": None, "preset": "aggressive", "fixed": torch.tensor([-0.5, 1.25, -0.125])}[mode]
    scenes = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    W = len(scenes)
    kw = dict(BASE, roadObservationAlgorithm=1, collisionBehaviour=2)
    a_sim, b_sim, c_sim = (P.make_gpu_sim(scenes, max_agents=128, **kw) for _ in range(3))
    try:
        if init_steps:
            for s in (a_sim, b_sim, c_sim):  # somewhere inside an episode: construction must reset every world first
                s.advance_log_playback(30)
        env = ConditionedLearnerEnv(a_sim, init_steps=init_steps, condition_mode=mode, agent_type=agent_type)
        plain = DeviceLearnerEnv(c_sim, init_steps=init_steps)
        table = action_table("classic").cuda()
        assert b_sim.direct_pack(only=True)
        cols = PLAIN_COLS(128).cuda()

        def reference_setup(reset):
            if reset and init_steps:
                b_sim.reset(list(range(W)))
            tr = EpisodeTracker(b_sim, reward_type="reward_conditioned", condition_mode=mode, agent_type=agent_type,
                                init_steps=init_steps)
            if init_steps:
                b_sim.advance_log_playback(init_steps)
            return tr, tr.controlled_agent_mask

        tr, mask = reference_setup(True)
        obs = env.reset()
        plain.reset()
        assert env.reward_weights_tensor is env.tracker.reward_weights_tensor
        assert tuple(obs.shape) == (env.num_agents, D_ROW(128) + 3)

        def ref_obs():
            return b_sim.packed_observations(reward_weights=tr.reward_weights_tensor)[mask]

        _equal_bits(obs, ref_obs(), "setup")
        _equal_bits(obs[:, cols], plain.obs, "setup: the [N, D] rows")
        gen = torch.Generator().manual_seed(21)

        def run(steps, tag):
            s0 = a_sim.stat(0)
            for k in range(steps):
                idx = torch.randint(0, table.shape[0], (env.num_agents,), generator=gen).cuda()
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
                try:
                    out = env.step(idx)
                    p_out = plain.step(idx)
                finally:
                    torch.cuda.set_sync_debug_mode(0)
                act = b_sim.action_tensor().to_torch()
                act[:, :, :3][mask] = table[idx]
                r, t, u, m = tr.step()
                ref = (ref_obs(), r[mask], t[mask], u[mask], m[mask])
                torch.cuda.synchronize()
                for name, x, y in zip(("obs", "rewards", "terminals", "truncations", "masks"), out, ref):
                    _equal_bits(x, y, "%s %s step %d" % (tag, name, k))
                _equal_bits(out[0][:, cols], p_out[0], "%s step %d: the [N, D] rows" % (tag, k))
                for name, x, y in zip(("terminals", "truncations", "masks"), out[2:], p_out[2:]):
                    _equal_bits(x, y, "%s %s step %d: DeviceLearnerEnv" % (tag, name, k))
                if k == 50:  # a host redraw of two worlds in the environment's own mode
                    env.set_reward_weights([1, 3])
                    tr.set_reward_weights([1, 3], condition_mode=mode, agent_type=agent_type)
                    torch.cuda.synchronize()
                    _equal_bits(env.obs, ref_obs(), "%s set_reward_weights" % tag)
            assert a_sim.stat(0) - s0 == steps, "every learner step is a graph replay"

        run(120, "first")
        s_a, s_b = env.pop_stats(), tr.pop_stats()
        assert s_a and s_a.keys() == s_b.keys(), (s_a, s_b)
        for key in s_a:  # (running sums of float atomics: the order of the worlds' additions may differ)
            assert s_a[key] == pytest.approx(s_b[key], rel=1e-5), key
        new = scenes[2:] + scenes[:2]
        obs = env.resample(new)
        plain.resample(new)
        b_sim.set_maps(new)
        tr, mask = reference_setup(False)
        _equal_bits(obs, ref_obs(), "resample")
        _equal_bits(obs[:, cols], plain.obs, "resample: the [N, D] rows")
        run(20, "resampled")
    finally:
        a_sim.close()
        b_sim.close()
        c_sim.close()
