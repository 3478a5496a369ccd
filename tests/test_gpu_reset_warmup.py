"""GPU suite: the warm-up of the device auto-reset (gd_episode_set_warmup; EpisodeTracker / DeviceLearnerEnv init_steps).

Everything is held bit for bit to what the host composition of existing pieces leaves behind, on the same scenes and the same
scripted actions:
  - "all_worlds": step, EpisodeTracker(auto_reset=False) bookkeeping, done_worlds to the host, sim.reset(list) +
    advance_log_playback(k) -- the reference's PufferGPUDrive.step() / env.reset(env_idx_list) with init_steps = k;
  - "reset_worlds": a warmed world equals that world of a freshly built simulator advanced k steps, every other world the
    same run without the warm-up.
Every exported tensor is compared after every learner step: the state, the observations, the action tensor (its uncontrolled
slots keep the logged action the warm-up left), the tracker's buffers, and the learner rows, BEV and LiDAR where attached."""
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
SIM_TENSORS = ("action_tensor", "reward_tensor", "done_tensor", "info_tensor", "steps_remaining_tensor",
               "self_observation_tensor", "absolute_self_observation_tensor", "partner_observations_tensor",
               "agent_roadmap_tensor")
# what the learner rows with only = 1 leave current (the raw partner and road rows are not written any more)
STATE_TENSORS = SIM_TENSORS[:7]
TRACKER_TENSORS = ("rewards", "terminals", "truncations", "masks", "agent_episode_returns", "episode_lengths",
                   "collided_in_episode", "offroad_in_episode", "live_agent_mask", "done_worlds")
D_ROW = lambda A: 6 + (A - 1) * 6 + 200 * 13


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


def _scenes(tmp_path):
    return [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]


def _make(scenes, roads, cb, slots, bev=False, lidar=False):
    knn_order, algo, _ = ROADS[roads]
    kw = dict(BASE, roadObservationAlgorithm=algo, collisionBehaviour=cb)
    gkw = dict(max_agents=slots, knn_order=knn_order)
    if bev:
        gkw["enable_bev"] = True
    if lidar:
        kw["enableLidar"] = 1
        gkw["lidar_half_angle"] = 0.5
    sim = P.make_gpu_sim(scenes, **gkw, **kw)
    if bev:
        sim.bev_observation_tensor()  # created (and rasterised) on the first call
    return sim


def _sim_tensors(sim, bev=False, lidar=False, names=SIM_TENSORS):
    names = names + (("bev_observation_tensor",) if bev else ()) + (("lidar_tensor",) if lidar else ())
    return {n: getattr(sim, n)().to_torch() for n in names}


def _compare_sims(a, b, what, worlds=None, bev=False, lidar=False, names=SIM_TENSORS):
    ta, tb = _sim_tensors(a, bev, lidar, names), _sim_tensors(b, bev, lidar, names)
    for n in ta:
        x, y = ta[n], tb[n]
        if worlds is not None:
            x, y = x[worlds], y[worlds]
        _equal_bits(x, y, "%s %s" % (what, n))


def _compare_trackers(a, b, what, worlds=None):
    for n in TRACKER_TENSORS:
        x, y = getattr(a, n), getattr(b, n)
        if worlds is not None:
            x, y = x[worlds], y[worlds]
        _equal_bits(x, y, "%s tracker.%s" % (what, n))


def _act(sim, mask, gen):
    """Scripted actions for the controlled slots only (columns 0..2, as the learner writes them): every other slot keeps what
    the action tensor holds -- after a warm-up, the logged action of its last step."""
    W, A = mask.shape
    a = torch.zeros(W, A, 3)
    a[..., 0] = torch.rand(W, A, generator=gen) * 5.0 - 3.0
    a[..., 1] = torch.rand(W, A, generator=gen) * 1.4 - 0.7
    return a.to(sim._device)


def _write(sim, mask, a):
    act = sim.action_tensor().to_torch()
    act[:, :, :3][mask] = a[mask]


def _attach_rows(sim, mask):
    n = sim.set_learner_rows(mask)
    return sim.direct_pack_rows(only=False, out=torch.empty((max(n, 1) * D_ROW(sim._A),), device=sim._device))


def _host_reset(sim, tracker, k):
    """The host composition of one reset: the finished worlds to the host, sim.reset(list), advance_log_playback(k)."""
    done = tracker.done_worlds.cpu().nonzero().flatten().tolist()
    if done:
        sim.reset(done)
        if k > 0:
            sim.advance_log_playback(k)
    return done


def _all_worlds_case(monkeypatch, tmp_path, roads, cb, slots, k, steps=130, bev=False, lidar=False, rows=False, pre=80,
                     scope="all_worlds"):
    from gpudrive_lab_amd.episode import EpisodeTracker
    for key, v in ROADS[roads][2].items():
        monkeypatch.setenv(key, v)
    scenes = _scenes(tmp_path)
    W = len(scenes)
    dsim = _make(scenes, roads, cb, slots, bev, lidar)
    hsim = _make(scenes, roads, cb, slots, bev, lidar)
    try:
        mask = dsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        if rows:
            drows, hrows = _attach_rows(dsim, mask), _attach_rows(hsim, mask)
        for s in (dsim, hsim):
            s.advance_log_playback(pre)  # the first episode ends inside the compared steps
        td = EpisodeTracker(dsim, init_steps=k, warmup=scope)
        th = EpisodeTracker(hsim, auto_reset=False)
        gen = torch.Generator().manual_seed(17 + k)
        events, warmed = 0, 0
        for step in range(steps):
            a = _act(dsim, mask, gen)
            _write(dsim, mask, a)
            _write(hsim, mask, a)
            td.step()
            th.step()
            done = _host_reset(hsim, th, k)
            if done:
                events += 1
                if scope == "reset_worlds":
                    assert len(done) == W, "step %d: the composition holds for reset_worlds only when every world ends" % step
                warmed += W if k > 0 else 0
            if step == 20:  # a host reset of one world: from here on the worlds end on different steps
                for s in (dsim, hsim):
                    s.reset([0])
            torch.cuda.synchronize()
            what = "%s cb%d A=%d k=%d step %d" % (roads, cb, slots, k, step)
            _compare_sims(dsim, hsim, what, bev=bev, lidar=lidar)
            _compare_trackers(td, th, what)
            if rows:
                _equal_bits(drows, hrows, what + " learner rows")
        assert events >= 2, "fewer than two reset events (%d)" % events
        assert dsim.stat(46) == warmed, (dsim.stat(46), warmed)
        print("WARMUP all_worlds %s cb%d A=%d k=%d events=%d warmed=%d" % (roads, cb, slots, k, events, warmed))
    finally:
        dsim.close()
        hsim.close()


ALL_MATRIX = ([("linear", cb, 64, 11, "") for cb in (0, 1, 2)] +
              [("linear", 1, 128, 1, ""), ("set_order_fused", 1, 64, 11, ""), ("set_order_row_kernel", 0, 64, 1, ""),
               ("ref_order", 1, 64, 11, ""), ("ref_order", 2, 128, 1, ""),
               ("linear", 1, 64, 11, "rows"), ("ref_order", 0, 128, 11, "rows"), ("linear", 1, 64, 11, "bev"),
               ("linear", 2, 64, 1, "lidar")])


@pytest.mark.parametrize("roads,cb,slots,k,extra", ALL_MATRIX, ids=["%s-cb%d-%d-k%d-%s" % c for c in ALL_MATRIX])
def test_all_worlds_equals_the_host_composition(monkeypatch, tmp_path, roads, cb, slots, k, extra):
    _all_worlds_case(monkeypatch, tmp_path, roads, cb, slots, k, bev=extra == "bev", lidar=extra == "lidar",
                     rows=extra == "rows")


@pytest.mark.parametrize("roads,cb,slots", [("linear", 1, 64), ("ref_order", 0, 128), ("set_order_fused", 2, 64)])
def test_reset_worlds_staggered(monkeypatch, tmp_path, roads, cb, slots):
    """Worlds 1 and 3 are reset early by the host: the two halves reach the step limit on different steps.  A warmed world
    must equal that world of a fresh simulator advanced k steps (learner rows and action slots included); a world not warmed
    so far must equal the same run with k = 0."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    for key, v in ROADS[roads][2].items():
        monkeypatch.setenv(key, v)
    k = 11
    scenes = _scenes(tmp_path)
    W = len(scenes)
    dsim, zsim, fsim = (_make(scenes, roads, cb, slots) for _ in range(3))
    try:
        mask = dsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        drows, zrows = _attach_rows(dsim, mask), _attach_rows(zsim, mask)
        n_w = mask.sum(1).tolist()
        first = [sum(n_w[:w]) for w in range(W)]
        assert fsim.direct_pack(only=False)
        fsim.advance_log_playback(k)  # what a warmed world must look like
        fpack = fsim.packed_observations()
        for s in (dsim, zsim):
            s.advance_log_playback(70)
        td = EpisodeTracker(dsim, init_steps=k)  # "reset_worlds" is the default
        tz = EpisodeTracker(zsim)
        gen = torch.Generator().manual_seed(5)
        ever = torch.zeros(W, dtype=torch.bool)
        events = []
        for step in range(120):
            if step == 5:
                for s in (dsim, zsim):
                    s.reset([1, 3])
            a = _act(dsim, mask, gen)
            _write(dsim, mask, a)
            _write(zsim, mask, a)
            td.step()
            tz.step()
            torch.cuda.synchronize()
            what = "%s cb%d A=%d step %d" % (roads, cb, slots, step)
            now = td.done_worlds.cpu().bool()
            fresh = (~ever).nonzero().flatten().tolist()  # never warmed before this step: still the k = 0 run
            if fresh:
                _compare_trackers(td, tz, what, worlds=fresh)
            keep = [w for w in fresh if not now[w]]
            if keep:
                _compare_sims(dsim, zsim, what + " unwarmed", worlds=keep)
                for w in keep:
                    _equal_bits(drows[first[w]:first[w] + n_w[w]], zrows[first[w]:first[w] + n_w[w]], "%s rows w%d" % (what, w))
            for w in now.nonzero().flatten().tolist():
                _compare_sims(dsim, fsim, what + " warmed", worlds=[w])
                _equal_bits(drows[first[w]:first[w] + n_w[w]], fpack[w][mask[w]], "%s warmed rows w%d" % (what, w))
            if bool(now.any()):
                events.append((step, now.nonzero().flatten().tolist()))
            ever |= now
        assert bool(ever.all()), events
        assert len({s for s, _ in events}) >= 2, events
        assert dsim.stat(46) == sum(len(ws) for _, ws in events), (dsim.stat(46), events)
        assert zsim.stat(46) == 0
        print("WARMUP reset_worlds %s cb%d A=%d events=%s" % (roads, cb, slots, events))
    finally:
        for s in (dsim, zsim, fsim):
            s.close()


@pytest.mark.parametrize("scope", ["reset_worlds", "all_worlds"])
def test_zero_init_steps_is_todays_tracker(tmp_path, scope):
    from gpudrive_lab_amd.episode import EpisodeTracker
    scenes = _scenes(tmp_path)
    dsim, zsim = _make(scenes, "linear", 1, 64), _make(scenes, "linear", 1, 64)
    try:
        mask = dsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        for s in (dsim, zsim):
            s.advance_log_playback(80)
        td, tz = EpisodeTracker(dsim, init_steps=0, warmup=scope), EpisodeTracker(zsim)
        gen = torch.Generator().manual_seed(3)
        ends = 0
        for step in range(110):
            a = _act(dsim, mask, gen)
            _write(dsim, mask, a)
            _write(zsim, mask, a)
            td.step()
            tz.step()
            ends += int(tz.done_worlds.sum())
            torch.cuda.synchronize()
            _compare_sims(dsim, zsim, "k=0 step %d" % step)
            _compare_trackers(td, tz, "k=0 step %d" % step)
        assert ends > 0
        assert dsim.stat(46) == 0 and zsim.stat(46) == 0
    finally:
        dsim.close()
        zsim.close()


def test_ninety_init_steps_warms_every_step(monkeypatch, tmp_path):
    """k = 90 leaves one step of the episode: every learner step ends every world and warms it again."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    scenes = _scenes(tmp_path)
    W = len(scenes)
    dsim, hsim = _make(scenes, "linear", 1, 64), _make(scenes, "linear", 1, 64)
    try:
        mask = dsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        for s in (dsim, hsim):
            s.advance_log_playback(90)
        td, th = EpisodeTracker(dsim, init_steps=90), EpisodeTracker(hsim, auto_reset=False)
        gen = torch.Generator().manual_seed(90)
        for step in range(4):
            a = _act(dsim, mask, gen)
            _write(dsim, mask, a)
            _write(hsim, mask, a)
            td.step()
            th.step()
            assert _host_reset(hsim, th, 90) == list(range(W)), step
            torch.cuda.synchronize()
            _compare_sims(dsim, hsim, "k=90 step %d" % step)
            _compare_trackers(td, th, "k=90 step %d" % step)
        for step in range(100):
            a = _act(dsim, mask, gen)
            _write(dsim, mask, a)
            td.step()
        torch.cuda.synchronize()
        assert bool(td.done_worlds.all())
        assert dsim.stat(46) == 104 * W
        assert bool((dsim.steps_remaining_tensor().to_torch()[mask] == 1).all())
    finally:
        dsim.close()
        hsim.close()


@pytest.fixture
def side_stream():
    """The step graph is captured and replayed on a stream of torch's own (the legacy null stream cannot be captured)."""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        yield st


@pytest.mark.parametrize("scope", ["all_worlds", "reset_worlds"])
def test_device_learner_env_with_init_steps(tmp_path, side_stream, scope):
    """DeviceLearnerEnv(init_steps=11) against the loop built from existing pieces: reset every world + advance_log_playback
    at setup, then step, bookkeeping, done worlds to the host, sim.reset(list) + advance_log_playback(11).  With
    "reset_worlds" the composition holds while every world ends on the same step (they all start together here)."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table
    k = 11
    scenes = _scenes(tmp_path)
    W = len(scenes)
    kw = dict(BASE, roadObservationAlgorithm=1, collisionBehaviour=2)
    a_sim = P.make_gpu_sim(scenes, max_agents=128, **kw)
    b_sim = P.make_gpu_sim(scenes, max_agents=128, **kw)
    try:
        for s in (a_sim, b_sim):  # somewhere inside an episode: construction must reset every world first
            s.advance_log_playback(30)
        env = DeviceLearnerEnv(a_sim, init_steps=k, warmup=scope)
        table = action_table("classic").cuda()
        assert b_sim.direct_pack(only=True)

        def reference_setup(reset):
            tr = EpisodeTracker(b_sim, auto_reset=False)
            if reset:
                b_sim.reset(list(range(W)))
            b_sim.advance_log_playback(k)
            return tr, tr.controlled_agent_mask

        tr, mask = reference_setup(True)
        obs = env.reset()
        _equal_bits(obs, b_sim.packed_observations()[mask], "setup")
        _compare_sims(a_sim, b_sim, "setup", names=STATE_TENSORS)
        gen = torch.Generator().manual_seed(21)

        def run(steps, tag):
            s0, events = a_sim.stat(0), 0
            for step in range(steps):
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
                done = _host_reset(b_sim, tr, k)
                if done:
                    events += 1
                    assert scope == "all_worlds" or len(done) == W, (step, done)
                    ref = (b_sim.packed_observations()[mask],) + ref[1:]
                torch.cuda.synchronize()
                for name, x, y in zip(("obs", "rewards", "terminals", "truncations", "masks"), out, ref):
                    _equal_bits(x, y, "%s %s step %d" % (tag, name, step))
                _compare_sims(a_sim, b_sim, "%s step %d" % (tag, step), names=STATE_TENSORS)
            assert a_sim.stat(0) - s0 == steps, "every learner step is a graph replay"
            return events

        assert run(120, "first") >= 1
        assert a_sim.stat(46) > 0
        new = scenes[2:] + scenes[:2]
        obs = env.resample(new)
        b_sim.set_maps(new)
        tr, mask = reference_setup(False)
        _equal_bits(obs, b_sim.packed_observations()[mask], "resample")
        run(20, "resampled")
    finally:
        a_sim.close()
        b_sim.close()
