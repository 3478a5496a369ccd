"""GPU suite: the set-up of the rank path run by the state step (csrc/rank_setup.hpp; k_world_step's FOLD instantiations in
csrc/kernels.hip) instead of k_knn_scan's launch.  Where the set-up runs may never show in a result, so every case runs twin
simulators on the same scenes and the same actions -- one as it is by default (the set-up inside k_world_step, the rank path
starting with k_knn_rank), one created under GPUDRIVE_RANK_SCAN_KERNEL=1 (the separate launch, no set-up in the state step) --
and requires after every pass: agent_roadmap_tensor, self_observation, partner_observations, reward, done and info (and every
other exported tensor) bit-equal, the bounds audit of the rank path (gd_stat 21) at zero in both, the same number of checkpoint
rows written by the set-up (gd_stat 22), and the same road path per agent (debug_road_path(): candidate counts, fallback,
out of reach).  The cases are the smallest that reach every branch of the set-up: own checkpoints of either set, a donor's,
bounded afresh, out of reach of every road, the fallback raised for a small world, partial waves, two halves per workgroup,
reset passes, rebuilt worlds and the gated reset pass of the episode tracker.  tests/test_rank_setup_fn.py holds the per-lane
decision on the host."""
import json

import numpy as np
import pytest

from gpudrive_lab_amd import synth
from tests import parity as P
from tests import ref_cases as RC
from tests import road_cases as RCS
from tests.test_gpu_rank_candidates import BENCH
from tests.test_gpu_rank_deal import EXPORTED, _close

pytestmark = pytest.mark.gpu

STAT_AUDIT, STAT_ROWS, STAT_FOLDED = 21, 22, 47
NAMED = ["agent_roadmap_tensor", "self_observation_tensor", "partner_observations_tensor", "reward_tensor", "done_tensor", "info_tensor"]


def _twins(monkeypatch, scenes, slots, min_roads=200, **kw):
    """(the default simulator: the set-up in the state step; the one whose set-up is k_knn_scan's launch)"""
    monkeypatch.setenv("GPUDRIVE_RANK_MIN_ROADS", str(min_roads))
    monkeypatch.delenv("GPUDRIVE_RANK_SCAN_KERNEL", raising=False)
    a = P.make_gpu_sim(scenes, max_agents=slots, **kw)
    monkeypatch.setenv("GPUDRIVE_RANK_SCAN_KERNEL", "1")  # read once, when the engine is created
    b = P.make_gpu_sim(scenes, max_agents=slots, **kw)
    monkeypatch.delenv("GPUDRIVE_RANK_SCAN_KERNEL")
    assert a.stat(7) == 1 and b.stat(7) == 1, "the rank path is off"
    assert a.stat(STAT_FOLDED) == 1 and b.stat(STAT_FOLDED) == 0, "which twin runs the set-up in the state step"
    return a, b


def _same(a, b, tag, log=None, names=None):
    """After a pass: the twins bit-equal, audit zero, the same rows and road paths.  Returns the road paths."""
    assert set(NAMED) <= set(EXPORTED)
    for name in names or EXPORTED:
        x, y = RC.as_np(getattr(a, name)()), RC.as_np(getattr(b, name)())
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, name)
        same = np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)
        assert same.all(), "%s: %s differs between the twins in %d bytes, first at byte %d" % (tag, name, int((~same).sum()), int(np.argmin(same)))
    pa, pb = a.debug_road_path(), b.debug_road_path()
    assert np.array_equal(pa, pb), "%s: the twins' road paths differ at %s" % (tag, np.argwhere(pa != pb)[:4].tolist())
    assert a.stat(STAT_AUDIT) == 0 and b.stat(STAT_AUDIT) == 0, "%s: bounds audit of the rank path: %d / %d" % (tag, a.stat(STAT_AUDIT), b.stat(STAT_AUDIT))
    ra, rb = a.stat(STAT_ROWS), b.stat(STAT_ROWS)
    assert ra == rb, "%s: the set-up wrote %d rows in the state step, %d as a launch of its own" % (tag, ra, rb)
    if log is not None:
        live = np.arange(pa.shape[1])[None, :] < RC.as_np(a.shape_tensor())[:, 0:1]
        log.append((tag, int(((pa > 0) & live).sum()), ra, int(((pa <= 0) & (pa != -3) & live).sum()), int(((pa == -3) & live).sum())))
    return pa


def _steps(a, b, steps, seed, log, tag=""):
    rng = np.random.default_rng(seed)
    W, A = a.debug_road_path().shape
    for k in range(steps):
        act = P.random_actions(rng, W, A, 0)
        for s in (a, b):
            RC.write_actions(s, act)
            s.step()
        _same(a, b, "%sstep %d" % (tag, k + 1), log)


def _scene(tmp_path, name, n_agents, n_poly, pts, seed):
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps(synth.make_scene(seed, n_agents=n_agents, n_polylines=n_poly, pts_per_polyline=pts)))
    return str(p)


def test_nine_bench_worlds_with_the_oracle(oracle_mod, tmp_path, monkeypatch):
    """Nine of the bench's worlds x 64 agents, twelve steps with a whole-batch reset after the fifth and a reset of one world
    after the ninth; the default twin in lockstep with the oracle (the other twin takes the oracle's state too, so every
    step is followed by a reset pass of both).  The first selection bounds every agent afresh (a row each); from then on every
    agent is bounded by its own checkpoints -- the previous selection's, or after a reset the episode's first."""
    scenes = synth.write_scenes(str(tmp_path), list(range(9)))
    a, b = _twins(monkeypatch, scenes, 64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **BENCH)
    assert (RC.as_np(a.shape_tensor())[:, 0] == 64).all()
    log = []

    def take_oracle_state(tag, fresh=False):
        if fresh:
            P.compare_fresh(a, orc)  # (leaves the oracle's state in a)
        else:
            P.inject_and_compare(a, orc)
        b.debug_set_state(orc.get_state())
        b.reset([])
        _same(a, b, tag + ", the oracle's state", log)

    _same(a, b, "start", log)
    take_oracle_state("start", fresh=True)
    rng = np.random.default_rng(61)
    for k in range(12):
        act = P.random_actions(rng, 9, 64, 0)
        for s in (a, b):
            RC.write_actions(s, act)
            s.step()
        _same(a, b, "step %d" % (k + 1), log)
        np.copyto(orc.action_tensor(), act)
        orc.step()
        P.compare_state(a, orc)
        take_oracle_state("step %d" % (k + 1))
        worlds = list(range(9)) if k == 4 else [7] if k == 8 else None
        if worlds is not None:
            for s in (a, b, orc):
                s.reset(worlds)
            P.compare_ints(a, orc)
            _same(a, b, "reset of %d worlds" % len(worlds), log)
            take_oracle_state("reset of %d worlds" % len(worlds))
    print(log)
    assert log[0][1] == 9 * 64 and log[0][2] == 9 * 64, "the first selection: every agent ranked, a row each: %s" % (log[0],)
    assert all(e[1] > 0 and e[2] == 0 for e in log[1:]), "rows written after the first selection: %s" % [e for e in log[1:] if e[2]]
    _close(a, b)


def test_seventeen_worlds_of_eight(tmp_path, monkeypatch):
    """17 worlds of 8 agents: partial waves in every call of the set-up, two dealt groups of worlds and a partial one (lists by index)."""
    scenes = [_scene(tmp_path, "w%d" % w, 8, 12 + w % 5, 129, 100 + w) for w in range(17)]
    a, b = _twins(monkeypatch, scenes, 64, **BENCH)
    assert (RC.as_np(a.shape_tensor())[:, 0] == 8).all()
    log = []
    _same(a, b, "start", log)
    _steps(a, b, 3, 63, log)
    for s in (a, b):
        s.reset([11])
    _same(a, b, "reset", log)
    print(log)
    assert log[0][1] == log[0][2] == 17 * 8
    _close(a, b)


def test_three_worlds_128_slots(tmp_path, monkeypatch):
    """Three worlds at 128 slots, 100, 64 and 70 agents: the workgroup of a world runs the set-up once per half of 64 -- a
    partial second half, none, a partial one."""
    scenes = [_scene(tmp_path, "wide%d" % w, n, 20, 129, 7 + w) for w, n in enumerate((100, 64, 70))]
    a, b = _twins(monkeypatch, scenes, 128, **BENCH)
    assert RC.as_np(a.shape_tensor())[:, 0].tolist() == [100, 64, 70]
    log = []
    _same(a, b, "start", log)
    _steps(a, b, 3, 64, log)
    for s in (a, b):
        s.reset([0])
    _same(a, b, "reset", log)
    print(log)
    assert log[0][1] == log[0][2] == 234
    assert all(e[1] + e[4] == 234 and e[3] == 0 for e in log), "every agent ranked or out of reach of every road: %s" % log
    _close(a, b)


def _scripted(monkeypatch, tmp_path, name, on_pass):
    """A case of tests/road_cases.py on the twins (reference order, rank path); on_pass(run, p, paths, log entry)."""
    case = RCS.CASES[name]
    _, knn_order, algo, _ = RCS.MODES["ref_order_rank"]
    paths = RCS.write_scenes(case, tmp_path)
    a, b = _twins(monkeypatch, paths[:len(case.worlds)], case.slots, knn_order=knn_order, **case.params(algo))
    run = RCS.Run(case, [a, b], "ref_order_rank")
    run.scene_paths = paths
    log = []

    def check(p):
        pa = _same(a, b, "%s, %s" % (name, run.passes[p]["tag"]), log)
        on_pass(run, p, pa, log[-1])

    RCS.script(run, check)
    print(log)
    _close(a, b)
    return log


def test_road_jump_donors_and_fresh_bounds(tmp_path, monkeypatch):
    """road_jump: agents that swap places, one that lands next to where another stood (a donor's checkpoints: a row copied
    by the state step) and one that jumps to where nobody was (bounded afresh by the state step's four waves)."""
    seen = []

    def on_pass(run, p, path, entry):
        if p == 0:
            return
        src = [RCS.bound_source(run, p, 0, ag) for ag in range(7)]
        want = sum(1 for ag in range(7) if path[0, ag] > 0 and src[ag] != "own")
        seen.append((p, src, entry[2]))
        assert entry[2] == want, "pass %d: %d rows, bounds %s, paths %s" % (p, entry[2], src, path[0, :7].tolist())

    _scripted(monkeypatch, tmp_path, "road_jump", on_pass)
    flat = [s for _, src, _ in seen for s in src]
    assert "borrowed" in flat and "fresh" in flat and "own" in flat, seen


def test_road_return_far_agents(tmp_path, monkeypatch):
    """road_return: agents that go to the padding position -- out of reach of every road: the state step writes their empty
    hand-over -- and come back with a reset."""
    far = []
    _scripted(monkeypatch, tmp_path, "road_return", lambda run, p, path, entry: far.append(entry[4]))
    assert max(far) > 0, "no agent was ever out of reach of every road: %s" % far


def test_set_maps_small_world_and_delete_agents(tmp_path, monkeypatch):
    """set_maps big -> small -> big with rk_min_roads pinned to 500: the small batch holds a world of 590 roads (ranked) and
    one of 236 (at least K, below rk_min_roads: the state step raises its fallback flag), then deleteAgents on one world."""
    big = [_scene(tmp_path, "big_a", 64, 16, 129, 41), _scene(tmp_path, "big_b", 40, 12, 129, 42)]  # 2048 and 1536 roads
    small = [_scene(tmp_path, "small_a", 9, 10, 60, 43), _scene(tmp_path, "small_b", 5, 4, 60, 44)]  # 590 and 236 roads
    a, b = _twins(monkeypatch, big, 64, min_roads=500, **BENCH)
    firsts, falls = [], []
    for k, new in enumerate((None, small, big)):
        if new is not None:
            for s in (a, b):
                s.set_maps(new)
            assert a.stat(STAT_FOLDED) == 1 and b.stat(STAT_FOLDED) == 0
        log = []
        _same(a, b, "batch %d, start" % k, log)
        _steps(a, b, 2, 66 + k, log, "batch %d, " % k)
        firsts.append(log[0])
        falls.append([e[3] for e in log])
    print(firsts, falls)
    assert all(ranked > 0 and rows == ranked for _, ranked, rows, _, _ in firsts), firsts
    assert falls[0] == [0, 0, 0] and falls[2] == [0, 0, 0] and falls[1] == [5, 5, 5], "agents selected by the fallback: %s" % falls
    ids = RC.as_np(a.self_observation_tensor())[..., 7]  # (the agents' ids: collectSelfObsSystem's last column)
    victims = {1: [int(ids[1, 0]), int(ids[1, 39]), int(ids[1, 17])]}
    for s in (a, b):
        s.deleteAgents(victims)
    assert int(RC.as_np(a.shape_tensor())[1, 0]) == 37
    log = []
    _same(a, b, "deleteAgents", log)
    _steps(a, b, 2, 69, log, "deleteAgents, ")
    assert log[0][1] == log[0][2] == 64 + 37, log[0]
    _close(a, b)


def test_gated_reset_passes_of_the_episode_tracker(tmp_path, monkeypatch):
    """`EpisodeTracker(auto_reset)` on two worlds through the end of an episode: every step launches the gated reset pass, whose
    state kernel (and with it the set-up) returns at once while no world has finished and runs for every world in the step
    in which one has; the reset agents go back to the checkpoints of the episode's first selection."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    kw = dict(BENCH, collisionBehaviour=0, maxNumControlledAgents=4, isStaticAgentControlled=0)
    scenes = [_scene(tmp_path, "ep_a", 8, 12, 129, 71), _scene(tmp_path, "ep_b", 5, 12, 129, 72)]
    a, b = _twins(monkeypatch, scenes, 64, **kw)
    ta, tb = (EpisodeTracker(s, collision_weight=-0.75, goal_achieved_weight=1.0, off_road_weight=-0.5) for s in (a, b))
    rng = np.random.default_rng(73)
    finished, quiet, log = 0, 0, []
    for k in range(94):
        act = P.random_actions(rng, 2, 64, 0)
        outs = []
        for s, t in ((a, ta), (b, tb)):
            RC.write_actions(s, act)
            outs.append([x.cpu().numpy() for x in t.step()] + [t.done_worlds.cpu().numpy()])
        for x, y in zip(*outs):
            assert np.array_equal(x, y, equal_nan=True), "step %d: the trackers differ" % (k + 1)
        done = outs[0][-1]
        finished += int(done.any())
        quiet += int(not done.any())
        _same(a, b, "tracked step %d" % (k + 1), log, names=NAMED)
    assert finished > 0 and quiet > 0, "gated passes that ran / returned at once: %d / %d" % (finished, quiet)
    assert all(e[1] > 0 for e in log), "steps without a ranked agent: %s" % [e for e in log if e[1] == 0]
    _close(a, b)
