"""GPU suite: k_knn_replay with the push chain in registers (csrc/rank_heap.hpp: slots 12, 25, 50, 100 are mirrored in `q`
across the rounds, and where the pop's path went is told by the choices made on the way down, not by comparing slot numbers).
Nothing of that may show in a result.  Every case runs the simulator in lockstep with the oracle and beside a twin created
under GPUDRIVE_NO_RANK_REPLAY=1, whose road selection never enters k_knn_replay (k_map_obs replays the insert history on keys),
on the same scenes, actions and states, and requires after every pass: every exported tensor of the twins bit-equal and the
device-side bounds audit of the rank path (gd_stat 21) at zero; the simulator under test against the oracle as everywhere in
the suite (ints exact, state and observations within the suite's tolerances under teacher forcing).  The cases: the bench's
worlds; worlds with duplicated polylines, whose exactly equal keys put waves on the equal-key and the checked form of the
round; an unreduced Waymo tile with agents on the long list (4-bit tie field, tiles of 64 candidates); 128 agent slots; and a
batch whose only ranked agent sits in the last slot of the last world (a replay wave of one heap and 63 idle lanes).
tests/test_replay_chain_model.py holds the rounds on the host, checked after every round."""
import json

import numpy as np
import pytest

from gpudrive_lab_amd import synth
from tests import parity as P
from tests import ref_cases as RC
from tests.conftest import SCENE_407
from tests.test_gpu_rank_candidates import BENCH
from tests.test_gpu_rank_deal import EXPORTED

pytestmark = pytest.mark.gpu

STAT_AUDIT = 21


def _twins(monkeypatch, scenes, slots, **kw):
    """(the simulator under test: the rank replay; its twin without it)"""
    monkeypatch.setenv("GPUDRIVE_RANK_MIN_ROADS", "200")    # every world with K roads goes to the rank path
    monkeypatch.setenv("GPUDRIVE_RANK_MAX_ROADS", "20000")  # the largest too
    monkeypatch.delenv("GPUDRIVE_NO_RANK_REPLAY", raising=False)
    a = P.make_gpu_sim(scenes, max_agents=slots, **kw)
    monkeypatch.setenv("GPUDRIVE_NO_RANK_REPLAY", "1")  # read once, when the engine is created
    b = P.make_gpu_sim(scenes, max_agents=slots, **kw)
    monkeypatch.delenv("GPUDRIVE_NO_RANK_REPLAY")
    assert a.stat(7) == 1 and b.stat(7) == 0, "which twin runs the rank replay"
    return a, b


def _same(a, b, tag, paths):
    for name in EXPORTED:
        x, y = RC.as_np(getattr(a, name)()), RC.as_np(getattr(b, name)())
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, name)
        same = np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)
        assert same.all(), "%s: %s differs between the twins in %d bytes, first at byte %d" % (tag, name, int((~same).sum()), int(np.argmin(same)))
    assert a.stat(STAT_AUDIT) == 0, "%s: bounds audit of the rank path: %d" % (tag, a.stat(STAT_AUDIT))
    assert (b.debug_road_path() == -2).all(), "%s: the twin took the rank path" % tag
    paths.append(a.debug_road_path().copy())


def _lockstep(a, b, orc, steps, seed, reset_worlds=None):
    """The passes of a case: the first selection, the oracle's state, `steps` steps with seeded actions -- each followed by a
    reset pass that recomputes every observation from the oracle's state -- and a reset of `reset_worlds`.  Returns the road
    path of the simulator under test after every pass."""
    paths = []

    def take_oracle_state(tag, fresh=False):
        if fresh:
            P.compare_fresh(a, orc)  # (leaves the oracle's state in a)
        else:
            P.inject_and_compare(a, orc)
        b.debug_set_state(orc.get_state())
        b.reset([])
        _same(a, b, tag + ", the oracle's state", paths)

    _same(a, b, "start", paths)
    take_oracle_state("start", fresh=True)
    rng = np.random.default_rng(seed)
    for k in range(steps):
        act = P.random_actions(rng, orc.W, orc.A, 0)
        for s in (a, b):
            RC.write_actions(s, act)
            s.step()
        _same(a, b, "step %d" % (k + 1), paths)
        np.copyto(orc.action_tensor(), act)
        orc.step()
        P.compare_ints(a, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
        P.compare_state(a, orc)
        take_oracle_state("step %d" % (k + 1))
    if reset_worlds is not None:
        for s in (a, b, orc):
            s.reset(reset_worlds)
        P.compare_ints(a, orc)
        _same(a, b, "reset", paths)
        take_oracle_state("reset")
    return paths


def _live(sim):
    W, A = sim.debug_road_path().shape
    return np.arange(A)[None, :] < RC.as_np(sim.shape_tensor())[:, 0:1]


def _all_ranked(sim, paths):
    """every live agent ranked (path: its candidate count) or parked out of reach of every road (-3), in every pass"""
    live = _live(sim)
    for p in paths:
        assert ((p[live] > 0) | (p[live] == -3)).all(), sorted(set(p[live][p[live] <= 0].tolist()))
        assert (p[live] > 0).any()


def _scene(tmp_path, name, sc):
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps(sc))
    return str(p)


def test_nine_bench_worlds(oracle_mod, tmp_path, monkeypatch):
    """Nine of the bench's worlds x 64 agents (nine replay waves, no equal keys: the plain form throughout), six steps and a
    reset of the whole batch."""
    scenes = synth.write_scenes(str(tmp_path), list(range(9)))
    a, b = _twins(monkeypatch, scenes, 64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **BENCH)
    paths = _lockstep(a, b, orc, 6, 81, reset_worlds=list(range(9)))
    assert (paths[0][:, :64] > 0).all()
    _all_ranked(a, paths)
    a.close()
    b.close()


def _dup_scene(tmp_path, name, seed, n_agents, n_polylines, pts, twice):
    """The first `twice` polylines twice: exactly equal keys among the candidates (as tests/test_gpu_round3.py's _dup_scene)."""
    sc = synth.make_scene(seed, n_agents=n_agents, n_polylines=n_polylines, pts_per_polyline=pts)
    sc["roads"] = sc["roads"] + [dict(r, id=100 + i) for i, r in enumerate(sc["roads"][:twice])]
    return _scene(tmp_path, name, sc)


def test_duplicated_polylines(oracle_mod, tmp_path, monkeypatch):
    """Worlds with duplicated polylines at a radius that makes nearly every road a candidate: groups of two equal keys arrive
    all along the replay (the equal-key form where a block holds a second member, the checked form while one sits in a heap,
    the plain form between), next to the unreduced Waymo tile as in tests/test_gpu_round3.py; four steps and a reset."""
    kw = dict(BENCH, observationRadius=200.0)
    scenes = [_dup_scene(tmp_path, "dup", 5, 12, 10, 60, 3), _dup_scene(tmp_path, "dup_b", 6, 20, 14, 60, 5), SCENE_407]
    a, b = _twins(monkeypatch, scenes, 64, **kw)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **kw)
    paths = _lockstep(a, b, orc, 4, 82, reset_worlds=[0, 1, 2])
    live = _live(a)
    for p in paths:  # the duplicated-polyline worlds are ranked with their equal keys (the tile's agents may overflow to the fallback)
        assert ((p[:2][live[:2]] > 0) | (p[:2][live[:2]] == -3)).all(), p[:2][live[:2]].tolist()
        assert (p[:2][live[:2]] > 200).any(), "no agent of the duplicated-polyline worlds had a round to run"
    a.close()
    b.close()


def test_unreduced_waymo_tile_long_list(oracle_mod, monkeypatch):
    """One Waymo tile with every point of its polylines kept: agents with more candidates than the standard ranking holds go
    to the long list, whose ranks have a 4-bit tie field and checkpoints every 64 candidates; repeated points give equal keys."""
    a, b = _twins(monkeypatch, [SCENE_407], 64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, [SCENE_407], max_agents=64, **BENCH)
    paths = _lockstep(a, b, orc, 3, 83, reset_worlds=[0])
    _all_ranked(a, paths)
    assert max(int(p.max()) for p in paths) > 1272, "no agent of the tile went to the long list"
    a.close()
    b.close()


def test_three_worlds_128_slots(oracle_mod, tmp_path, monkeypatch):
    """Three worlds at 128 slots with 100, 64 and 70 agents: 234 heaps in four replay waves, the last one partial."""
    scenes = [_scene(tmp_path, "wide%d" % w, synth.make_scene(7 + w, n_agents=n, n_polylines=20, pts_per_polyline=129))
              for w, n in enumerate((100, 64, 70))]
    a, b = _twins(monkeypatch, scenes, 128, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=128, **BENCH)
    assert RC.as_np(a.shape_tensor())[:, 0].tolist() == [100, 64, 70]
    paths = _lockstep(a, b, orc, 3, 84, reset_worlds=[1])
    _all_ranked(a, paths)
    a.close()
    b.close()


def test_only_the_last_slot_of_the_last_world_is_ranked(oracle_mod, tmp_path, monkeypatch):
    """Two worlds of 64 agents whose logged trajectories lie 3 km from every road, except the last agent of the last world:
    127 agents are out of reach of every road (no selection), and the replay is one wave of one heap beside 63 idle lanes."""
    scenes = []
    for w in range(2):
        sc = synth.make_scene(90 + w, n_agents=64, n_polylines=16, pts_per_polyline=129)
        for o in sc["objects"][:64 if w == 0 else 63]:
            o["position"] = [dict(p, x=p["x"] + 3000.0) for p in o["position"]]
            o["goalPosition"] = dict(o["goalPosition"], x=o["goalPosition"]["x"] + 3000.0)
        scenes.append(_scene(tmp_path, "far%d" % w, sc))
    a, b = _twins(monkeypatch, scenes, 64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **BENCH)
    paths = _lockstep(a, b, orc, 4, 85, reset_worlds=[0, 1])
    want = np.full((2, 64), -3)
    for p in paths:
        assert p[1, 63] > 200, "the last agent has no round to run: %d candidates" % p[1, 63]
        want[1, 63] = p[1, 63]
        assert np.array_equal(p[:, :64], want), "ranked agents: %s" % np.argwhere(p[:, :64] > 0).tolist()
    a.close()
    b.close()
