"""GPU suite: how k_knn_rank deals agents to its waves (csrc/map_obs_rank.hip: a wave draws its next agent from the cursor of
its XCD's list; short lists and the long list go by index).  Which wave ranks which agent depends on timing and must never show in
a result, so every case runs twin simulators on the same scenes and the same seeded actions -- one on the default grid, one
with GPUDRIVE_RANK_WAVES set to a few waves that take many turns each -- and requires, after every step and every reset
pass: all exported tensors of the two bit-equal, the same candidate count per agent, every live agent in reach of a road
ranked (debug_road_path() > 0) in both, and the device-side bounds audit (gd_stat 21) at zero.  Nothing here looks at which
wave took which agent.  GPUDRIVE_RANK_MIN_ROADS=200 puts every world with K roads on the rank path."""
import json

import numpy as np
import pytest

from gpudrive_lab_amd import synth
from gpudrive_lab_amd.madrona_gpudrive_impl import _SLOT_GETTERS
from tests import parity as P
from tests import ref_cases as RC
from tests.conftest import SCENE_407
from tests.test_gpu_rank_candidates import BENCH

pytestmark = pytest.mark.gpu

EXPORTED = sorted(_SLOT_GETTERS)


def _twins(monkeypatch, scenes, slots, waves, **kw):
    """(simulator on the default grid, simulator whose standard ranking launch has `waves` workgroups)"""
    monkeypatch.setenv("GPUDRIVE_RANK_MIN_ROADS", "200")
    monkeypatch.delenv("GPUDRIVE_RANK_WAVES", raising=False)
    a = P.make_gpu_sim(scenes, max_agents=slots, **dict(BENCH, **kw))
    monkeypatch.setenv("GPUDRIVE_RANK_WAVES", str(waves))  # read once, when the engine is created
    b = P.make_gpu_sim(scenes, max_agents=slots, **dict(BENCH, **kw))
    monkeypatch.delenv("GPUDRIVE_RANK_WAVES")
    assert a.stat(7) == 1 and b.stat(7) == 1, "the rank path is off"
    return a, b


def _check(a, b, tag):
    """After a selection: the twins bit-equal in every exported tensor, every live agent in reach of roads ranked."""
    for name in EXPORTED:
        x, y = RC.as_np(getattr(a, name)()), RC.as_np(getattr(b, name)())
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, name)
        same = np.ascontiguousarray(x).view(np.uint8) == np.ascontiguousarray(y).view(np.uint8)
        assert same.all(), "%s: %s differs between the twins in %d bytes, first at byte %d" % (tag, name, int((~same).sum()), int(np.argmin(same)))
    pa, pb = a.debug_road_path(), b.debug_road_path()
    assert np.array_equal(pa, pb), "%s: the twins' road paths differ at %s" % (tag, np.argwhere(pa != pb)[:4].tolist())
    live = np.arange(pa.shape[1])[None, :] < RC.as_np(a.shape_tensor())[:, 0:1]
    reach = live & (pa != -3)  # (-3: parked at the padding position, out of reach of every road: no selection)
    assert reach.any(), "%s: nobody to rank" % tag
    assert (pa[reach] > 0).all(), "%s: live agents off the rank path: %s" % (tag, sorted(set(pa[reach][pa[reach] <= 0].tolist())))
    assert a.stat(21) == 0 and b.stat(21) == 0, "%s: bounds audit of the rank path: %d / %d" % (tag, a.stat(21), b.stat(21))
    return pa


def _drive(a, b, steps, seed, reset_world=None, orc=None):
    """The twins (and the oracle, if given: rows within the suite's tolerances, as tests/test_gpu_rank_candidates.py does it)
    on the same seeded actions; returns the road paths of every selection."""
    paths = [_check(a, b, "start")]
    if orc is not None:
        P.compare_fresh(a, orc)  # (leaves the oracle's state in a; b takes it too)
        b.debug_set_state(orc.get_state())
        b.reset([])
        paths.append(_check(a, b, "start, the oracle's state"))
    rng = np.random.default_rng(seed)
    W, A = paths[0].shape
    for k in range(steps):
        act = P.random_actions(rng, W, A, 0)
        for s in (a, b):
            RC.write_actions(s, act)
            s.step()
        paths.append(_check(a, b, "step %d" % (k + 1)))
        if orc is not None:
            np.copyto(orc.action_tensor(), act)
            orc.step()
            P.compare_state(a, orc)
            # both twins recompute their observations from the oracle's state: one more selection each
            b.debug_set_state(orc.get_state())
            b.reset([])
            P.inject_and_compare(a, orc)
            paths.append(_check(a, b, "step %d, the oracle's state" % (k + 1)))
    if reset_world is not None:
        for s in (a, b):
            s.reset([reset_world])
        if orc is not None:
            orc.reset([reset_world])
            P.compare_ints(a, orc)
            b.debug_set_state(orc.get_state())
            b.reset([])
            P.inject_and_compare(a, orc)
        paths.append(_check(a, b, "reset"))
    return paths


def _close(*sims):
    for s in sims:
        s.close()


def test_nine_worlds_eight_waves(oracle_mod, tmp_path, monkeypatch):
    """(a) 9 of the bench's worlds x 64 agents, 8 waves: one XCD's list holds two worlds, the others one, and each wave takes
    64 or 128 turns.  Six steps and a reset of one world, the default-grid twin in lockstep with the oracle."""
    scenes = synth.write_scenes(str(tmp_path), list(range(9)))
    a, b = _twins(monkeypatch, scenes, 64, 8)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **BENCH)
    assert (RC.as_np(a.shape_tensor())[:, 0] == 64).all()
    _drive(a, b, 6, 31, reset_world=8, orc=orc)
    _close(a, b)


def test_one_world_sixteen_waves(tmp_path, monkeypatch):
    """(b) one world, 16 waves: seven lists are empty and two waves share the eighth."""
    scenes = synth.write_scenes(str(tmp_path), [2])
    a, b = _twins(monkeypatch, scenes, 64, 16)
    _drive(a, b, 4, 32, reset_world=0)
    _close(a, b)


def test_a_turn_per_wave_at_most(tmp_path, monkeypatch):
    """One world, 1024 waves: the list has fewer entries than its XCD has waves, which index alone shares out (no cursor);
    the default-grid twin (64 waves, 8 per list) draws."""
    scenes = synth.write_scenes(str(tmp_path), [6])
    a, b = _twins(monkeypatch, scenes, 64, 1024)
    _drive(a, b, 3, 38, reset_world=0)
    _close(a, b)


def test_more_waves_than_entries(tmp_path, monkeypatch):
    """(c) three worlds on the default grid (a wave per live agent, an eighth of them per XCD): five lists are empty, so most
    waves draw past the end at once; the twin has 8 waves."""
    scenes = synth.write_scenes(str(tmp_path), [3, 4, 5])
    a, b = _twins(monkeypatch, scenes, 64, 8)
    _drive(a, b, 4, 33, reset_world=1)
    _close(a, b)


def test_128_slots_eight_waves(tmp_path, monkeypatch):
    """(d) one world with more than 64 live agents at 128 slots (k_knn_scan's two workgroups fill two lists), 8 waves."""
    p = tmp_path / "wide.json"
    p.write_text(json.dumps(synth.make_scene(7, n_agents=100, n_polylines=20, pts_per_polyline=129)))
    a, b = _twins(monkeypatch, [str(p)], 128, 8)
    assert int(RC.as_np(a.shape_tensor())[0, 0]) == 100
    _drive(a, b, 3, 34, reset_world=0)
    _close(a, b)


def test_long_list_small_grid(monkeypatch):
    """(e) an unreduced Waymo tile (thousands of roads): agents with more candidates than the standard ranking holds go to
    the long-list launch, which the waves of the standard one feed while they draw; 8 waves in the standard launch."""
    a, b = _twins(monkeypatch, [SCENE_407], 64, 8)
    paths = _drive(a, b, 3, 35, reset_world=0)
    assert max(int(p.max()) for p in paths) > 1272, "no agent of the tile went to the long list"
    _close(a, b)


def test_cursors_start_at_zero_after_rebuilds(tmp_path, monkeypatch):
    """(f) set_maps big -> small -> big on both twins, 8 waves: a list drawn from a cursor that a rebuild left where the last
    selection ended would leave its first agents unranked."""
    def scene(name, n_agents, n_poly, pts, seed):
        p = tmp_path / (name + ".json")
        p.write_text(json.dumps(synth.make_scene(seed, n_agents=n_agents, n_polylines=n_poly, pts_per_polyline=pts)))
        return str(p)
    big = [scene("big_a", 64, 16, 129, 41), scene("big_b", 40, 12, 129, 42)]  # 2048 and 1536 roads
    small = [scene("small_a", 9, 10, 60, 43), scene("small_b", 5, 4, 60, 44)]  # 590 and 236 roads
    a, b = _twins(monkeypatch, big, 64, 8)
    _drive(a, b, 2, 36)
    for k, new in enumerate((small, big)):
        for s in (a, b):
            s.set_maps(new)
        _drive(a, b, 2, 37 + k)
    _close(a, b)
