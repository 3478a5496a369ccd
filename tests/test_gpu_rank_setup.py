"""GPU suite: the set-up around k_knn_rank (csrc/map_obs_rank.hip k_knn_scan -> k_knn_rank).  An agent that is bounded by its own
checkpoints gets no row from k_knn_scan: its ranking wave reads the checkpoints where they are and makes the row itself
(csrc/rank_cand.hpp cp_threshold); only a donor's checkpoints and those made afresh are handed over as rows.  And k_knn_scan's
workgroups append to the XCD list that rank_cand.hpp deal_list gives their world, so that every list gets the same mix of worlds.  Neither may ever
show in a result, so every case runs twin simulators on the same scenes and the same seeded actions -- one as it is by default,
one with GPUDRIVE_RANK_SCAN_ROWS=1 (every row written by k_knn_scan, world b on list b % 8, as before) -- and requires after
every pass: all exported tensors of the two bit-equal, the same candidate count per agent (debug_road_path()), every live agent
in reach of a road ranked, and the device-side bounds audit (gd_stat 21) at zero.  gd_stat 22 counts the rows k_knn_scan wrote
for the ranked agents of the last selection: every one's in the twin, and by default exactly those of the agents without a usable bound of
their own.  tests/test_rank_setup_model.py holds the row's arithmetic and the deal on the host."""
import json

import numpy as np
import pytest

from gpudrive_lab_amd import synth
from tests import parity as P
from tests import ref_cases as RC
from tests import road_cases as RCS
from tests.test_gpu_rank_candidates import BENCH
from tests.test_gpu_rank_deal import _check, _close

pytestmark = pytest.mark.gpu

STAT_ROWS = 22


def _twins(monkeypatch, scenes, slots, **kw):
    """(the default simulator, the one whose k_knn_scan writes every row and deals worlds by index)"""
    monkeypatch.setenv("GPUDRIVE_RANK_MIN_ROADS", "200")
    monkeypatch.delenv("GPUDRIVE_RANK_SCAN_ROWS", raising=False)
    a = P.make_gpu_sim(scenes, max_agents=slots, **kw)
    monkeypatch.setenv("GPUDRIVE_RANK_SCAN_ROWS", "1")  # read once, when the engine is created
    b = P.make_gpu_sim(scenes, max_agents=slots, **kw)
    monkeypatch.delenv("GPUDRIVE_RANK_SCAN_ROWS")
    assert a.stat(7) == 1 and b.stat(7) == 1, "the rank path is off"
    return a, b


def _pass(a, b, tag, log):
    """_check of tests/test_gpu_rank_deal.py, and the row counts of the selection: (ranked agents, rows of a, rows of b)."""
    pa = _check(a, b, tag)
    live = np.arange(pa.shape[1])[None, :] < RC.as_np(a.shape_tensor())[:, 0:1]  # (dead slots keep the entry of an earlier batch)
    ranked = int(((pa > 0) & live).sum())
    log.append((tag, ranked, a.stat(STAT_ROWS), b.stat(STAT_ROWS)))
    assert log[-1][3] == ranked, "%s: the twin that writes every row wrote %d for %d ranked agents" % (tag, log[-1][3], ranked)
    assert 0 <= log[-1][2] <= ranked, "%s: %d rows for %d ranked agents" % (tag, log[-1][2], ranked)
    return pa


def _drive(a, b, steps, seed, log, reset_world=None, orc=None):
    """The twins (and the oracle, if given: rows within the suite's tolerances) on the same seeded actions."""
    _pass(a, b, "start", log)
    if orc is not None:
        P.compare_fresh(a, orc)  # (leaves the oracle's state in a; b takes it too)
        b.debug_set_state(orc.get_state())
        b.reset([])
        _pass(a, b, "start, the oracle's state", log)
    rng = np.random.default_rng(seed)
    W, A = a.debug_road_path().shape
    for k in range(steps):
        act = P.random_actions(rng, W, A, 0)
        for s in (a, b):
            RC.write_actions(s, act)
            s.step()
        _pass(a, b, "step %d" % (k + 1), log)
        if orc is not None:
            np.copyto(orc.action_tensor(), act)
            orc.step()
            P.compare_state(a, orc)
            b.debug_set_state(orc.get_state())
            b.reset([])
            P.inject_and_compare(a, orc)
            _pass(a, b, "step %d, the oracle's state" % (k + 1), log)
    if reset_world is not None:
        for s in (a, b):
            s.reset([reset_world])
        if orc is not None:
            orc.reset([reset_world])
            P.compare_ints(a, orc)
            b.debug_set_state(orc.get_state())
            b.reset([])
            P.inject_and_compare(a, orc)
        _pass(a, b, "reset", log)


def test_nine_bench_worlds(oracle_mod, tmp_path, monkeypatch):
    """9 of the bench's worlds x 64 agents: one whole group of 8 workgroups (dealt) and a partial one (by index).  Six steps,
    a reset of one world, two more steps, the default twin in lockstep with the oracle.  The first selection bounds every agent
    afresh (a row each); from then on every agent is within reach of its previous or its episode's first selection: no rows."""
    scenes = synth.write_scenes(str(tmp_path), list(range(9)))
    a, b = _twins(monkeypatch, scenes, 64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **BENCH)
    assert (RC.as_np(a.shape_tensor())[:, 0] == 64).all()
    log = []
    _drive(a, b, 6, 51, log, reset_world=8, orc=orc)
    _drive(a, b, 2, 52, log)
    print(log)
    assert log[0][1] == 9 * 64 and log[0][2] == log[0][1], "the first selection: a row per ranked agent: %s" % (log[0],)
    assert all(rows == 0 for _, _, rows, _ in log[1:]), "rows written after the first selection: %s" % [e for e in log[1:] if e[2]]
    _close(a, b)


def test_seventeen_worlds_of_eight(tmp_path, monkeypatch):
    """17 worlds of 8 agents: two dealt groups and a partial one, lists of a few agents per XCD."""
    scenes = []
    for w in range(17):
        p = tmp_path / ("w%d.json" % w)
        p.write_text(json.dumps(synth.make_scene(100 + w, n_agents=8, n_polylines=12 + w % 5, pts_per_polyline=129)))
        scenes.append(str(p))
    a, b = _twins(monkeypatch, scenes, 64, **BENCH)
    assert (RC.as_np(a.shape_tensor())[:, 0] == 8).all()
    log = []
    _drive(a, b, 3, 53, log, reset_world=11)
    print(log)
    assert log[0][2] == log[0][1] == 17 * 8
    _close(a, b)


def test_three_worlds_128_slots(tmp_path, monkeypatch):
    """Three worlds at 128 slots, 100, 64 and 70 agents: a world's two halves are separate workgroups (six in all: one partial group)."""
    scenes = []
    for w, n in enumerate((100, 64, 70)):
        p = tmp_path / ("wide%d.json" % w)
        p.write_text(json.dumps(synth.make_scene(7 + w, n_agents=n, n_polylines=20, pts_per_polyline=129)))
        scenes.append(str(p))
    a, b = _twins(monkeypatch, scenes, 128, **BENCH)
    assert RC.as_np(a.shape_tensor())[:, 0].tolist() == [100, 64, 70]
    log = []
    _drive(a, b, 3, 54, log, reset_world=0)
    print(log)
    assert log[0][2] == log[0][1] == 234
    _close(a, b)


def _scripted(monkeypatch, tmp_path, name, on_pass):
    """A case of tests/road_cases.py on the twins (reference order, rank path); on_pass(run, p, path, rows of a)."""
    case = RCS.CASES[name]
    _, knn_order, algo, _ = RCS.MODES["ref_order_rank"]
    paths = RCS.write_scenes(case, tmp_path)
    a, b = _twins(monkeypatch, paths[:len(case.worlds)], case.slots, knn_order=knn_order, **case.params(algo))
    run = RCS.Run(case, [a, b], "ref_order_rank")
    run.scene_paths = paths
    log = []

    def check(p):
        pa = _pass(a, b, "%s, %s" % (name, run.passes[p]["tag"]), log)
        on_pass(run, p, pa, log[-1][2])

    RCS.script(run, check)
    print(log)
    _close(a, b)
    return run, log


def test_road_jump_rows_are_the_jumped_agents(tmp_path, monkeypatch):
    """road_jump: agents that swap places, one that lands next to where another stood (a donor's checkpoints) and one that jumps
    to where nobody was (bounded afresh).  The rows k_knn_scan writes are exactly those of the ranked agents whose bound is not
    their own."""
    seen = []

    def on_pass(run, p, path, rows):
        if p == 0:
            return
        src = [RCS.bound_source(run, p, 0, ag) for ag in range(7)]
        want = sum(1 for ag in range(7) if path[0, ag] > 0 and src[ag] != "own")
        seen.append((p, src, rows))
        assert rows == want, "pass %d: %d rows, bounds %s, paths %s" % (p, rows, src, path[0, :7].tolist())

    _scripted(monkeypatch, tmp_path, "road_jump", on_pass)
    flat = [s for _, src, _ in seen for s in src]
    assert "borrowed" in flat and "fresh" in flat and "own" in flat, seen
    assert sum(rows for _, _, rows in seen) > 0


def test_agents_at_the_padding_position(tmp_path, monkeypatch):
    """road_return: agents that go to the padding position (out of reach of every road: no selection, no row) and come back
    with a reset."""
    far = []

    def on_pass(run, p, path, rows):
        far.append(int((path[:, :6] == -3).sum()))

    _scripted(monkeypatch, tmp_path, "road_return", on_pass)
    assert max(far) > 0, "no agent was ever out of reach of every road: %s" % far


def test_set_maps_big_small_big(tmp_path, monkeypatch):
    """set_maps big -> small -> big on both twins: the records and rows of a rebuilt batch start afresh (a row per ranked agent
    in the first selection after every rebuild)."""
    def scene(name, n_agents, n_poly, pts, seed):
        p = tmp_path / (name + ".json")
        p.write_text(json.dumps(synth.make_scene(seed, n_agents=n_agents, n_polylines=n_poly, pts_per_polyline=pts)))
        return str(p)
    big = [scene("big_a", 64, 16, 129, 41), scene("big_b", 40, 12, 129, 42)]  # 2048 and 1536 roads
    small = [scene("small_a", 9, 10, 60, 43), scene("small_b", 5, 4, 60, 44)]  # 590 and 236 roads
    a, b = _twins(monkeypatch, big, 64, **BENCH)
    firsts = []
    log = []
    _drive(a, b, 2, 56, log)
    firsts.append(log[0])
    for k, new in enumerate((small, big)):
        for s in (a, b):
            s.set_maps(new)
        log = []
        _drive(a, b, 2, 57 + k, log)
        firsts.append(log[0])
    print(firsts)
    assert all(ranked > 0 and rows == ranked for _, ranked, rows, _ in firsts), firsts
    _close(a, b)
