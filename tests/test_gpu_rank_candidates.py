"""GPU suite: the candidates of the rank path (csrc/map_obs_rank.hip k_knn_rank: the block cull and the ordered scan of
csrc/rank_cand.hpp, from the checkpoint rows that k_knn_scan leaves) against the oracle -- on the bench's synthetic worlds,
on an unreduced Waymo tile with thousands of roads (several batches of the cull, long candidate lists) and with 128 agent
slots (two halves of k_knn_scan per world).  After every selection: the rows within the suite's tolerances, every live agent
on the rank path, and the candidate set a superset of what the reference inserts into its heap (src/knn.hpp:128-151) -- per
agent against the inserts counted on the oracle's own rows, in total against the oracle's insert counter -- and the
device-side bounds audit at zero.  tests/test_rank_cand_model.py holds the same logic against a plain loop on the host."""
import heapq

import numpy as np
import pytest

from gpudrive_lab_amd import synth
from tests import parity as P
from tests import ref_cases as RC
from tests.conftest import SCENE_407

pytestmark = pytest.mark.gpu

K = 200
ALL_OBJECTS = dict(isStaticAgentControlled=1, initOnlyValidAgentsAtFirstStep=0, IgnoreNonVehicles=0)
BENCH = dict(observationRadius=50.0, collisionBehaviour=2, rewardType=1, distanceToGoalThreshold=2.0, dynamicsModel=0,
             roadObservationAlgorithm=0, polylineReductionThreshold=0.0, **ALL_OBJECTS)


def _inserts(orc, w, a):
    """Heap inserts of the reference's selection for one agent, counted on the oracle's rows of every road in that agent's
    frame (columns 0, 1: the road's position): roads K.. that are closer than the K-th nearest road so far."""
    rows = orc.road_obs_of(w, a).astype(np.float64)
    key = rows[:, 0] ** 2 + rows[:, 1] ** 2
    heap = [-k for k in key[:K]]
    heapq.heapify(heap)
    n = 0
    for k in key[K:]:
        if k < -heap[0]:
            heapq.heapreplace(heap, -k)
            n += 1
    return n


def _check_selection(gpu, orc, tag):
    """Both simulators recompute their observations from the oracle's state (one selection each): rows, paths, candidates."""
    before = orc.knn_inserts()
    P.inject_and_compare(gpu, orc)
    total = orc.knn_inserts() - before
    path = gpu.debug_road_path()
    live = P._live_mask(orc)
    # an agent that finished is parked at the padding position, out of reach of every road (-3): no selection, no candidates;
    # the oracle still runs its loop for it, to K padding rows
    rows = np.asarray(orc.agent_roadmap_tensor())
    for w, a in np.argwhere(live & (path == -3)):
        assert (rows[w, a, :, 6] == 0).all(), "%s: world %d agent %d is marked out of reach of every road but has rows" % (tag, w, a)
        total -= _inserts(orc, int(w), int(a))
    live = live & (path != -3)
    print("%s: candidates min %d mean %.1f max %d over %d live agents, %d not ranked; the oracle inserted %d" %
          (tag, path[live].min(), path[live].mean(), path[live].max(), int(live.sum()), int((path[live] <= 0).sum()), total))
    assert (path[live] > 0).all(), "%s: live agents off the rank path: %s" % (tag, sorted(set(path[live][path[live] <= 0].tolist())))
    assert int((path[live] - K).sum()) >= total, "%s: %d candidates beyond the first K for %d inserts" % (tag, int((path[live] - K).sum()), total)
    for w, a in np.argwhere(live):  # every agent with a selection, at every selection
        ins = _inserts(orc, int(w), int(a))
        assert path[w, a] - K >= ins, "%s: world %d agent %d has %d candidates beyond the first K for %d inserts" % (tag, w, a, path[w, a] - K, ins)
    assert gpu.stat(21) == 0, "%s: device-side bounds audit of the rank path: %d indices out of range" % (tag, gpu.stat(21))
    return path


def _run(gpu, orc, steps, seed, reset_world):
    assert gpu.stat(7) == 1, "the rank path is off"
    P.compare_fresh(gpu, orc)
    rng = np.random.default_rng(seed)
    paths = []
    for k in range(steps):
        act = P.random_actions(rng, orc.W, orc.A, 0)
        RC.write_actions(gpu, act)
        np.copyto(orc.action_tensor(), act)
        gpu.step()
        orc.step()
        P.compare_ints(gpu, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
        P.compare_state(gpu, orc)
        paths.append(_check_selection(gpu, orc, "step %d" % (k + 1)))
    if reset_world is not None:
        gpu.reset([reset_world])
        orc.reset([reset_world])
        P.compare_ints(gpu, orc)
        paths.append(_check_selection(gpu, orc, "reset"))
    return paths


def test_bench_worlds(oracle_mod, tmp_path):
    """Two of bench.py's synthetic worlds (4096 roads: four batches of the cull), 64 agents each: the reset pass, six steps
    with random actions in lockstep with the oracle, then a reset of one world."""
    scenes = synth.write_scenes(str(tmp_path), [0, 1])
    gpu = P.make_gpu_sim(scenes, max_agents=64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=64, **BENCH)
    paths = _run(gpu, orc, 6, 3, 1)
    assert all((p[:, :64] < 1272).all() for p in paths), "the bench worlds' candidates fit the standard ranking"
    gpu.close()


def test_unreduced_waymo_tile(oracle_mod):
    """One Waymo tile with every point of its polylines kept (polylineReductionThreshold = 0: thousands of roads, repeated
    points; BENCH sets polylineReductionThreshold = 0), 64 slots, three steps: several batches of the cull per agent, and agents
    with more candidates than the standard ranking holds (the long list)."""
    gpu = P.make_gpu_sim([SCENE_407], max_agents=64, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, [SCENE_407], max_agents=64, **BENCH)
    roads = int(RC.as_np(gpu.shape_tensor())[0, 1])
    print("roads: %d" % roads)
    assert roads > 2 * 1024, "the tile should take several batches of 64 blocks"
    paths = _run(gpu, orc, 3, 5, None)
    assert max(int(p.max()) for p in paths) > 1272, "no agent of the tile went to the long list"
    gpu.close()


def test_128_slots(oracle_mod, tmp_path):
    """One world with more than 64 agents at 128 slots (the kernels' 128-slot instantiations, two workgroups of k_knn_scan
    per world), two steps."""
    p = tmp_path / "wide.json"
    import json
    p.write_text(json.dumps(synth.make_scene(7, n_agents=100, n_polylines=20, pts_per_polyline=129)))
    gpu = P.make_gpu_sim([str(p)], max_agents=128, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, [str(p)], max_agents=128, **BENCH)
    assert int(RC.as_np(gpu.shape_tensor())[0, 0]) == 100
    _run(gpu, orc, 2, 9, None)
    gpu.close()
