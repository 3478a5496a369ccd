"""GPU suite: the front end of k_knn_rank (csrc/map_obs_rank.hip: the table of checkpoints per 32-road chunk, the block cull
that reads it, the ordered scan) at the world sizes where it takes another path -- 208 roads (13 blocks, half a chunk at the
end), 1024 (exactly one batch of the cull), 1040 (a second batch of one block), 2064 (three batches, the last partial), an
inward spiral of 1300 roads on which every road is a candidate (a checkpoint in every chunk until the 40 are used, then the
long list), and one world at 128 slots.  One world each, at most 8 agents, three steps and a reset, in lockstep with the
oracle, with the checks of tests/test_gpu_rank_candidates.py after every selection: rows within the suite's tolerances, every
live agent on the rank path, candidates beyond K at least the oracle's inserts per agent, gd_stat 21 == 0.

Rows cannot tell a candidate set that drifted to another superset; the counts can: debug_road_path() after every selection is
compared with tests/golden/rank_front_end_counts.json, recorded from the commit before this front end
(tools/rank_front_end_counts.py <library> --out <file> runs this file against any build of the library and writes what it sees;
--check compares with the golden file)."""
import json
import math
import os

import numpy as np
import pytest

from gpudrive_lab_amd import synth
from tests import parity as P
from tests import ref_cases as RC
from tests.test_gpu_rank_candidates import BENCH, _run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rank_front_end_counts.json")
RECORD = os.environ.get("GPUDRIVE_RANK_FRONT_END_RECORD")  # (the tool: write the counts to this file instead of comparing them)

#         name: (scene seed, agents, polylines, points per polyline, slots, roads)
CASES = {
    "roads_208": (21, 8, 13, 17, 64, 208),
    "roads_1024": (22, 8, 8, 129, 64, 1024),
    "roads_1040": (23, 8, 8, 131, 64, 1040),
    "roads_2064": (24, 8, 16, 130, 64, 2064),
    "spiral_1300": (25, 6, 10, 131, 64, 1300),
    "slots_128": (26, 8, 8, 131, 128, 1040),
}


def _scene(case):
    seed, agents, polylines, pts, _, roads = CASES[case]
    scene = synth.make_scene(seed, n_agents=agents, n_polylines=polylines, pts_per_polyline=pts)
    if case.startswith("spiral"):
        # one inward spiral around the agents, cut into polylines that each start where the last one ended: the radius falls by
        # 55 m over K = 200 roads, more than an agent's distance to the roads swings over a turn (the agents stay within 25 m of
        # the centre), so every road is nearer than the K-th nearest before it, for every agent
        cx = float(np.mean([o["position"][0]["x"] for o in scene["objects"]]))
        cy = float(np.mean([o["position"][0]["y"] for o in scene["objects"]]))
        k = 0
        for road in scene["roads"]:
            geom = []
            for j in range(pts):
                rho, ph = 400.0 - 0.277 * (k + j), 0.05 * (k + j)
                geom.append({"x": cx + rho * math.cos(ph), "y": cy + rho * math.sin(ph), "z": 0.0})
            road["geometry"] = geom
            k += pts - 1
        for o in scene["objects"]:  # slow agents: they stay near the centre
            vx, vy = o["velocity"][0]["x"] * 0.2, o["velocity"][0]["y"] * 0.2
            x0, y0 = o["position"][0]["x"], o["position"][0]["y"]
            o["position"] = [{"x": x0 + vx * 0.1 * t, "y": y0 + vy * 0.1 * t, "z": 0.0} for t in range(91)]
            o["velocity"] = [{"x": vx, "y": vy}] * 91
            o["goalPosition"] = {"x": o["position"][-1]["x"], "y": o["position"][-1]["y"], "z": 0.0}
    assert polylines * (pts - 1) == roads
    return scene


@pytest.mark.parametrize("case", list(CASES))
def test_front_end(case, oracle_mod, tmp_path, monkeypatch):
    monkeypatch.setenv("GPUDRIVE_RANK_MIN_ROADS", "200")
    seed, agents, _, _, slots, roads = CASES[case]
    path = tmp_path / ("%s.json" % case)
    path.write_text(json.dumps(_scene(case)))
    gpu = P.make_gpu_sim([str(path)], max_agents=slots, **BENCH)
    orc = P.make_oracle_sim(oracle_mod, [str(path)], max_agents=slots, **BENCH)
    shape = RC.as_np(gpu.shape_tensor())
    assert int(shape[0, 0]) == agents and int(shape[0, 1]) == roads, "the case became another one: %s" % shape[0].tolist()
    paths = _run(gpu, orc, 3, seed, 0)
    counts = [p[0, :agents].tolist() for p in paths]
    print("%s: candidate counts %s" % (case, counts))
    assert len(counts) == 4
    if case.startswith("spiral"):
        assert max(max(c) for c in counts) > 1272, "no agent of the spiral went to the long list"
    else:
        assert all(max(c) <= 1272 for c in counts), "the standard ranking holds these worlds' candidates"
    gpu.close()
    if RECORD:
        seen = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        seen[case] = counts
        with open(RECORD, "w") as fh:
            json.dump(seen, fh, indent=0, sort_keys=True)
        return
    want = json.load(open(GOLDEN))[case]
    assert counts == want, "%s: the candidate counts are not those of the recorded front end: %s, recorded %s" % (case, counts, want)
