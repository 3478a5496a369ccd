"""GPU suite: the observations a STEP writes, held to the oracle at every step.

The lockstep tests elsewhere compare the step's ints and state, then inject the oracle's state and compare the observations
of a reset pass -- and injection makes the next step a full pass.  The step's own rows, rasters, returns and packed columns,
i.e. what the skip machinery (pose stamps, the linear scan's step list, the BEV / LiDAR dirty flags, the direct pack) leaves
behind, are compared here: the State model (dynamicsModel = 3) writes position, yaw and velocity straight from the action on
both sides, so on the same scripted actions the two states stay bit-identical and no injection is needed
(tests/parity.py scripted_state_lockstep).  Most agents are handed back their own pose (their rows may be left in place), a
few are shifted or turned, and a controlled car is put on a parked (Static) one now and then -- under AgentRemoved that
moves the parked car to the padding position, which a Static-free step list never visits.  Through a partial reset, a
set_maps and a deleteAgents, with every step compared before and after them."""
import pytest

from tests import parity as P
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

# the default init rules (parked cars are Static), State model
BASE = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0, dynamicsModel=3,
            isStaticAgentControlled=0, initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1)

# road selection: (knn_order, roadObservationAlgorithm, environment)
ROADS = {
    "ref_order_rank": (0, 0, {"GPUDRIVE_RANK_MIN_ROADS": "200"}),
    "ref_order_history": (0, 0, {"GPUDRIVE_NO_RANK_REPLAY": "1"}),
    "set_order_fused": (1, 0, {"GPUDRIVE_SET_FUSED_ROWS": "1"}),
    "set_order_row_kernel": (1, 0, {"GPUDRIVE_SET_FUSED_ROWS": "0"}),
    "linear": (0, 1, {}),
}

STEPS = 36


def _events(scenes):
    """Hits before steps 4, 14, 24 and 31; a partial reset after step 11, a set_maps after step 21 and a deleteAgents after
    step 28 (the step behind each is a full pass, the ones after it skip again)."""
    W = len(scenes)
    every = list(range(W))
    return {3: [("hit", every)],
            10: [("reset", [0, W - 1])],
            13: [("hit", [0, W - 1])],
            20: [("set_maps", scenes[1:] + scenes[:1])],
            23: [("hit", every)],
            27: [("delete", {1: [0]})],
            30: [("hit", every)]}


def _run(O, monkeypatch, tmp_path, case, roads, scenes, slots, cb, bev=False, lidar_half_angle=None, pack=None):
    knn_order, algo, env = ROADS[roads]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scenes = scenes + [P.parked_car_scene(tmp_path)]
    kw = dict(BASE, roadObservationAlgorithm=algo, collisionBehaviour=cb)
    okw = dict(kw)
    gkw = dict(knn_order=knn_order)
    if bev:
        okw["enableBev"] = 1
        gkw["enable_bev"] = True
    if lidar_half_angle is not None:
        kw["enableLidar"] = okw["enableLidar"] = 1
        okw["lidarHalfAngle"] = lidar_half_angle
        gkw["lidar_half_angle"] = lidar_half_angle
    gpu = P.make_gpu_sim(scenes, max_agents=slots, **gkw, **kw)
    orc = P.make_oracle_sim(O, scenes, max_agents=slots, **okw)
    if pack is not None:
        assert gpu.direct_pack(only=pack == "only")
    try:
        got = P.scripted_state_lockstep(gpu, orc, STEPS, events=_events(scenes), roads_as_set=knn_order == 1, pack=pack,
                                        bev=bev, lidar=lidar_half_angle is not None)
    finally:
        gpu.close()
    assert got["parked_hit"] > 0, "no parked car was hit"
    if cb == 1:
        assert got["parked_removed"] > 0, "no parked car was moved to the padding position"
    print("STEP_OUTPUTS %s steps=%d elements=%d stat30=%d parked_hit=%d parked_removed=%d" %
          (case, got["steps"], got["elements"], got["skipped"], got["parked_hit"], got["parked_removed"]))
    return got


MATRIX = [(roads, cb, 64) for roads in ROADS for cb in (0, 1, 2)] + \
         [(roads, cb, 128) for roads in ("ref_order_rank", "linear") for cb in (0, 1, 2)]


@pytest.mark.parametrize("roads,cb,slots", MATRIX, ids=["%s-cb%d-%d" % c for c in MATRIX])
def test_step_outputs_match_the_oracle(oracle_mod, monkeypatch, tmp_path, roads, cb, slots):
    _run(oracle_mod, monkeypatch, tmp_path, "%s-cb%d-%d" % (roads, cb, slots), roads, [TEST_JSON, SCENE_407, SCENE_4], slots, cb)


def test_step_bev_matches_the_oracle(oracle_mod, monkeypatch, tmp_path):
    _run(oracle_mod, monkeypatch, tmp_path, "bev", "linear", [SCENE_407], 64, 1, bev=True)


@pytest.mark.parametrize("half_angle", [0.0, 3.14159265], ids=["120deg", "360deg"])
def test_step_lidar_matches_the_oracle(oracle_mod, monkeypatch, tmp_path, half_angle):
    _run(oracle_mod, monkeypatch, tmp_path, "lidar-%g" % half_angle, "linear", [SCENE_4], 64, 1, lidar_half_angle=half_angle)


PACK = [("linear", "only"), ("linear", "both"), ("ref_order_rank", "only")]


@pytest.mark.parametrize("roads,pack", PACK, ids=["%s-%s" % c for c in PACK])
def test_step_direct_pack_matches_the_oracle(oracle_mod, monkeypatch, tmp_path, roads, pack):
    _run(oracle_mod, monkeypatch, tmp_path, "pack-%s-%s" % (roads, pack), roads, [TEST_JSON, SCENE_407], 64, 1, pack=pack)
