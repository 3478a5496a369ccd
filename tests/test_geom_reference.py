"""CPU suite: the float64 BEV / LiDAR references (tests/geom_reference.py) against hand-checked answers, and the oracle against
the references on the constructed worlds (tests/geom_cases.py) and on the Waymo BEV combinations -- outside the references' own
margin masks hit / miss, entity type and cell value are equal without exception."""
import math

import numpy as np
import pytest

from tests import geom_cases as GC
from tests import geom_reference as GR
from tests import parity as P
from tests.conftest import SCENE_4, TEST_JSON


# ------------------------------------------------------------------------------------------------------------------
# the references themselves, against answers worked out by hand
# ------------------------------------------------------------------------------------------------------------------
def _inputs(agents, roads):
    """Reference inputs for one world written by hand.  agents: (x, y, z, yaw, length, width, type); roads: 9-float rows."""
    n, R = len(agents), len(roads)
    st = np.zeros((1, max(n, 1), 11), np.float32)
    ab = np.zeros((1, max(n, 1), 14), np.float32)
    info = np.zeros((1, max(n, 1), 5), np.int32)
    for i, (x, y, z, yaw, length, width, t) in enumerate(agents):
        st[0, i, :3] = (x, y, z)
        st[0, i, 3], st[0, i, 6] = math.cos(yaw / 2), math.sin(yaw / 2)
        ab[0, i, 10:12] = (length, width)
        info[0, i, 4] = t
    mo = np.zeros((1, max(R, 1), 9), np.float32)
    for r, row in enumerate(roads):
        mo[0, r] = row
    return dict(shape=np.asarray([[n, R]], np.int32), state=st, abs_obs=ab, info=info, controlled=np.zeros((1, max(n, 1), 1), np.int32),
                action=np.zeros((1, max(n, 1), 10), np.float32), map_obs=mo)


def test_lidar_reference_on_one_box_dead_ahead():
    """A 4 x 2 m box (a crosswalk: scales 2, 1, 0.1, z 0.9 +- 0.1) centred 10 m dead ahead of an agent at z = 1, 120 degree
    cone.  Ray idx = 25 points straight ahead and meets the front face at t = 10 - 2 = 8.  The front face spans |y| <= 1 at
    x = 8, so a ray at angle th meets it when |tan th| <= 1 / 8, |th| <= 0.12435: rays are 2 pi / 150 = 0.041888 apart, so
    idx 23 ... 27 (|th| <= 0.08378) hit at t = 8 / cos th and idx 22 / 28 (0.12566) pass the corner -- they cross x = 8 at
    |y| = 1.0106 and only move outwards.  Only plane 2 (height 0.9) lies in the box's z range [0.8, 1.0]."""
    inp = _inputs([(0.0, 0.0, 1.0, 0.0, 4.0, 2.0, 7)], [(10.0, 0.0, 2.0, 1.0, 0.1, 0.0, 4, 0, 0)])
    ref = GR.lidar_reference(inp, 0, 0, 0.0)
    out = ref["out"]
    assert not out[0].any() and not out[1].any()
    hit = np.nonzero(out[2, :, 0] > 0)[0]
    assert hit.tolist() == [23, 24, 25, 26, 27]
    step = 2 * GR.lidar_half_angle(0.0) / 50
    for idx in hit:
        th = (idx - 25) * step
        assert abs(out[2, idx, 0] - 8 / math.cos(th)) < 1e-9 and out[2, idx, 1] == 4
        assert abs(out[2, idx, 2] - 8.0) < 1e-9 and abs(out[2, idx, 3] - 8 * math.tan(th)) < 1e-9
    assert out[2, 25, 0] == 8.0 and out[2, 25, 3] == 0.0
    assert not ref["margin"].any()
    # the same box turned by a quarter turn is 2 x 4 m: front face at x = 9, |tan th| <= 2 / 9 -> five rays either side
    inp["map_obs"][0, 0, 5] = np.float32(math.pi / 2)
    out = GR.lidar_reference(inp, 0, 0, 0.0)["out"]
    assert np.nonzero(out[2, :, 0] > 0)[0].tolist() == list(range(20, 31)) and abs(out[2, 25, 0] - 9.0) < 1e-6
    # behind the agent nothing is hit in the cone; all the way round (half angle pi) ray 0 points astern
    inp["map_obs"][0, 0, 0] = -10.0
    assert not GR.lidar_reference(inp, 0, 0, 0.0)["out"].any()
    assert abs(GR.lidar_reference(inp, 0, 0, math.pi)["out"][2, 0, 0] - 9.0) < 1e-5


def test_lidar_reference_rules():
    """Front faces only, range, plane eligibility and the tie rule, each on a two-entity world."""
    me = (0.0, 0.0, 1.0, 0.0, 4.0, 2.0, 7)
    # an agent around the origin is not hit; the one behind it is (plane 0 and 1: equal z)
    inp = _inputs([me, (0.5, 0.0, 1.0, 0.3, 10.0, 6.0, 7), (20.0, 0.0, 1.0, 0.0, 4.0, 2.0, 9)], [])
    ref = GR.lidar_reference(inp, 0, 0, 0.0)
    assert not (ref["row"] == 1).any() and ref["row"][0, 25] == 2 and ref["row"][2, 25] == -1
    assert abs(ref["out"][0, 25, 0] - (20 - 0.7 * 2)) < 1e-6 and ref["out"][0, 25, 1] == 9
    # 200 m: a face at 199.9 is hit, at 200.1 not
    for x, want in ((201.3, True), (201.5, False)):
        inp = _inputs([me, (x, 0.0, 1.0, 0.0, 4.0, 2.0, 7)], [])
        assert (GR.lidar_reference(inp, 0, 0, 0.0)["row"][0, 25] == 1) == want
    # equal distance: the lower row's type
    a, b = (10.0, 0.0, 2.0, 0.1, 0.1, 0.0, 3, 0, 0), (10.0, 0.0, 2.0, 0.1, 0.1, 0.0, 2, 0, 0)
    for rows, want in (((a, b), 3), ((b, a), 2)):
        ref = GR.lidar_reference(_inputs([me], rows), 0, 0, 0.0)
        assert ref["out"][2, 25, 1] == want and ref["row"][2, 25] == 1 and not ref["margin"][2, 25]


def test_bev_reference_on_one_axis_aligned_partner():
    """A 4 x 2 m partner at yaw 0, at (10, 0) in the frame of an ego at yaw 0, radius 50: cells are 0.5 m, cell x has its centre
    at 0.5 x - 50.  Painted: |0.5 x - 60| <= 2.001 and |0.5 y - 50| <= 1.001, i.e. x = 116 ... 124 and y = 98 ... 102, 45 cells.
    The centre falls exactly on cell corner (120, 100): that is a knife edge the reference must report.  Moved to (10.2, 0.1):
    |0.5 x - 60.2| <= 2.001 -> x = 117 ... 124; |0.5 y - 50.1| <= 1.001 -> y = 99 ... 102."""
    grid, margin, knife = GR.paint_rectangles(np.asarray([[10.0, 0.0, 0.0, 4.0, 2.0, 7]]), 50.0)
    want = np.zeros((200, 200), np.int32)
    want[98:103, 116:125] = 7
    assert np.array_equal(grid, want) and knife
    # every cell of the outline has its centre exactly 1e-3 inside the painted extent, the rounding of 2.001 - 2 decides whether
    # that counts as "within 1e-3": nothing but outline cells may be marked
    outline = want.astype(bool)
    outline[99:102, 117:124] = False
    assert not (margin & ~outline).any()
    inp = _inputs([(5.0, 5.0, 1.0, 0.0, 4.0, 2.0, 7), (15.2, 5.1, 1.0, 0.0, 4.0, 2.0, 9)], [])
    ref = GR.bev_reference(inp, 0, 0, 50.0)
    want[:] = 0
    want[99:103, 117:125] = 9
    assert ref["usable"] and np.array_equal(ref["grid"], want) and not ref["margin"].any()
    assert ref["n_roads"] == 0 and ref["n_partners"] == 1
    # the ego turned by a quarter turn to the left sees it on its right, at (0.1, -10.2)
    inp["state"][0, 0, 3], inp["state"][0, 0, 6] = math.cos(math.pi / 4), math.sin(math.pi / 4)
    ref = GR.bev_reference(inp, 0, 0, 50.0)
    ys, xs = np.nonzero(ref["grid"])
    # relative yaw -pi/2: the 4 m side now runs along y; centre (0.1, -10.2): |0.5 x - 50.1| <= 1.001, |0.5 y - 39.8| <= 2.001
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (99, 102, 76, 83)


def test_bev_reference_roads_width_floor_cap_and_order():
    """A road is painted with half its first scale as half length and its width floored at one cell; the 201st road in reach is
    not painted; a partner is painted over a road."""
    ego = (0.0, 0.0, 1.0, 0.0, 4.0, 2.0, 7)
    # scales (8, 0.1): half length 4, width max(0.1, 0.5) -> half width 0.25: |0.5 x - 60.2| <= 4.001, |0.5 y - 50.1| <= 0.251
    ref = GR.bev_reference(_inputs([ego], [(10.2, 0.1, 8.0, 0.1, 0.1, 0.0, 1, 0, 0)]), 0, 0, 50.0)
    ys, xs = np.nonzero(ref["grid"])
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (113, 128, 100, 100) and ref["usable"]
    rows = [(-20.3 + 0.1 * k, 3.1, 0.4, 0.1, 0.1, 0.0, 1, 0, 0) for k in range(200)] + [(10.2, 0.1, 8.0, 0.1, 0.1, 0.0, 3, 0, 0)]
    ref = GR.bev_reference(_inputs([ego, (10.2, 0.1, 1.0, 0.0, 1.0, 1.0, 8)], rows), 0, 0, 50.0)
    assert ref["n_roads"] == 200 and 3 not in ref["grid"] and ref["grid"][100, 120] == 8
    ref = GR.bev_reference(_inputs([ego, (10.2, 0.1, 1.0, 0.0, 1.0, 1.0, 8)], rows[1:]), 0, 0, 50.0)
    assert ref["grid"][100, 120] == 8 and ref["grid"][100, 114] == 3
    # out of the radius: not painted; within 1e-3 of it: the raster is reported unusable
    assert not GR.bev_reference(_inputs([ego, (50.2, 0.1, 1.0, 0.0, 4.0, 2.0, 7)], []), 0, 0, 50.0)["grid"].any()
    assert not GR.bev_reference(_inputs([ego, (50.0004, 0.0, 1.0, 0.0, 4.0, 2.0, 7)], []), 0, 0, 50.0)["usable"]


# ------------------------------------------------------------------------------------------------------------------
# the oracle against the references
# ------------------------------------------------------------------------------------------------------------------
def _lidar_check(case, orc, variant, tag, stats):
    got = GC.compare_lidar_to_reference(orc, variant, tag)
    stats["masked"] = stats.get("masked", 0) + got["share"] * got["rays"]
    stats["rays"] = stats.get("rays", 0) + got["rays"]
    stats["depth"] = max(stats.get("depth", 0.0), got["depth"])


def _bev_check(case, orc, variant, tag, stats):
    rasters = [(w, a) for w, agents in enumerate(case.rasters) for a in agents]
    assert len(rasters) <= 8
    got = GC.compare_bev_to_reference(orc, variant, tag, rasters)
    for k, v in got.items():
        stats[k] = stats.get(k, 0) + v


def _report(name, kind, stats):
    if kind == "lidar":
        share = stats["masked"] / stats["rays"]
        print("GEOM %s: rays per plane %d, masked share per plane %s, depth |oracle - reference| %.3g" %
              (name, stats["rays"], np.round(share, 5).tolist(), stats["depth"]))
        assert (share <= GC.LIDAR_MARGIN_RAYS).all(), share
        assert stats["depth"] <= GC.ORACLE_DEPTH_MAX, stats["depth"]
    else:
        cells, painted = stats["masked"] / stats["cells"], stats["masked_painted"] / max(stats["painted"], 1)
        print("GEOM %s: cells %d, painted %d, masked share of cells %.5f, of painted cells %.5f" %
              (name, stats["cells"], stats["painted"], cells, painted))
        assert stats["painted"] > 0
        assert cells <= GC.BEV_MARGIN_CELLS and painted <= GC.BEV_MARGIN_PAINTED, (cells, painted)


@pytest.mark.parametrize("name", list(GC.CASES))
def test_oracle_meets_the_reference_on_constructed_worlds(oracle_mod, tmp_path, name):
    """Reset pass (poses written with set_state) and a State-model step pass that moves two agents, every variant of the case."""
    case = GC.CASES[name]
    scenes = case.write(tmp_path)
    check = _lidar_check if case.kind == "lidar" else _bev_check
    stats = {}
    for k, variant in enumerate(case.variants):
        for model in (0, 3):
            kw, okw, _ = case.params(variant, model)
            orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=case.slots, **kw, **okw)
            GC.place(case, [orc], k)
            if model == 0:
                print("GEOM %s premise (%g): %s" % (name, variant, case.premise(case, GR.read_inputs(orc), variant)))
            else:
                np.copyto(orc.action_tensor(), GC.state_step_actions(case, orc))
                orc.step()
            check(case, orc, variant, "%s (%g, %s pass)" % (name, variant, "reset" if model == 0 else "step"), stats)
            orc.close()
    _report(name, case.kind, stats)


WAYMO_BEV = [(scene, thr, radius) for scene in (SCENE_4, TEST_JSON) for radius, thr in ((50.0, 0.1), (100.0, 0.0), (20.0, 0.1))]


@pytest.mark.parametrize("scene,thr,radius", WAYMO_BEV, ids=["%s-r%g-t%g" % (s.split("_")[-1].split("/")[-1], r, t) for s, t, r in WAYMO_BEV])
def test_oracle_bev_meets_the_reference_on_waymo_scenes(oracle_mod, scene, thr, radius):
    """The first 8 live agents of the scene whose raster has no discrete decision on a knife edge (chosen by the reference)."""
    orc = P.make_oracle_sim(oracle_mod, [scene], max_agents=64, polylineReductionThreshold=thr, observationRadius=radius,
                            collisionBehaviour=2, rewardType=1, distanceToGoalThreshold=2.0, dynamicsModel=0, enableBev=1,
                            isStaticAgentControlled=1, initOnlyValidAgentsAtFirstStep=0, IgnoreNonVehicles=0)
    inp = GR.read_inputs(orc)
    rasters = [(0, a) for a in range(int(inp["shape"][0, 0])) if abs(inp["state"][0, a, 0]) < 1e4 and
               GR.bev_reference(inp, 0, a, radius)["usable"]][:8]
    assert len(rasters) == 8
    stats = GC.compare_bev_to_reference(orc, radius, "waymo", rasters)
    orc.close()
    _report("waymo %s r%g t%g" % (scene.split("/")[-1][:24], radius, thr), "bev", stats)
