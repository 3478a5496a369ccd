"""Constructed worlds for the BEV and LiDAR references (tests/geom_reference.py): each case aims the geometry at one piece of
k_bev / k_lidar that the Waymo scenes never reach, and asserts its own premise FROM THE REFERENCE'S GEOMETRY so that it cannot
quietly stop exercising that piece.

Scenes are JSON dicts in the reference's scene format, written at run time.  Every agent stands still in the log (its goal is
far away, so it is Dynamic and controlled unless marked as an expert); poses -- z and yaw included -- are then written with
set_state / debug_set_state and recomputed through reset([]) on both simulators, head angles go into the action tensor first.
All cases: collisionBehaviour = 2, polylineReductionThreshold = 0.

The comparison helpers at the bottom hold any simulator (the oracle on the CPU, the HIP engine on the GPU) to the reference
outside the reference's own margin masks."""
import json
import math
import os

import numpy as np

from tests import geom_reference as GR
from tests import parity as P

f32 = np.float32
PI = float(np.pi)

# Largest |oracle - reference| of a LiDAR depth or hit position (columns 0, 2, 3) over every non-marginal hit ray of every case
# below, reset and step pass: measured 8.00e-4 m (lidar_fork128, step pass).  The depth of a glancing return is ill-conditioned
# -- a ray that meets a face at incidence angle i turns an error e across the face into e / sin i along the ray -- and the 400
# agent-by-segment pairs of that world hold a few: every case but lidar_fork128 stays below 9.5e-5 (one ulp of a float32
# coordinate at 200 m is 1.5e-5, and the oracle's ray direction carries the float32 rounding of cos / sin over up to 200 m).
# The GPU test allows twice this (the kernel multiplies by v_rcp_f32's reciprocal where the oracle divides: about one ulp more
# per operation; nothing else differs).
ORACLE_DEPTH_MAX = 8.1e-4
GPU_DEPTH_FACTOR = 2.0

# Conditions on the reference's own masks (not measurements: a case that exceeds one has its geometry moved)
BEV_MARGIN_CELLS = 1e-3       # share of a case's cells
BEV_MARGIN_PAINTED = 2e-2     # share of a case's painted cells
LIDAR_MARGIN_RAYS = 1e-2      # share of a case's rays, per plane


# ------------------------------------------------------------------------------------------------------------------
# scene building
# ------------------------------------------------------------------------------------------------------------------
def car(i, x, y, yaw, length=4.0, width=2.0, kind="vehicle", expert=False):
    return {"position": [{"x": float(x), "y": float(y), "z": 0.0}] * 91, "width": float(width), "length": float(length),
            "height": 1.6, "heading": [float(yaw)] * 91, "velocity": [{"x": 0.0, "y": 0.0}] * 91, "valid": [True] * 91,
            "goalPosition": {"x": float(x) + 1000.0, "y": float(y), "z": 0.0}, "type": kind, "id": i,
            "mark_as_expert": bool(expert)}


def road(rid, kind, pts):
    return {"geometry": [{"x": float(x), "y": float(y), "z": 0.0} for x, y in pts], "type": kind,
            "map_element_id": {"road_edge": 15, "road_line": 6, "lane": 2, "crosswalk": 18, "speed_bump": 19,
                               "stop_sign": 17}[kind], "id": rid}


def scene(name, cars, roads):
    return {"name": name, "scenario_id": name, "objects": cars, "roads": roads, "tl_states": {},
            "metadata": {"sdc_track_index": 0, "objects_of_interest": [], "tracks_to_predict": []}}


def segment(cx, cy, ang, half_len):
    dx, dy = half_len * math.cos(ang), half_len * math.sin(ang)
    return [(cx - dx, cy - dy), (cx + dx, cy + dy)]


class World:
    """One scene and the poses written over it: z and yaw per live agent (x, y stay where the log puts them), head angles."""

    def __init__(self, name, cars, roads, z=None, heads=None, moves=()):
        self.n = len(cars)
        # (a yaw whose rotation the host's and the device's sin / cos give the same bits for: the logged heading too, so that
        # an expert agent the step puts back on its log has the same state on both sides)
        self.yaw = np.asarray([P.agreeing_yaw(f32(c["heading"][0])) for c in cars], f32)
        for c, yaw in zip(cars, self.yaw):
            c["heading"] = [float(yaw)] * 91
        self.scene = scene(name, cars, roads)
        self.z = np.ones(self.n, f32) if z is None else np.asarray(z, f32)
        self.heads = np.zeros(self.n, f32) if heads is None else np.asarray(heads, f32)
        self.moves = list(moves)   # the step pass: (agent, dx, dy, dyaw) for two controlled agents


class Case:
    def __init__(self, name, kind, worlds, variants, slots=64, rasters=None, premise=None, heads_for=None):
        self.name, self.kind, self.worlds, self.variants, self.slots = name, kind, worlds, variants, slots
        self.rasters = rasters          # BEV: per world, the agents whose rasters are compared (at most 8 per case)
        self.premise = premise          # premise(case, inp, variant): asserts, returns a short text
        self.heads_for = heads_for      # optional: head angles per variant index

    def write(self, directory):
        paths = []
        for wd in self.worlds:
            path = os.path.join(str(directory), wd.scene["name"] + ".json")
            with open(path, "w") as f:
                json.dump(wd.scene, f)
            paths.append(path)
        return paths

    def params(self, variant, model=0):
        """(shared parameters, oracle-only, HIP-only) for one variant: a half angle (lidar) or a radius (bev)."""
        kw = dict(polylineReductionThreshold=0.0, collisionBehaviour=2, dynamicsModel=model,
                  observationRadius=float(variant) if self.kind == "bev" else 50.0)
        if self.kind == "lidar":
            kw["enableLidar"] = 1
            return kw, dict(lidarHalfAngle=float(variant)), dict(lidar_half_angle=float(variant))
        return kw, dict(enableBev=1), dict(enable_bev=True)


def quat_of_yaw(yaw):
    """q_angle_axis_up of a float32 yaw, rounded once from double (what both simulators store for an agreeing yaw)."""
    half = np.asarray(yaw, f32) / f32(2)
    c, s = np.cos(half.astype(np.float64)).astype(f32), np.sin(half.astype(np.float64)).astype(f32)
    return np.stack([c, f32(0) * s, f32(0) * s, s], -1)


def place(case, sims, variant_index=0):
    """Write the case's poses and head angles into every simulator of `sims` (the first one's state is the template, so all
    hold the same bits) and recompute through reset([])."""
    st = sims[0].get_state() if hasattr(sims[0], "get_state") else sims[0].debug_get_state()
    act = np.zeros(st.shape[:2] + (10,), f32)
    for w, wd in enumerate(case.worlds):
        st[w, :wd.n, 2] = wd.z
        st[w, :wd.n, 3:7] = quat_of_yaw(wd.yaw)
        st[w, :wd.n, 7:10] = 0
        st[w, :wd.n, 10] = 0
        heads = wd.heads if case.heads_for is None else case.heads_for(wd, variant_index)
        act[w, :wd.n, 2] = heads
    for s in sims:
        (s.set_state if hasattr(s, "set_state") else s.debug_set_state)(st)
        P.write_actions(s, act)
        s.reset([])


def state_step_actions(case, sim):
    """State-model actions for one step: every agent is handed back its own pose, except each world's two `moves`."""
    st = sim.get_state() if hasattr(sim, "get_state") else sim.debug_get_state()
    act = np.zeros(st.shape[:2] + (10,), f32)
    act[..., 0:3] = st[..., 0:3]
    for w, wd in enumerate(case.worlds):
        yaw = wd.yaw.copy()
        assert len(wd.moves) == 2
        for a, dx, dy, dyaw in wd.moves:
            act[w, a, 0] += f32(dx)
            act[w, a, 1] += f32(dy)
            yaw[a] = P.agreeing_yaw(f32(yaw[a] + f32(dyaw)))
        act[w, :wd.n, 3] = yaw
    return act


# ------------------------------------------------------------------------------------------------------------------
# LiDAR cases
# ------------------------------------------------------------------------------------------------------------------
ROAD_KINDS = ("road_edge", "lane", "road_line")


def _heavy_world(front):
    """One hub agent inside the bounding circle of 320 two-point polylines, 15-25 m long, laid tangentially 5-9 m around it
    (all the way round, or packed into the 120 degree cone in front of it); six more agents 10-60 m out."""
    rng = np.random.default_rng(3 if front else 2)
    hub_yaw = 0.3
    cars = [car(0, 0.0, 0.0, hub_yaw)]
    for k, dist in enumerate((10.5, 18.0, 27.0, 36.0, 48.0, 60.0)):
        ang = hub_yaw + (-0.8 + 0.32 * k if front else 0.4 + 1.05 * k)
        cars.append(car(k + 1, dist * math.cos(ang), dist * math.sin(ang), ang + 2.0 + 0.3 * k, length=4.0 + 0.2 * k,
                        expert=k == 5))
    roads = []
    for i in range(320):
        hl = rng.uniform(7.5, 12.5)
        r = 5.0 + rng.uniform(0, 1) * min(4.0, hl - 5.5)
        phi = hub_yaw + rng.uniform(-0.9, 0.9) if front else rng.uniform(-PI, PI)
        # (edges and lanes only: every plane then sees one road type, and crossing segments cannot disagree about the type)
        roads.append(road(i, ROAD_KINDS[i % 2], segment(r * math.cos(phi), r * math.sin(phi),
                                                        phi + PI / 2 + rng.uniform(-0.3, 0.3), hl)))
    return World("heavy_front" if front else "heavy_ring", cars, roads, moves=[(0, 0.25, -0.15, 0.05), (2, -0.4, 0.3, 0.0)])


def _heavy_premise(case, inp, half):
    out = []
    for w in range(len(case.worlds)):
        count, mask = GR.subtended_rays(inp, w, 0, half)
        wide = int(((count >= 25) & (mask != 0)).sum())
        assert wide >= 300, "world %d: only %d eligible entities subtend >= 25 rays of the hub" % (w, wide)
        out.append("world %d: %d eligible entities subtend >= 25 rays of the hub (kernel heavy list: 256)" % (w, wide))
    return "; ".join(out)


def _planes_world(name="planes"):
    """12 agents at heights that give an agent target every plane mask the z rules can produce, road edges, lines, lanes, a
    crosswalk, a speed bump and a stop sign in reach; entities dead ahead, dead astern and abeam of agents at yaw 0 and pi."""
    poses = [  # x, y, yaw, z
        (0.0, 0.0, 0.0, 1.0), (12.0, 0.0, 0.0, 1.0), (-12.0, 0.0, PI / 2, 0.2), (0.0, 12.0, 0.7, -0.45),
        (0.0, -12.0, -1.2, 1.34), (9.0, 9.0, 2.0, 1.75), (-9.0, 9.0, -2.6, 2.62), (-9.0, -9.0, 3.0, 0.55),
        (9.0, -9.0, 1.0, 2.07), (20.0, 0.0, PI, 1.0), (-18.0, -4.0, 0.2, 0.72), (3.0, 22.0, -1.57, 1.52)]
    cars = [car(i, x, y, yaw, length=4.0 + 0.1 * i, width=1.8 + 0.05 * i, kind=("vehicle", "cyclist", "pedestrian")[i % 3],
                expert=i == 11) for i, (x, y, yaw, z) in enumerate(poses)]
    ring = [(30.0 * math.cos(0.55 * k), 26.0 * math.sin(0.55 * k)) for k in range(12)]
    roads = [road(0, "road_edge", ring),
             road(1, "road_line", [(-25.0 + 12.5 * k, -6.0 + 0.4 * (k % 2)) for k in range(5)]),
             road(2, "lane", [(-25.0 + 12.5 * k, 6.0 - 0.3 * (k % 2)) for k in range(5)]),
             road(3, "stop_sign", [(6.0, 15.0)]),
             road(4, "crosswalk", [(-7.0, -17.0), (-3.0, -17.0), (-3.0, -15.0), (-7.0, -15.0)]),
             road(5, "speed_bump", [(14.0, -16.0), (17.0, -15.0), (16.5, -13.5), (13.5, -14.5)]),
             road(6, "road_edge", [(-4.0, 16.0), (4.0, 17.0)])]
    return World(name, cars, roads, z=[p[3] for p in poses], moves=[(0, 0.25, -0.15, 0.05), (4, -0.3, 0.2, -0.05)])


POSSIBLE_MASKS = (0, 1, 2, 3, 4, 6, 7)   # 5 (planes 0 and 2 without plane 1 between them) is impossible for a z interval


def _planes_premise(case, inp, half):
    seen = {}
    ents = GR.lidar_entities(inp, 0)
    for a in range(ents["n"]):
        _, mask = GR.subtended_rays(inp, 0, a, half, ents)
        for e, m in enumerate(mask):
            if e != a:
                seen.setdefault(int(m), (a, e))
        _, near = GR.plane_masks(ents, float(inp["state"][0, a, 2]))
        near[:, a] = False
        assert not near.any(), "agent %d: a plane height sits on an entity's z bound" % a
    missing = [m for m in POSSIBLE_MASKS if m not in seen]
    assert not missing and 5 not in seen, "plane masks missing %s (seen %s)" % (missing, sorted(seen))
    agent_masks = set()
    for a in range(ents["n"]):
        mask = GR.subtended_rays(inp, 0, a, half, ents)[1]
        agent_masks |= {int(mask[e]) for e in range(ents["n"]) if e != a}
    agent_masks = sorted(agent_masks)
    assert agent_masks == [0, 1, 3, 4, 6, 7], agent_masks
    return "plane masks (origin, entity row): " + ", ".join("%d:%s" % (m, seen[m]) for m in sorted(seen)) + \
        "; agent targets give " + str(agent_masks)


HEADS = (-PI, -2.5, -0.5, 0.0, 0.5, 2.5, PI)


def _wrap_heads(wd, k):
    return np.asarray([HEADS[(a + k) % len(HEADS)] for a in range(wd.n)], f32)


def _wrap_premise(case, inp, half):
    st = inp["state"][0].astype(np.float64)
    found = set()
    for a in (0, 1, 9):   # the agents at yaw 0 / pi on the x axis
        rx, ry = GR._to_frame(st[:12, 0], st[:12, 1], st[a, 0], st[a, 1], GR.yaw_of(st[a, 3:7]))
        phi = np.arctan2(ry, rx)
        for e in range(12):
            if e == a:
                continue
            if abs(phi[e]) < 1e-6:
                found.add("ahead")
            if abs(abs(phi[e]) - PI) < 1e-6:
                found.add("astern")
            if abs(abs(phi[e]) - PI / 2) < 1e-6:
                found.add("abeam")
    assert found == {"ahead", "astern", "abeam"}, found
    heads = sorted({round(float(inp["action"][0, a, 2]), 4) for a in range(12) if inp["controlled"][0, a, 0]})
    assert len(heads) == len(HEADS), heads
    return "entities dead ahead, astern and abeam; head angles %s" % heads


REACH_D = (150.0, 190.0, 199.0, 205.0, 230.0, 260.0, 270.0)


def _reach_world():
    """A compact road cluster whose easternmost centre is a long edge segment at x = 20 (bounding radius 20), and agents on a
    line leaving it eastwards, facing it, out to beyond 200 + 20 + 1 m from the box around the road centres."""
    ys = (0.0, 3.1, -2.7, 1.9, -1.4, 0.6, -0.8)
    cars = [car(i, 20.0 + d, y, PI) for i, (d, y) in enumerate(zip(REACH_D, ys))]
    roads = [road(k, ROAD_KINDS[k], [(-20.0 + 4.0 * j, -8.0 + 7.0 * k + 1.2 * math.sin(0.9 * j + k)) for j in range(9)])
             for k in range(3)]
    roads.append(road(3, "road_edge", [(20.0, -20.0), (20.0, 20.0)]))
    return World("reach", cars, roads, moves=[(1, 0.25, -0.15, 0.02), (5, -0.4, 0.3, 0.0)])


def _reach_premise(case, inp, half):
    ents = GR.lidar_entities(inp, 0)
    n = ents["n"]
    cx, cy = ents["cx"][n:], ents["cy"][n:]
    rbmax = float(np.hypot(ents["hx"][n:], ents["hy"][n:]).max())
    far = 200.0 + rbmax + 1.0
    st = inp["state"][0].astype(np.float64)
    dist = np.hypot(np.maximum(np.maximum(cx.min() - st[:n, 0], st[:n, 0] - cx.max()), 0),
                    np.maximum(np.maximum(cy.min() - st[:n, 1], st[:n, 1] - cy.max()), 0))
    assert np.allclose(dist, REACH_D, atol=0.5), dist
    assert dist[3] < far < dist[4], (far, dist)
    face = st[:n, 0] - (ents["cx"][-1] + ents["hy"][-1])   # the long edge runs along y: its near face
    assert 195.0 <= face[2] <= 199.5 and 200.5 <= face[3] <= 205.0, face
    last = GR.lidar_reference(inp, 0, 6, half, ents)
    assert (last["row"] >= n).sum() == 0 and (last["row"] == 5).any(), "the far pair must see each other and no road"
    near = GR.lidar_reference(inp, 0, 2, half, ents)
    assert (near["row"][1] == len(ents["cx"]) - 1).any(), "the agent at 199 m must reach the long edge on plane 1"
    return "box distances %s, far %.2f, near-face distances %.2f / %.2f" % (np.round(dist, 2).tolist(), far, face[2], face[3])


def _ties_world():
    """An agent inside another agent's box, an agent inside a road's bounding circle but outside its box, and twice a lane and a
    road line with identical geometry (once in either order)."""
    cars = [car(0, 0.0, 0.0, 0.2, length=10.0, width=4.0), car(1, 1.0, 0.3, 0.9), car(2, 15.0, 2.0, PI),
            car(3, -14.0, -3.0, -1.5), car(4, 10.0, 0.5, 1.57), car(5, 12.0, -20.0, 1.8, expert=True)]
    top = [(5.0, 8.0), (12.0, 9.5), (19.0, 8.5)]
    bottom = [(5.0, -9.0), (12.0, -10.0), (19.0, -9.5)]
    roads = [road(0, "road_edge", [(-24.0, -6.0), (-4.0, -6.0)]), road(1, "lane", top), road(2, "road_line", top),
             road(3, "road_line", bottom), road(4, "lane", bottom)]
    return World("ties", cars, roads, moves=[(2, 0.25, -0.15, 0.05), (4, -0.2, 0.1, 0.0)])


def _ties_premise(case, inp, half):
    ents = GR.lidar_entities(inp, 0)
    n = ents["n"]

    def inside(o, e):
        lx, ly = GR._to_frame(ents["cx"][o], ents["cy"][o], ents["cx"][e], ents["cy"][e], ents["yaw"][e])
        return abs(lx) < ents["hx"][e] - 0.05 and abs(ly) < ents["hy"][e] - 0.05
    assert inside(1, 0) and inside(0, 1), "agents 0 and 1 must stand inside each other's box"
    for o, e in ((0, 1), (1, 0)):
        assert not (GR.lidar_reference(inp, 0, o, half, ents)["row"] == e).any(), "a box around the origin was hit"
    e = n   # the 20 m edge
    rho = math.hypot(ents["cx"][3] - ents["cx"][e], ents["cy"][3] - ents["cy"][e])
    assert rho < math.hypot(ents["hx"][e], ents["hy"][e]) and not inside(3, e)
    assert (GR.lidar_reference(inp, 0, 3, half, ents)["row"][1] == e).any(), "agent 3 must hit the edge whose circle it is in"
    # rows n+1, n+2: lane; n+3, n+4: the same two boxes as road lines; then road line first, lane second
    assert np.array_equal(ents["type"][n + 1:n + 9], [3, 3, 2, 2, 2, 2, 3, 3])
    for k in ("cx", "cy", "yaw", "hx", "hy"):
        assert np.array_equal(ents[k][n + 1:n + 3], ents[k][n + 3:n + 5]) and np.array_equal(ents[k][n + 5:n + 7], ents[k][n + 7:n + 9])
    tied = {2: 0, 3: 0}
    for a in range(n):
        ref = GR.lidar_reference(inp, 0, a, half, ents)
        hit = ref["row"][2]
        tied[3] += int(((hit == n + 1) | (hit == n + 2)).sum())
        tied[2] += int(((hit == n + 5) | (hit == n + 6)).sum())
        assert not ((hit == n + 3) | (hit == n + 4) | (hit == n + 7) | (hit == n + 8)).any(), "a tie went to the higher row"
    assert tied[2] > 0 and tied[3] > 0, tied
    return "tied returns on plane 2: %d reported as lane, %d as road line" % (tied[3], tied[2])


def _fork128_world():
    """100 live agents in 128 slots (more than one 64-entity batch of agents, the agent / road boundary in mid-batch) and 300
    road segments."""
    rng = np.random.default_rng(5)
    cars = []
    zs = []
    for i in range(100):
        x = (i % 10 - 4.5) * 12.0 + rng.uniform(-3, 3)
        y = (i // 10 - 4.5) * 12.0 + rng.uniform(-3, 3)
        cars.append(car(i, x, y, rng.uniform(-PI, PI), length=rng.uniform(4.0, 5.5), width=rng.uniform(1.8, 2.3),
                        kind=("vehicle", "vehicle", "cyclist", "pedestrian")[i % 4], expert=i % 10 == 7))
        zs.append((1.0, 1.0, 1.0, 0.55, 1.32)[i % 5])
    roads = []
    for r in range(10):
        x, y, th = rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(-PI, PI)
        pts = [(x, y)]
        for _ in range(30):
            th += rng.normal(0.0, 0.25)
            step = rng.uniform(2.0, 6.0)
            x, y = x + step * math.cos(th), y + step * math.sin(th)
            pts.append((x, y))
        roads.append(road(r, ROAD_KINDS[r % 3], pts))
    heads = rng.uniform(-3.0, 3.0, 100)
    return World("fork128", cars, roads, z=zs, heads=heads, moves=[(0, 0.25, -0.15, 0.05), (65, -0.4, 0.3, -0.05)])


def _fork128_premise(case, inp, half):
    n, R = (int(v) for v in inp["shape"][0])
    assert n == 100 and R == 300, (n, R)
    return "100 live agents, 300 roads"


LIDAR_CASES = [
    Case("lidar_heavy_overflow", "lidar", [_heavy_world(False), _heavy_world(True)], [PI, 0.0], premise=_heavy_premise),
    Case("lidar_planes", "lidar", [_planes_world()], [0.0, PI], premise=_planes_premise),
    Case("lidar_reach", "lidar", [_reach_world()], [0.0, PI], premise=_reach_premise),
    Case("lidar_head_wrap", "lidar", [_planes_world("head_wrap")], [0.0, 0.5, PI], premise=_wrap_premise, heads_for=_wrap_heads),
    Case("lidar_inside_and_ties", "lidar", [_ties_world()], [0.0, PI], premise=_ties_premise),
    Case("lidar_fork128", "lidar", [_fork128_world()], [0.0, PI], slots=128, premise=_fork128_premise),
]


# ------------------------------------------------------------------------------------------------------------------
# BEV cases
# ------------------------------------------------------------------------------------------------------------------
def _full_list_world():
    """128 live agents within 30 m of the centre and 270 road segments within 40 m: at radius 50 the central agent's list
    holds 200 roads and 127 partners."""
    cars = []
    for i in range(128):
        r, ang = 29.0 * math.sqrt((i + 0.5) / 128.0), 2.39996323 * i
        cars.append(car(i, r * math.cos(ang) + 0.013, r * math.sin(ang) + 0.029, 0.37 * i, length=3.6 + 0.01 * i,
                        width=1.6 + 0.005 * i, kind=("vehicle", "cyclist", "pedestrian")[i % 3], expert=i % 16 == 5))
    roads = []
    for k in range(9):
        pts = [((4.0 + 34.0 * j / 30.0) * math.cos(0.7 * k + 0.15 * j) + 0.021, (4.0 + 34.0 * j / 30.0) * math.sin(0.7 * k + 0.15 * j) + 0.017)
               for j in range(31)]
        roads.append(road(k, ROAD_KINDS[k % 3], pts))
    return World("full_list", cars, roads, moves=[(0, 0.25, -0.15, 0.05), (64, -0.4, 0.3, -0.05)])


def _full_list_premise(case, inp, radius):
    ref = GR.bev_reference(inp, 0, 0, radius)
    total = int((np.hypot(inp["map_obs"][0, :int(inp["shape"][0, 1]), 0] - inp["state"][0, 0, 0],
                          inp["map_obs"][0, :int(inp["shape"][0, 1]), 1] - inp["state"][0, 0, 1]) <= radius).sum())
    assert ref["n_roads"] == 200 and total >= 260 and ref["n_partners"] == 127, (ref["n_roads"], total, ref["n_partners"])
    return "central agent: %d roads in radius (200 painted), %d partners" % (total, ref["n_partners"])


AXIS_RADII = (20.0, 50.0, 100.0)


def _axes_world():
    """Egos at yaw 0 and pi; for each of the three radii, agents and road segments at yaw 0, +-pi/2, pi centred 0.4 m inside the
    radius at the compass points (their boxes leave the raster) and the diagonals; a 90 m road edge through the middle."""
    cars = [car(0, 0.0, 0.0, 0.0), car(1, 0.13, 0.07, PI, length=4.6, width=2.1)]
    roads = [road(0, "road_edge", segment(3.3, 1.2, 1.45, 45.0))]
    yaws = (0.0, PI / 2, PI, -PI / 2)
    for ri, R in enumerate(AXIS_RADII):
        for k in range(8):
            ang = k * PI / 4
            # (every entity has its own small offset: round distances between them would put centres on cell corners)
            idx = ri * 8 + k
            x, y = (R - 0.4) * math.cos(ang) + 0.031 + 0.0037 * idx, (R - 0.4) * math.sin(ang) + 0.017 + 0.0023 * idx
            if k % 2 == 0 or ri == 1:
                cars.append(car(len(cars), x, y, yaws[(k + ri) % 4], length=4.8, width=2.2,
                                kind=("vehicle", "cyclist")[k % 2]))
            if k % 2 == 1 or ri == 1:
                # (a road is painted with half its half length: 12 m long segments give 6 x 0.2 m rectangles)
                roads.append(road(len(roads), ROAD_KINDS[(k + ri) % 3], segment(x - 0.9, y + 0.6, yaws[(k + 1) % 4], 6.0)))
    return World("axes", cars, roads, moves=[(0, 0.25, -0.15, 0.0), (3, -0.4, 0.3, 0.0)])


def _axes_premise(case, inp, radius):
    out = []
    for a in (0, 1):
        rows, n_roads, _ = GR.bev_entities(inp, 0, a, radius)
        rel = np.abs(((rows[:, 2] + PI / 4) % (PI / 2)) - PI / 4)     # distance of the relative yaw from a multiple of pi / 2
        axis = rel < 1e-6
        over = {side: 0 for side in "WESN"}
        for cx, cy, yaw, length, width, _t in rows:
            hx = abs(math.cos(yaw)) * length / 2 + abs(math.sin(yaw)) * width / 2
            hy = abs(math.sin(yaw)) * length / 2 + abs(math.cos(yaw)) * width / 2
            over["W"] += cx - hx < -radius
            over["E"] += cx + hx > radius - 2 * radius / GR.RES
            over["S"] += cy - hy < -radius
            over["N"] += cy + hy > radius - 2 * radius / GR.RES
        assert axis.sum() >= 8 and all(v > 0 for v in over.values()), (a, int(axis.sum()), over)
        out.append("ego %d: %d axis-aligned rectangles, %s over the border" % (a, int(axis.sum()), over))
    return "; ".join(out)


def _stack_world():
    """Three roads (a lane, a crosswalk, a stop sign) and two partners (a long car, a pedestrian) centred on one point."""
    px, py = 10.13, 5.21
    cars = [car(0, 0.0, 0.0, 0.4), car(1, px, py, 1.1, length=6.0, width=2.6), car(2, px, py, 0.3, length=0.9, width=0.9, kind="pedestrian"),
            car(3, -8.0, 3.0, 2.0, kind="cyclist", length=1.8, width=0.7)]
    roads = [road(0, "lane", segment(px, py, 2.2, 8.0)),
             road(1, "crosswalk", [(px - 6.0, py - 4.0), (px + 6.0, py - 4.0), (px + 6.0, py + 4.0), (px - 6.0, py + 4.0)]),
             road(2, "stop_sign", [(px, py)])]
    return World("stack", cars, roads, moves=[(0, 0.25, -0.15, 0.05), (3, -0.4, 0.3, 0.0)])


def _stack_premise(case, inp, radius):
    rows, n_roads, _ = GR.bev_entities(inp, 0, 0, radius)
    assert n_roads == 3 and len(rows) == 6, (n_roads, len(rows))
    assert [int(t) for t in rows[:, 5]] == [3, 4, 6, 7, 8, 9], rows[:, 5]
    assert np.ptp(rows[:5, 0]) < 1e-4 and np.ptp(rows[:5, 1]) < 1e-4, "the five entities must share a centre"
    grid = GR.bev_reference(inp, 0, 0, radius)["grid"]
    cell = 2 * radius / GR.RES
    gx, gy = int((rows[0, 0] + radius) / cell), int((rows[0, 1] + radius) / cell)
    assert grid[gy, gx] == 8, "the centre cell must show the last entity in the paint order (the pedestrian)"
    seen = set(np.unique(grid).tolist())
    assert {3, 4, 7, 8} <= seen and 6 not in seen, "ring cells must show lane, crosswalk, car; the stop sign lies under the partners: %s" % seen
    return "centre cell shows 8; types in the raster %s" % sorted(seen)


BEV_CASES = [
    Case("bev_full_list", "bev", [_full_list_world()], [50.0], slots=128, rasters=[[0, 1, 17, 40, 63, 64, 100, 127]],
         premise=_full_list_premise),
    Case("bev_axes_and_border", "bev", [_axes_world()], list(AXIS_RADII), rasters=[[0, 1, 2, 5, 9, 14]], premise=_axes_premise),
    # (the rasters of the two stacked partners are not used: each sees the other centred exactly on a cell corner)
    Case("bev_stack", "bev", [_stack_world()], [50.0, 20.0], rasters=[[0, 3]], premise=_stack_premise),
]

CASES = {c.name: c for c in LIDAR_CASES + BEV_CASES}


# ------------------------------------------------------------------------------------------------------------------
# comparison with the reference
# ------------------------------------------------------------------------------------------------------------------
def compare_lidar_to_reference(sim, half, what, worlds=None):
    """Every live agent's returns against lidar_reference of the simulator's own tensors: outside the margin mask hit / miss and
    type exact.  Returns dict(share = the masked share of rays per plane [3], depth = the largest depth / hit position
    difference on the compared hit rays, rays)."""
    inp = GR.read_inputs(sim)
    got = GR._np(sim.lidar_tensor()).astype(np.float64)
    masked = np.zeros(3)
    total = 0
    depth = 0.0
    for w in (range(inp["shape"].shape[0]) if worlds is None else worlds):
        ents = GR.lidar_entities(inp, w)
        for a in range(ents["n"]):
            ref = GR.lidar_reference(inp, w, a, half, ents)
            g, r, ok = got[w, a], ref["out"], ~ref["margin"]
            masked += ref["margin"].sum(axis=1)
            total += GR.N_RAYS
            bad = ok & (((g[..., 0] > 0) != (r[..., 0] > 0)) | (g[..., 1] != r[..., 1]))
            if bad.any():
                p, idx = np.argwhere(bad)[0]
                raise AssertionError("%s: world %d agent %d: %d non-marginal rays differ from the reference; first plane %d ray %d: "
                                     "got %s, reference %s (entity row %d)" %
                                     (what, w, a, int(bad.sum()), p, idx, g[p, idx].tolist(), r[p, idx].tolist(), ref["row"][p, idx]))
            both = ok & (r[..., 0] > 0)
            if both.any():
                depth = max(depth, float(np.abs(g[both][:, [0, 2, 3]] - r[both][:, [0, 2, 3]]).max()))
    return dict(share=masked / max(total, 1), depth=depth, rays=total)


def compare_bev_to_reference(sim, radius, what, rasters):
    """The listed rasters [(world, agent), ...] against bev_reference of the simulator's own tensors: every cell outside the
    margin mask exact.  Returns dict(cells, painted, masked, masked_painted)."""
    inp = GR.read_inputs(sim)
    got = GR._np(sim.bev_observation_tensor())
    out = dict(cells=0, painted=0, masked=0, masked_painted=0)
    for w, a in rasters:
        ref = GR.bev_reference(inp, w, a, radius)
        assert ref["usable"], "%s: world %d agent %d: a discrete decision of this raster sits on a knife edge" % (what, w, a)
        g = got[w, a, :, :, 0].astype(np.int64)
        bad = (g != ref["grid"]) & ~ref["margin"]
        if bad.any():
            y, x = np.argwhere(bad)[0]
            raise AssertionError("%s: world %d agent %d: %d non-marginal cells differ from the reference; first (x %d, y %d): got %d, "
                                 "reference %d" % (what, w, a, int(bad.sum()), x, y, g[y, x], ref["grid"][y, x]))
        out["cells"] += g.size
        out["painted"] += int((ref["grid"] != 0).sum())
        out["masked"] += int(ref["margin"].sum())
        out["masked_painted"] += int((ref["margin"] & (ref["grid"] != 0)).sum())
    return out


def marginal_differences(sim_a, sim_b, case, variant):
    """For a failure text: where two simulators differ, and whether the reference calls those elements marginal."""
    inp = GR.read_inputs(sim_b)
    lines = []
    if case.kind == "lidar":
        a, b = GR._np(sim_a.lidar_tensor()), GR._np(sim_b.lidar_tensor())
        for w in range(len(case.worlds)):
            for ag in range(case.worlds[w].n):
                d = ((a[w, ag, ..., 0] > 0) != (b[w, ag, ..., 0] > 0)) | (a[w, ag, ..., 1] != b[w, ag, ..., 1])
                if d.any():
                    m = GR.lidar_reference(inp, w, ag, variant)["margin"]
                    lines.append("world %d agent %d: %d rays differ, %d of them marginal" % (w, ag, int(d.sum()), int((d & m).sum())))
    else:
        a, b = GR._np(sim_a.bev_observation_tensor()), GR._np(sim_b.bev_observation_tensor())
        for w in range(len(case.worlds)):
            for ag in range(case.worlds[w].n):
                d = a[w, ag, :, :, 0] != b[w, ag, :, :, 0]
                if d.any():
                    m = GR.bev_reference(inp, w, ag, variant)["margin"]
                    lines.append("world %d agent %d: %d cells differ, %d of them marginal" % (w, ag, int(d.sum()), int((d & m).sum())))
    return "; ".join(lines)
