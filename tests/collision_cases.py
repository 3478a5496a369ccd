"""Constructed worlds for the collision reference (tests/collision_reference.py): each case aims the geometry at one piece of
the collision phase of k_world_step that the Waymo scenes never reach -- the host-built broadphase grid (cell listing, reach,
pad, "off the grid", wide cells, no grid at all), the item list with its scan, owner search and trips, the type filter, the
activity rules, the narrowphase close to touching -- and asserts its own premise FROM THE REFERENCE'S GEOMETRY so that it
cannot quietly stop exercising that piece.

Scenes are built with the helpers of tests/geom_cases.py; every agent stands still in its log.  All cases:
polylineReductionThreshold = 0, initOnlyValidAgentsAtFirstStep = 0 (agents whose log is invalid exist), isStaticAgentControlled
= 0 (an agent whose goal is where it stands is parked: Static).  Road rows: every polyline has two points and every other road
one box, so road row r of map_observation_tensor is road r of the scene.

MARGIN BAND.  The separating-axis test is ill-conditioned in float32 far from the origin: the minor axis of a 0.2 m wide
segment is a difference of two corners rounded at the ulp of the coordinate.  tests/test_collision_reference.py sweeps
near-touching pairs of the cases' own box shapes (gaps 1e-6 ... 1e-1 m of either sign) over each span through the oracle's obb_collide
and records below the largest |separation| at which the float32 verdict differs from float64.  A case's band is
GPU_BAND_FACTOR times the figure of its span -- the factor of GC.GPU_DEPTH_FACTOR, for the same reason: the device's sincos /
reciprocal differ from the host's by about an ulp -- and never a figure taken from the kernel's output."""
import math

import numpy as np

from tests import collision_reference as CR
from tests import geom_cases as GC
from tests import geom_reference as GR
from tests import parity as P

f32 = np.float32
PI = GC.PI

# span (coordinates within +- span metres): the largest |separation| at which oracle_mod.obb_collide and float64 disagree,
# measured by test_the_oracles_narrowphase_flips_only_inside_the_recorded_band (20,000 pairs per span: car boxes against car
# boxes and against 0.1 m half-width segments up to 80 m long; a tenth to a fifth of them flip).  Measured: 1.11e-3, 4.79e-3,
# 7.94e-3 and 1.87e-2 m; the constants are those figures rounded up.
ORACLE_FLIP_MAX = {150.0: 1.2e-3, 400.0: 4.8e-3, 600.0: 8.0e-3, 1500.0: 1.9e-2}
GPU_BAND_FACTOR = 2.0
AIMED_FACTOR = 4.0            # every aimed pair keeps |sep| >= AIMED_FACTOR * band
MARGIN_AGENTS = 1e-2          # share of a case's agents that may be marginal at all (a condition, not a measurement)
SVCAP = 1536                  # (agent, candidate) items per trip of the kernel's road-box phase


def band_of(span):
    return GPU_BAND_FACTOR * ORACLE_FLIP_MAX[span]


# ------------------------------------------------------------------------------------------------------------------
# scene building
# ------------------------------------------------------------------------------------------------------------------
def parked(i, x, y, yaw, **kw):
    """A car whose goal is where it stands: Static, nobody controls it, done from its first step on."""
    c = GC.car(i, x, y, yaw, **kw)
    c["goalPosition"] = {"x": float(x), "y": float(y), "z": 0.0}
    return c


def ghost(i, x, y, yaw, **kw):
    """An expert whose log is invalid at every step."""
    c = GC.car(i, x, y, yaw, expert=True, **kw)
    c["valid"] = [False] * 91
    return c


def box4(cx, cy, ang, half_l, half_w):
    """The four corners of a crosswalk / speed bump."""
    c, s = math.cos(ang), math.sin(ang)
    return [(cx + sx * half_l * c - sy * half_w * s, cy + sx * half_l * s + sy * half_w * c)
            for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


class Case:
    def __init__(self, name, worlds, span, premise, slots=64, goal_threshold=0.0):
        self.name, self.worlds, self.span, self.premise, self.slots = name, worlds, span, premise, slots
        self.band = band_of(span)
        self.goal_threshold = goal_threshold
        self.heads_for = None
        for wd in worlds:
            assert wd.n <= min(slots, 128) and len(wd.scene["roads"]) <= 400 and len(wd.moves) == 2, name
            assert all(len(r["geometry"]) in (1, 2, 4) for r in wd.scene["roads"])

    write = GC.Case.write

    def params(self, behaviour=2, model=0):
        return dict(polylineReductionThreshold=0.0, collisionBehaviour=behaviour, dynamicsModel=model, observationRadius=50.0,
                    initOnlyValidAgentsAtFirstStep=0, isStaticAgentControlled=0, rewardType=1,
                    distanceToGoalThreshold=self.goal_threshold)


def _aimed_ok(case, ref, pairs, what):
    """Every aimed (agent, entity row) pair is looked at and keeps |sep| >= 4 bands."""
    for a, e in pairs:
        assert abs(ref["sep"][a, e]) >= AIMED_FACTOR * case.band, "%s: aimed pair (%d, %d) has |sep| %.3g < %.3g" % \
            (what, a, e, abs(ref["sep"][a, e]), AIMED_FACTOR * case.band)


def _circles(ref):
    """[n, E] bool: the float64 bounding circles of agent and entity overlap."""
    e = ref["ents"]
    n = e["n"]
    rad = np.hypot(e["hx"], e["hy"])
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.hypot(e["cx"][:n, None] - e["cx"][None, :], e["cy"][:n, None] - e["cy"][None, :])
    return d <= rad[:n, None] + rad[None, :]


def grid_of(ref):
    """The broadphase grid's origin, cell and pad restated in float64 from the boxes (road edges and stop signs) and the
    agents' sizes: cells of max(16, extent / 64) m, the box centres' bounding box grown by (largest agent radius + largest
    box radius) * 1.002 + 0.05.  None when the world has no box."""
    e = ref["ents"]
    n = e["n"]
    box = np.nonzero((e["type"][n:] == CR.ET_ROAD_EDGE) | (e["type"][n:] == CR.ET_STOP_SIGN))[0] + n
    if len(box) == 0:
        return None
    rad = np.hypot(e["hx"], e["hy"])
    pad = (rad[:n].max() + rad[box].max()) * 1.002 + 0.05
    x0, x1, y0, y1 = e["cx"][box].min() - pad, e["cx"][box].max() + pad, e["cy"][box].min() - pad, e["cy"][box].max() + pad
    cell = max(16.0, max(x1 - x0, y1 - y0) / 64.0)
    return dict(ox=x0, oy=y0, x1=x1, y1=y1, cell=cell, pad=pad, boxes=box, reach=rad[:n].max() + rad[box].max())


# ------------------------------------------------------------------------------------------------------------------
# coll_far_cells
# ------------------------------------------------------------------------------------------------------------------
FAR_LENGTHS = (70.0, 68.0, 66.0, 70.0, 68.0, 66.0, 70.0, 68.0, 40.0, 55.0)


FAR_BUS_R = 0.7 * math.hypot(11.0, 1.5)


def _far_world():
    """Ten road-edge segments 40-70 m long, about 110 m apart; segment k points in compass direction k * 45 degrees (+ 0.07
    rad).  Around each: a car over either tip, one over the flank at 0.9 of the half length, and two aligned cars 0.5 m off the
    flanks.  A 22 x 3 m bus far from everything fixes the largest agent radius (7.8 m), and with it how far from its centre a
    box is listed.  Two short edges at the corners fix the grid (16 m cells); every segment is then shifted by less than a cell
    until the cell under the car on its first tip lies WHOLLY farther from the segment's centre than the segment's own radius:
    that cell lists the segment only because the reach counts the agent's radius in."""
    cars = [GC.car(0, 0.0, -160.0, 0.3, length=22.0, width=3.0)]
    roads = [GC.road(0, "road_edge", GC.segment(-300.0, -140.0, 0.5, 2.0)), GC.road(1, "road_edge", GC.segment(300.0, 140.0, 2.5, 2.0))]
    pad = (FAR_BUS_R + math.hypot(35.0, 0.1)) * 1.002 + 0.05
    ox, oy = -300.0 - pad, -140.0 - pad
    assert (600.0 + 2 * pad) / 64.0 < 16.0
    for k, length in enumerate(FAR_LENGTHS):
        ang, h = k * PI / 4 + 0.07, length / 2
        ux, uy, nx, ny = math.cos(ang), math.sin(ang), -math.sin(ang), math.cos(ang)
        found = None
        for sx in np.arange(0.0, 16.0, 0.25):
            for sy in np.arange(0.0, 16.0, 0.25):
                cx, cy = (k % 5 - 2) * 110.0 + 3.7 * k + sx, (k // 5) * 110.0 - 55.0 + sy
                px, py = cx + (h + 0.9) * ux, cy + (h + 0.9) * uy
                qx, qy = ox + math.floor((px - ox) / 16.0) * 16.0, oy + math.floor((py - oy) / 16.0) * 16.0
                near = math.hypot(min(max(cx, qx), qx + 16.0) - cx, min(max(cy, qy), qy + 16.0) - cy)
                if found is None and near > math.hypot(h, 0.1) * 1.002 + 0.05 + 0.3:
                    found = (cx, cy)
        cx, cy = found
        roads.append(GC.road(k + 2, "road_edge", GC.segment(cx, cy, ang, h)))
        for along, off, yaw in ((h + 0.9, 0.0, ang), (-(h + 0.9), 0.0, ang + 0.4), (0.9 * h, 0.5, ang + 1.0),
                                (-0.9 * h, 1.3, ang), (0.5 * h, -1.3, ang + PI)):
            cars.append(GC.car(len(cars), cx + along * ux + off * nx, cy + along * uy + off * ny, yaw))
    # car 1 leaves segment 0's tip; car 9 (segment 1's clear flank car) drives onto segment 1
    n1 = (-math.sin(PI / 4 + 0.07), math.cos(PI / 4 + 0.07))
    return GC.World("far_cells", cars, roads, moves=[(1, 2.5 * math.cos(0.07), 2.5 * math.sin(0.07), 0.0),
                                                     (9, -1.0 * n1[0], -1.0 * n1[1], 0.0)])


def _far_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    g = grid_of(ref)
    assert np.hypot(e["hx"][0], e["hy"][0]) > 7.7 and g["cell"] == 16.0, "the bus must fix the largest agent radius; cells of 16 m"
    dist = np.hypot(e["cx"][:n, None] - e["cx"][None, n:], e["cy"][:n, None] - e["cy"][None, n:])
    hit = ref["pairs"][:, n:] & (ref["sep"][:, n:] <= 0)
    far = hit & (dist > 32.0)
    octants, beyond = set(), 0
    for a, r in np.argwhere(far):
        octants.add(int(np.floor((math.atan2(e["cy"][a] - e["cy"][n + r], e["cx"][a] - e["cx"][n + r]) + PI / 8) / (PI / 4))) % 8)
        # the cell under the agent's centre, and the point of it nearest the box's centre
        qx = g["ox"] + np.floor((e["cx"][a] - g["ox"]) / 16.0) * 16.0
        qy = g["oy"] + np.floor((e["cy"][a] - g["oy"]) / 16.0) * 16.0
        near = math.hypot(min(max(e["cx"][n + r], qx), qx + 16.0) - e["cx"][n + r], min(max(e["cy"][n + r], qy), qy + 16.0) - e["cy"][n + r])
        beyond += near > math.hypot(e["hx"][n + r], e["hy"][n + r]) * 1.002 + 0.05 + 0.1
    near = ref["pairs"][:, n:] & (ref["sep"][:, n:] > 0) & _circles(ref)[:, n:]
    assert far.sum() >= 8 and len(octants) == 8 and near.sum() >= 8, (int(far.sum()), sorted(octants), int(near.sum()))
    assert beyond >= 8, "only %d colliding agents stand in a cell wholly beyond the box's own radius" % beyond
    _aimed_ok(case, ref, [(a, n + r) for a, r in np.argwhere(far | near)], case.name)
    long = e["hx"][n + 2:]
    assert 40.0 - 1e-3 <= 2 * long.min() and 2 * long.max() <= 70.0 + 1e-3
    return "%d colliding (vehicle, edge) pairs with centre distance > 32 m (largest %.1f), in %d compass directions, %d of them " \
        "in a cell wholly beyond the edge's own radius; %d clear pairs with overlapping circles" % \
        (far.sum(), dist[far].max(), len(octants), beyond, near.sum())


# ------------------------------------------------------------------------------------------------------------------
# coll_grid_border
# ------------------------------------------------------------------------------------------------------------------
BORDER_R = 0.7 * math.hypot(2.0, 1.0) + math.hypot(30.0, 0.1)   # largest agent radius + largest box radius


def _border_world():
    """A ring of four 60 m road edges at x, y = +-40 (the box centres' bounding box is [-40, 40]^2) and two short ones inside.
    Cars 0-3 overlap the ring from outside that bounding box; cars 4-11 stand 1 m inside and 1 m outside the line
    +-(40 + largest agent radius + largest box radius) on every side; cars 12, 13 are 500 m out; 14 is clear of, 15 on an
    inner edge."""
    roads = [GC.road(0, "road_edge", GC.segment(-40.0, 0.0, PI / 2, 30.0)), GC.road(1, "road_edge", GC.segment(40.0, 0.0, PI / 2, 30.0)),
             GC.road(2, "road_edge", GC.segment(0.0, -40.0, 0.0, 30.0)), GC.road(3, "road_edge", GC.segment(0.0, 40.0, 0.0, 30.0)),
             GC.road(4, "road_edge", GC.segment(5.0, 6.0, 0.3, 6.0)), GC.road(5, "road_edge", GC.segment(-8.0, -9.0, 1.9, 5.0))]
    cars = [GC.car(0, -40.9, 11.0, 0.0), GC.car(1, 40.9, -7.0, 0.2), GC.car(2, 9.0, -40.8, PI / 2), GC.car(3, -13.0, 40.8, 1.4)]
    for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        for d in (-1.0, 1.0):
            r = 40.0 + BORDER_R + d
            cars.append(GC.car(len(cars), sx * r + 3.0 * sy, sy * r + 3.0 * sx, 0.5 * len(cars)))
    cars += [GC.car(12, 540.0, 2.0, 0.3), GC.car(13, -1.0, -540.0, 2.0)]
    cars += [GC.car(14, 5.0, 9.5, 0.3), GC.car(15, -8.0, -9.0, 0.4)]
    return GC.World("grid_border", cars, roads, moves=[(14, 3.0 * math.sin(0.3), -3.0 * math.cos(0.3), 0.0), (0, -3.0, 0.0, 0.0)])


def _border_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    g = grid_of(ref)
    bx0, bx1, by0, by1 = e["cx"][g["boxes"]].min(), e["cx"][g["boxes"]].max(), e["cy"][g["boxes"]].min(), e["cy"][g["boxes"]].max()
    x, y = e["cx"][:n], e["cy"][:n]
    outside = (x < bx0) | (x > bx1) | (y < by0) | (y > by1)
    assert outside[:4].all() and ref["collided"][:4].all() and (ref["info"][:4, 0] == 1).all(), "cars 0-3 collide from outside"
    sides = [bool(x[0] < bx0), bool(x[1] > bx1), bool(y[2] < by0), bool(y[3] > by1)]
    assert all(sides), sides
    # 1 m inside / outside the line (box centres' bounding box grown by agent radius + box radius), on all four sides
    lim = np.maximum(np.maximum(bx0 - x, x - bx1), np.maximum(by0 - y, y - by1)) - g["reach"]
    assert np.allclose(lim[4:12], [-1, 1] * 4, atol=0.05), lim[4:12]
    beyond = np.nonzero((x < g["ox"]) | (x > g["x1"]) | (y < g["oy"]) | (y > g["y1"]))[0]
    assert len(beyond) >= 6 and {12, 13} <= set(beyond.tolist()), beyond
    assert not (_circles(ref)[beyond][:, n:]).any(), "an agent off the grid has a road within its circle"
    assert max(abs(x[12] - bx1), abs(y[13] - by0)) > 490.0
    _aimed_ok(case, ref, [(a, n + a) for a in range(4)] + [(15, n + 5)], case.name)
    return "cars 0-3 collide from outside the box centres' bounding box; %d agents off the grid (pad %.2f m), none with a " \
        "road in its circle; two of them ~500 m out" % (len(beyond), g["pad"])


# ------------------------------------------------------------------------------------------------------------------
# coll_wide_world
# ------------------------------------------------------------------------------------------------------------------
WIDE_HALF = 20.0     # the anchor segments: the longest boxes of the world
WIDE_SITES = [(2, 3, 0), (4, 9, 1), (6, 14, 0), (8, 20, 1), (3, 27, 0), (7, 6, 1), (5, 17, 0), (9, 24, 1),
              (62, 4, 1), (60, 10, 0), (58, 15, 1), (56, 21, 0), (61, 28, 1), (57, 7, 0), (59, 18, 1), (55, 25, 0),
              (30, 12, 0), (34, 16, 1), (31, 22, 0), (33, 8, 1)]


def _wide_world():
    """Two 40 m anchor edges at (-1200, -600) and (1200, 600) fix the grid: extent 2400 m + pads, cells of extent / 64 = 38 m.
    At 20 sites -- corners (i, j) of that grid, and points on a cell boundary half a cell further up -- a 24 m edge passes
    through and a car stands on the site: squarely on the edge, or aligned with it 0.6 m off its flank."""
    pad = (0.7 * math.hypot(2.0, 1.0) + math.hypot(WIDE_HALF, 0.1)) * 1.002 + 0.05
    ox, oy = -1200.0 - pad, -600.0 - pad
    cell = (2400.0 + 2 * pad) / 64.0
    roads = [GC.road(0, "road_edge", GC.segment(-1200.0, -600.0, 0.4, WIDE_HALF)), GC.road(1, "road_edge", GC.segment(1200.0, 600.0, 2.0, WIDE_HALF))]
    cars = []
    for k, (i, j, clear) in enumerate(WIDE_SITES):
        px, py = ox + i * cell, oy + (j + (0.5 if k % 4 == 3 else 0.0)) * cell
        ang = 0.35 + 0.61 * k
        nx, ny = -math.sin(ang), math.cos(ang)
        off = 0.1 + 0.7 + 0.6 if clear else 0.25
        roads.append(GC.road(len(roads), "road_edge", GC.segment(px - off * nx, py - off * ny, ang, 12.0)))
        cars.append(GC.car(k, px, py, ang if clear else ang + 0.9))
    n0, n1 = (-math.sin(0.35), math.cos(0.35)), (-math.sin(0.96), math.cos(0.96))
    return GC.World("wide_world", cars, roads, moves=[(0, 3.0 * n0[0], 3.0 * n0[1], 0.0), (1, -1.2 * n1[0], -1.2 * n1[1], 0.0)])


def _wide_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    g = grid_of(ref)
    extent = max(np.ptp(e["cx"][g["boxes"]]), np.ptp(e["cy"][g["boxes"]]))
    assert extent > 1100.0 and g["cell"] > 16.0, (extent, g["cell"])
    fx, fy = (e["cx"][:n] - g["ox"]) / g["cell"], (e["cy"][:n] - g["oy"]) / g["cell"]
    on_x, on_y = np.abs(fx - np.rint(fx)) < 1e-3, np.abs(fy - np.rint(fy)) < 1e-3
    assert on_x.all() and on_y.sum() >= 12 and (~on_y).sum() >= 4, "agents must sit on cell corners and cell boundaries"
    far = np.abs(e["cx"][:n]) > 800.0
    own = ref["sep"][np.arange(n), n + 2 + np.arange(n)]
    hit, clear = (own <= 0) & far, (own > 0) & far
    assert hit.sum() >= 6 and clear.sum() >= 6, (int(hit.sum()), int(clear.sum()))
    assert (own[own > 0] >= 0.5).all() and np.array_equal(ref["collided"], own <= 0)
    _aimed_ok(case, ref, [(a, n + 2 + a) for a in range(n)], case.name)
    return "edge centres span %.0f m, cells of %.2f m; %d agents on cell corners, %d on cell boundaries; beyond +-800 m %d " \
        "colliding and %d clear (gaps >= %.2f m)" % (extent, g["cell"], on_y.sum(), (~on_y).sum(), hit.sum(), clear.sum(), own[own > 0].min())


# ------------------------------------------------------------------------------------------------------------------
# coll_crowd
# ------------------------------------------------------------------------------------------------------------------
STRIPES = (-6.0, -3.6, -1.2, 1.2, 3.6, 6.0)
LANES = (-4.8, -2.4, 0.0, 2.4, 4.8)
LANE_X = (-4.5, -1.5, 1.5, 4.5)


def _crowd_world(slots):
    """Every slot live, all within a 12 m patch: slot % 4 = 0 parked (Static), 1 vehicle, 2 pedestrian, 3 an expert whose log
    is invalid -- so slots 0, 63, 64 and the last one have no candidates and sit between agents with many.  240 road edges of
    10 m lie in six stripes 2.4 m apart; 3 stop signs stand in the lanes between them.  Two vehicles in three stand aligned
    in a lane (clear of the stripes by 0.6 m), the third is turned across a stripe; most parked cars stand along a stripe (on
    top of each other: Static pairs), the others, the pedestrians and the invalid experts are scattered over everything.  A
    scattered agent is drawn again while its box lies within 5 cm of touching any other box."""
    rng = np.random.default_rng(slots)
    roads = []
    for k in range(240):
        roads.append(GC.road(k, "road_edge", GC.segment(rng.uniform(-1.8, 1.8), STRIPES[k % 6], rng.uniform(-0.008, 0.008), 5.0)))
    signs = [(-3.0, 2.4), (0.0, -2.4), (3.0, 4.8)]
    for x, y in signs:
        roads.append(GC.road(len(roads), "stop_sign", [(x, y)]))
    rects = [[0.5 * (r["geometry"][0][k] + r["geometry"][-1][k]) for k in ("x", "y")] for r in roads]
    rects = [(x, y, math.atan2(r["geometry"][-1]["y"] - r["geometry"][0]["y"], r["geometry"][-1]["x"] - r["geometry"][0]["x"]) if i < 240 else 0.0,
              5.0 if i < 240 else 0.2, 0.1 if i < 240 else 0.2) for i, ((x, y), r) in enumerate(zip(rects, roads))]
    # slots 1 and 5 (65 in the second wave) are the step pass's: nothing is scattered within 2.6 m of where they stand / go
    mover2 = 5 if slots == 64 else 65
    first = (-4.5, -4.8)
    keep = [first, (0.0, 1.2), (0.0, 2.4)]
    sites = [(x, y) for y in LANES for x in LANE_X if (x, y) != first and not (y == 2.4 and abs(x) == 1.5)]
    sites = [sites[k] for k in rng.permutation(len(sites))]
    per_wave = len(sites) // (slots // 64)

    lane_cars = []

    def free(x, y, yaw, hx, hy, off_lanes):
        if not all(math.hypot(x - kx, y - ky) > 2.6 for kx, ky in keep):
            return False
        if off_lanes and (CR.separation((x, y, yaw, hx, hy), np.asarray(lane_cars).T) < 0.05).any():
            return False
        return bool((np.abs(CR.separation((x, y, yaw, hx, hy), np.asarray(rects).T)) > 0.05).all())

    def scattered(hx, hy, y=None, yaw=None, off_lanes=False):
        while True:
            pose = (rng.uniform(-5.6, 5.6), rng.uniform(-5.6, 5.6) if y is None else y(rng), rng.uniform(-PI, PI) if yaw is None else yaw(rng))
            if free(*pose, hx, hy, off_lanes):
                return pose

    # the agents whose place is given come first, so that every scattered one is tested against them
    poses = {1: (first[0], first[1], 0.0), mover2: (0.0, 1.2, 0.0)}   # (mover2: squarely on a stripe, the lane above it free)
    n_veh = 0
    for i in range(1, slots, 4):
        if i not in poses and n_veh % 3 != 2 and len(sites) > per_wave * (slots // 64 - 1 - i // 64):
            poses[i] = sites.pop() + ((0.0, PI)[n_veh % 2],)
            lane_cars.append(poses[i] + (0.7 * 1.5, 0.7 * 0.7))
        n_veh += 1
    for i in range(2, slots, 16):
        poses[i] = (signs[(i // 16) % 3][0], signs[(i // 16) % 3][1] - 0.15, 0.0)
    for i, (x, y, yaw) in poses.items():
        rects.append((x, y, yaw) + ((0.315, 0.315) if i % 4 == 2 else (1.05, 0.49)))
    assert (np.abs(CR.separation([np.asarray(rects)[:, None, k] for k in range(5)], [np.asarray(rects)[None, :, k] for k in range(5)])
                   + 10.0 * np.eye(len(rects))) > 0.05).all(), "a given place lies within 5 cm of touching another"
    cars = []
    for i in range(slots):
        kind = i % 4
        length, width, what = (0.9, 0.9, "pedestrian") if kind == 2 else (3.0, 1.4, "vehicle")
        hx, hy = 0.7 * length / 2, 0.7 * width / 2
        if i in poses:
            x, y, yaw = poses[i]
        else:
            if kind == 1:        # turned across a stripe, clear of the cars in the lanes
                x, y, yaw = scattered(hx, hy, yaw=lambda r: r.uniform(0.5, 2.6), off_lanes=True)
            elif kind == 2 and i % 16 != 6:     # along a stripe: clear of the cars in the lanes, over the parked ones
                x, y, yaw = scattered(hx, hy, y=lambda r: min(max(STRIPES[r.integers(0, 6)] + r.uniform(-0.2, 0.2), -6.0), 6.0))
            elif kind == 0 and i % 16 != 0:
                x, y, yaw = scattered(hx, hy, y=lambda r: STRIPES[i // 4 % 6], yaw=lambda r: 0.0)
            else:
                x, y, yaw = scattered(hx, hy)
            if kind != 3:    # (an invalid expert touches nothing)
                rects.append((x, y, yaw, hx, hy))
        make = (parked, GC.car, GC.car, ghost)[kind]
        cars.append(make(i, x, y, yaw, length=length, width=width, kind=what))
    return GC.World("crowd%d" % slots, cars, roads, moves=[(1, 0.0, 1.1, 0.0), (mover2, 0.0, 1.2, 0.0)])


def _crowd_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    slots = case.slots
    assert n == slots
    g = grid_of(ref)
    assert len(g["boxes"]) == 243 and (e["type"][n:] == CR.ET_STOP_SIGN).sum() == 3
    assert np.ptp(e["cx"][:n]) <= 12.001 and np.ptp(e["cy"][:n]) <= 12.001, "all agents within one 12 m patch"
    owners = ref["active"] & ~ref["static"]          # the agents whose cell's boxes go on the item list
    items = int((_circles(ref)[:, g["boxes"]] & owners[:, None]).sum())
    trips = 3 if slots == 64 else 4
    assert items > (trips - 1) * SVCAP, "%d (agent, box) pairs pass the circle test: not more than %d trips' worth" % (items, trips - 1)
    none = ~owners
    assert none[0] and none[63] and none[n - 1] and (slots == 64 or none[64]) and owners[1] and owners[n - 2]
    veh = (e["type"][:n] == CR.ET_VEHICLE) & owners
    waves = []
    for w0 in range(0, n, 64):
        sl = slice(w0, w0 + 64)
        hit, clear = int((veh[sl] & ref["collided"][sl]).sum()), int((veh[sl] & ~ref["collided"][sl]).sum())
        assert hit >= 2 and clear >= 2, "wave %d: %d colliding and %d clear vehicles" % (w0 // 64, hit, clear)
        waves.append("%d / %d" % (hit, clear))
    ped_sign = ref["pairs"] & (ref["sep"] <= 0) & (e["type"][:n, None] == CR.ET_PEDESTRIAN) & (e["type"][None, :] == CR.ET_STOP_SIGN)
    assert ped_sign.any(), "no pedestrian stands on a stop sign"
    movers = [a for a, _, _, _ in case.worlds[0].moves]
    assert not ref["collided"][movers[0]] and ref["collided"][movers[1]] and ref["info"][movers[1]].tolist() == [1, 0, 0]
    return "%d (agent, box) pairs pass the circle test (> %d x %d: >= %d trips); colliding / clear vehicles per wave %s; " \
        "%d pedestrians on stop signs" % (items, trips - 1, SVCAP, trips, ", ".join(waves), ped_sign.any(1).sum())


# ------------------------------------------------------------------------------------------------------------------
# coll_types
# ------------------------------------------------------------------------------------------------------------------
AGENT_KINDS = (("vehicle", 4.0, 2.0), ("cyclist", 1.8, 0.7), ("pedestrian", 0.9, 0.9))
ROAD_KINDS = ("road_edge", "road_line", "lane", "crosswalk", "speed_bump", "stop_sign")
TYPE_OF = dict(vehicle=CR.ET_VEHICLE, cyclist=CR.ET_CYCLIST, pedestrian=CR.ET_PEDESTRIAN, road_edge=CR.ET_ROAD_EDGE,
               road_line=CR.ET_ROAD_LINE, lane=CR.ET_ROAD_LANE, crosswalk=CR.ET_CROSSWALK, speed_bump=CR.ET_SPEED_BUMP,
               stop_sign=CR.ET_STOP_SIGN)


def _types_world(name="types"):
    """Agents 0-17: each of vehicle / cyclist / pedestrian squarely on each of the six road kinds, 25 m apart (road row k under
    agent k).  Agent 18, a vehicle, overlaps a vehicle (19), a pedestrian (20), a cyclist (21) and road edge 18 at once.
    Agent 22 stands beside a stop sign (road 19), clear."""
    cars, roads = [], []
    for k in range(18):
        kind, length, width = AGENT_KINDS[k // 6]
        rk = ROAD_KINDS[k % 6]
        x, y, ang = (k % 6 - 2.5) * 25.0 + 0.3 * k, (k // 6 - 1) * 25.0, 0.2 + 0.37 * k
        if rk in ("crosswalk", "speed_bump"):
            pts = box4(x, y, ang, 3.0, 1.5)
        elif rk == "stop_sign":
            pts = [(x, y)]
        else:
            pts = GC.segment(x, y, ang, 3.0)
        roads.append(GC.road(k, rk, pts))
        cars.append(GC.car(k, x + 0.05, y - 0.04, ang + 0.6, length=length, width=width, kind=kind))
    hx, hy = 0.0, 55.0
    cars.append(GC.car(18, hx, hy, 0.0))                                            # box 2.8 x 1.4
    cars.append(GC.car(19, hx + 2.4, hy + 0.3, 0.5))                                # a vehicle over its nose
    cars.append(GC.car(20, hx - 1.5, hy + 0.2, 0.3, length=0.9, width=0.9, kind="pedestrian"))
    cars.append(GC.car(21, hx - 0.3, hy + 0.8, 0.1, length=1.8, width=0.7, kind="cyclist"))
    roads.append(GC.road(18, "road_edge", GC.segment(hx - 0.3, hy - 0.6, 0.05, 3.0)))
    roads.append(GC.road(19, "stop_sign", [(40.0, 55.0)]))
    cars.append(GC.car(22, 40.0, 57.0, PI / 2))
    return GC.World(name, cars, roads, moves=[(0, -4.0 * math.sin(0.2), 4.0 * math.cos(0.2), 0.0), (22, 0.0, -1.2, 0.0)])


def _types_premise(case, inp, w=0):
    ref = CR.collision_reference(inp, w, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    verdicts = []
    for k in range(18):
        at, rt = TYPE_OF[AGENT_KINDS[k // 6][0]], TYPE_OF[ROAD_KINDS[k % 6]]
        assert e["type"][k] == at and e["type"][n + k] == rt and ref["sep"][k, n + k] < -0.2, (k, ref["sep"][k, n + k])
        table = (at, rt) not in CR.FILTERED_PAIRS and (rt, at) not in CR.FILTERED_PAIRS
        assert bool(ref["collided"][k]) == table and ref["info"][k].tolist() == [int(table), 0, 0], (k, ref["info"][k])
        alone = (ref["pairs"][k] & (ref["sep"][k] <= 0)).sum()
        assert alone == int(table), "placement %d is not isolated" % k
        verdicts.append(table)
    # the table lets four of the eighteen collide: a vehicle on a road edge, and all three kinds on a stop sign
    assert sum(verdicts) == 4 and verdicts[0] and verdicts[5] and verdicts[11] and verdicts[17]
    assert ref["info"][18].tolist() == [1, 1, 1]
    hits = np.nonzero(ref["pairs"][18] & (ref["sep"][18] <= 0))[0].tolist()
    assert hits == [19, 20, 21, n + 18], hits
    assert len({j % 4 for j in hits[:3]}) == 3 and len({j % 2 for j in hits[:3]}) == 2, "the partners share a thread of agent 18"
    assert not ref["collided"][22]
    _aimed_ok(case, ref, [(k, n + k) for k in range(18)] + [(18, j) for j in hits] + [(22, n + 19)], case.name)
    return "18 placements: verdicts equal the filter table (%d collide); agent 18 hits rows %s -> info %s" % \
        (sum(verdicts), hits, ref["info"][18].tolist())


# ------------------------------------------------------------------------------------------------------------------
# coll_static_inactive
# ------------------------------------------------------------------------------------------------------------------
def _static_world():
    """0, 1: parked on parked.  2: parked on road edge 0.  3 (controlled) on 4 (parked).  5 (expert, log invalid) on 6
    (controlled).  7 (controlled, at the padding height) on 8 (controlled).  9: controlled, 1 m from its goal, with 10
    (controlled) 8 m away -- the done rule, see done_rule_pass.  11 (controlled) beside 12 (parked), clear."""
    cars = [parked(0, 0.0, 0.0, 0.2), parked(1, 1.0, 0.5, 1.1), parked(2, 20.0, 0.0, 0.7), GC.car(3, 40.0, 0.0, 0.3),
            parked(4, 41.0, 0.6, 1.3), ghost(5, 60.0, 0.0, 0.4), GC.car(6, 60.8, 0.5, 2.0), GC.car(7, 80.0, 0.0, 0.1),
            GC.car(8, 80.7, -0.4, 1.0), GC.car(9, 0.0, 30.0, 0.5), GC.car(10, 8.0, 30.0, 0.9), GC.car(11, 40.0, 30.0, 0.0),
            parked(12, 40.0, 32.2, 0.0)]
    cars[9]["goalPosition"] = {"x": 1.0, "y": 30.0, "z": 0.0}
    roads = [GC.road(0, "road_edge", GC.segment(20.0, 0.0, 0.0, 5.0)), GC.road(1, "road_edge", GC.segment(100.0, 40.0, 1.0, 8.0))]
    z = np.ones(13, f32)
    z[7] = CR.PAD_Z
    return GC.World("static_inactive", cars, roads, z=z, moves=[(3, -4.0, -1.0, 0.0), (11, 0.0, 1.4, 0.0)])


def _static_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    n = ref["ents"]["n"]
    sep, hit = ref["sep"], ref["collided"]
    resp, ctl = inp["resp"][0], inp["controlled"][0, :, 0]
    assert [int(resp[a] == CR.RESP_STATIC) for a in range(13)] == [1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]
    assert [int(ctl[a]) for a in range(13)] == [0, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0]
    for a, b in ((0, 1), (2, n + 0), (3, 4), (5, 6), (7, 8)):
        assert sep[a, b] < -0.2, (a, b, sep[a, b])
    assert not hit[0] and not hit[1], "parked on parked"
    assert not hit[2], "parked on an edge"
    assert hit[3] and hit[4] and ref["info"][3].tolist() == [0, 1, 0] and ref["info"][4].tolist() == [0, 1, 0], "controlled on parked"
    assert not ref["active"][5] and not hit[5] and not hit[6], "an expert whose log is invalid"
    assert not ref["active"][7] and not hit[7] and not hit[8], "an agent at the padding height"
    assert not hit[9] and not hit[10] and sep[9, 10] > 1.0 and not hit[11] and not hit[12]
    return "parked on parked, parked on an edge, controlled on parked, invalid expert on controlled, padded on controlled: " \
        "every pair sep < -0.2 (largest %.2f), collided only 3 and 4" % max(sep[a, b] for a, b in ((0, 1), (2, n), (3, 4), (5, 6), (7, 8)))


def done_rule_pass(case, sims):
    """coll_static_inactive after its step pass: agent 9 has reached its goal and is done, not collided, and -- no further step
    having moved it away -- still in place.  Agent 10 is written on top of it and the world recomputed without a step.  Returns
    every simulator's snapshot ahead of that."""
    before = [CR.read_inputs(s) for s in sims]
    for b in before:
        assert b["done"][0, 9] == 1 and b["state"][0, 9, 10] == 0 and b["state"][0, 9, 2] != CR.PAD_Z
    st = before[0]["state"].copy()
    st[0, 10, 0:2] = st[0, 9, 0:2] + f32(0.4)
    st[..., 10] = 0
    for s in sims:
        (s.set_state if hasattr(s, "set_state") else s.debug_set_state)(st)
        s.reset([])
    return before


# ------------------------------------------------------------------------------------------------------------------
# coll_near_miss
# ------------------------------------------------------------------------------------------------------------------
NEAR_GAP = 0.03


def _solve_distance(A, byaw, bhx, bhy, direction, gap):
    """The distance t along `direction` from A's centre at which rectangle B has separation(A, B) = gap (bisection: the
    separation of two convex shapes moving apart from a common centre along a ray never decreases)."""
    lo, hi = 0.0, 60.0
    for _ in range(60):
        t = (lo + hi) / 2
        s = CR.separation(A, (A[0] + t * math.cos(direction), A[1] + t * math.sin(direction), byaw, bhx, bhy))
        lo, hi = (t, hi) if s < gap else (lo, t)
    return (lo + hi) / 2


def _near_world():
    """60 isolated pairs on a grid 32 m apart, gaps alternately +3 cm and -3 cm: 15 corner-to-side, 15 corner-to-corner, 15
    T-bone (car against car; relative yaws sweep the circle and include the multiples of pi / 2), 15 of a diagonal car against
    a 30 m road edge, near its tip."""
    cars, roads = [], []
    hx, hy = 0.7 * 2.0, 0.7 * 1.0
    for k in range(60):
        sx, sy = (k % 8 - 3.5) * 32.0, (k // 8 - 3.5) * 32.0
        gap = NEAR_GAP if k % 2 == 0 else -NEAR_GAP
        kind, j = k // 15, k % 15
        alpha = 0.41 * k
        if kind == 3:
            seg_ang = alpha
            A = (sx, sy, seg_ang, 15.0, 0.1)
            byaw = seg_ang + PI / 4 + 0.35 * (j % 3) + (PI / 2) * (j // 3)
            direction = seg_ang + (PI / 2 if j % 2 else -PI / 2)
            # the car's contact point lies 13 m along the segment: shift A's frame instead of the ray
            ox, oy = 13.0 * math.cos(seg_ang) * (1 if j % 4 < 2 else -1), 13.0 * math.sin(seg_ang) * (1 if j % 4 < 2 else -1)
            t = _solve_distance((sx + ox, sy + oy, seg_ang, 2.0, 0.1), byaw, hx, hy, direction, gap)
            roads.append(GC.road(len(roads), "road_edge", GC.segment(sx, sy, seg_ang, 15.0)))
            cars.append(GC.car(len(cars), sx + ox + t * math.cos(direction), sy + oy + t * math.sin(direction), byaw))
            continue
        A = (sx, sy, alpha, hx, hy)
        if kind == 0:      # a corner of B against a long side of A
            byaw, direction = alpha + PI / 4 + (PI / 2) * (j % 4) + 0.2 * (j // 4), alpha + PI / 2 + 0.15 * (j % 3 - 1)
        elif kind == 1:    # corner to corner: along A's diagonal, B turned by a multiple of pi / 2 (exactly, for j < 8)
            byaw = alpha + (PI / 2) * (j % 4) + (0.0 if j < 8 else 0.3)
            direction = alpha + math.atan2(hy, hx) * (1 if j % 2 else -1) + (PI if j % 3 == 0 else 0.0)
        else:              # T-bone: B across A's nose or tail
            byaw, direction = alpha + PI / 2 + (PI if j % 2 else 0.0) + 0.02 * (j // 10), alpha + (PI if j % 4 < 2 else 0.0)
        t = _solve_distance(A, byaw, hx, hy, direction, gap)
        cars.append(GC.car(len(cars), sx, sy, alpha))
        cars.append(GC.car(len(cars), sx + t * math.cos(direction), sy + t * math.sin(direction), byaw))
    # pair 0 (agents 0, 1; +3 cm) closes by 6 cm, pair 1 (agents 2, 3; -3 cm) opens by 6 cm
    d0, d1 = PI / 2 - 0.15, 0.41 + PI / 2
    return GC.World("near_miss", cars, roads, moves=[(1, -0.06 * math.cos(d0), -0.06 * math.sin(d0), 0.0),
                                                     (3, 0.06 * math.cos(d1), 0.06 * math.sin(d1), 0.0)])


def _near_pairs(n):
    """The 60 aimed pairs as (agent, entity row): 45 car pairs in slots (2 k, 2 k + 1), then car 90 + j against road row j."""
    return [(2 * k, 2 * k + 1) for k in range(45)] + [(90 + j, n + j) for j in range(15)]


def _near_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    assert n == 105
    pairs = _near_pairs(n)
    sep = np.asarray([ref["sep"][a, b] for a, b in pairs])
    assert np.allclose(np.abs(sep), NEAR_GAP, atol=1e-3), "gaps must be +-3 cm: %s" % sep[np.abs(np.abs(sep) - NEAR_GAP) > 1e-3]
    circ = _circles(ref)
    ext_x = np.abs(np.cos(e["yaw"])) * e["hx"] + np.abs(np.sin(e["yaw"])) * e["hy"]
    ext_y = np.abs(np.sin(e["yaw"])) * e["hx"] + np.abs(np.cos(e["yaw"])) * e["hy"]
    tight = [circ[a, b] and abs(e["cx"][a] - e["cx"][b]) <= ext_x[a] + ext_x[b] and abs(e["cy"][a] - e["cy"][b]) <= ext_y[a] + ext_y[b]
             for a, b in pairs]
    apart = int(sum(t and s > 0 for t, s in zip(tight, sep)))
    touching = int(((sep < 0) & (sep > -0.05)).sum())
    assert apart >= 25 and touching >= 25, (apart, touching)
    for a, b in pairs:   # isolated: each agent of a pair has no other pair within a metre
        close = ref["pairs"][a] & (ref["sep"][a] < 1.0)
        assert close.sum() == 1 and close[b], (a, b)
    rel = np.asarray([(e["yaw"][b] - e["yaw"][a]) % (PI / 2) for a, b in pairs[:45]])
    square = int((np.minimum(rel, PI / 2 - rel) < 1e-5).sum())
    assert square >= 15, square
    _aimed_ok(case, ref, pairs, case.name)
    return "60 pairs at +-3 cm: %d apart with circles and axis-aligned boxes overlapping, %d overlapping by < 5 cm; %d at " \
        "relative yaws that are multiples of pi / 2" % (apart, touching, square)


# ------------------------------------------------------------------------------------------------------------------
# coll_no_boxes
# ------------------------------------------------------------------------------------------------------------------
def _no_boxes_world():
    """Lanes and road lines only -- no road edge, no stop sign, so no broadphase grid -- under five vehicles: 0 on 1, 2 on a lane
    and alone, 3 beside 4 (the step pass pushes them together and 0 off 1)."""
    cars = [GC.car(0, 0.0, 0.0, 0.3), GC.car(1, 1.5, 0.8, 1.2), GC.car(2, 12.0, 0.0, 0.1), GC.car(3, 24.0, 0.0, 0.0), GC.car(4, 24.0, 2.0, 0.0)]
    roads = [GC.road(0, "lane", GC.segment(6.0, 0.0, 0.02, 20.0)), GC.road(1, "road_line", GC.segment(6.0, 3.0, 0.0, 20.0)),
             GC.road(2, "lane", GC.segment(12.0, -4.0, 1.0, 6.0))]
    return GC.World("no_boxes", cars, roads, moves=[(0, -5.0, -3.0, 0.0), (4, 0.0, -0.8, 0.0)])


def _no_boxes_premise(case, inp):
    ref = CR.collision_reference(inp, 0, case.band)
    e, n = ref["ents"], ref["ents"]["n"]
    assert grid_of(ref) is None, "world 0 must have no road edge and no stop sign"
    assert ref["sep"][0, 1] < -0.2 and ref["collided"][:5].tolist() == [True, True, False, False, False]
    assert ref["sep"][2, n + 0] < -0.2, "vehicle 2 stands on a lane (filtered)"
    _aimed_ok(case, ref, [(0, 1), (3, 4)], case.name)
    return "world 0: no boxes, vehicles 0 and 1 overlap (sep %.2f); world 1: " % ref["sep"][0, 1] + _types_premise(case, inp, 1)


CASE_LIST = [
    Case("coll_far_cells", [_far_world()], 400.0, _far_premise),
    Case("coll_grid_border", [_border_world()], 600.0, _border_premise),
    Case("coll_wide_world", [_wide_world()], 1500.0, _wide_premise),
    Case("coll_crowd64", [_crowd_world(64)], 150.0, _crowd_premise),
    Case("coll_crowd128", [_crowd_world(128)], 150.0, _crowd_premise, slots=128),
    Case("coll_types", [_types_world()], 150.0, _types_premise),
    Case("coll_static_inactive", [_static_world()], 150.0, _static_premise, goal_threshold=2.0),
    Case("coll_near_miss", [_near_world()], 150.0, _near_premise, slots=128),
    Case("coll_no_boxes", [_no_boxes_world(), _types_world("types_beside")], 150.0, _no_boxes_premise),
]
CASES = {c.name: c for c in CASE_LIST}
BEHAVIOUR_CASES = ("coll_types", "coll_crowd64", "coll_crowd128")


# ------------------------------------------------------------------------------------------------------------------
# the passes
# ------------------------------------------------------------------------------------------------------------------
def place(case, sims):
    """GC.place; returns every simulator's snapshot ahead of it (the info columns the pass keeps)."""
    before = [CR.read_inputs(s) for s in sims]
    GC.place(case, sims)
    return before


def step_pass(case, sims):
    """One State-model step on every simulator of `sims`: every agent is handed back its pose except each world's two `moves`.
    Returns every simulator's snapshot ahead of it."""
    before = [CR.read_inputs(s) for s in sims]
    act = GC.state_step_actions(case, sims[0])
    for s in sims:
        P.write_actions(s, act)
        s.step()
    return before


def hold_step(case, sims):
    """The step after step_pass: every agent is handed back the pose it has now.  Returns every simulator's snapshot ahead of
    it."""
    before = [CR.read_inputs(s) for s in sims]
    st = before[0]["state"]
    act = np.zeros(st.shape[:2] + (10,), f32)
    act[..., 0:3] = st[..., 0:3]
    for w, wd in enumerate(case.worlds):
        yaw = wd.yaw.copy()
        for a, _, _, dyaw in wd.moves:
            yaw[a] = P.agreeing_yaw(f32(yaw[a] + f32(dyaw)))
        act[w, :wd.n, 3] = yaw
    for s in sims:
        P.write_actions(s, act)
        s.step()
    return before


def moved_flags(case, refs_before, refs_after):
    """The step pass's two agents per world change their verdict: one from clear into contact, one from contact to clear."""
    for w, wd in enumerate(case.worlds):
        flips = sorted((bool(refs_before[w]["collided"][a]), bool(refs_after[w]["collided"][a])) for a, _, _, _ in wd.moves)
        assert flips == [(False, True), (True, False)], "%s world %d: the moves give %s" % (case.name, w, flips)


# ------------------------------------------------------------------------------------------------------------------
# comparison with the reference
# ------------------------------------------------------------------------------------------------------------------
def flags_of(sim):
    """(collided [W, A] from the state, info [W, A, 3], collided as the self observation shows it, done, z)."""
    st = np.asarray(sim.get_state() if hasattr(sim, "get_state") else sim.debug_get_state())
    return dict(collided=st[..., 10] != 0, info=GR._np(sim.info_tensor())[..., 0:3].copy(),
                self_obs=GR._np(sim.self_observation_tensor())[..., 6] != 0, done=GR._np(sim.done_tensor())[..., 0] != 0,
                z=st[..., 2].copy())


def compare_to_reference(case, sim, what, before=None, behaviour=None):
    """Every live agent's collided flag (state column 10 and self observation column 6) and info[0:3] against the reference of
    the simulator's own tensors, outside the margin.  before: the snapshot (CR.read_inputs) ahead of the pass; behaviour: the
    step's collision behaviour, or None for a pass that moves nothing and starts from collided flags written as 0 -- such a
    pass clears no info column, so what `before` shows is kept and the fresh flags are added.
    Returns dict(agents, colliding, marginal)."""
    inp = CR.read_inputs(sim)
    got = flags_of(sim)
    out = dict(agents=0, colliding=0, marginal=0)
    for w in range(len(case.worlds)):
        if behaviour is None:
            seen = before or inp
            ref = CR.collision_reference(inp, w, case.band, dict(done=seen["done"] != 0, collided=np.zeros(seen["done"].shape, bool),
                                                                 step=CR.EPISODE - seen["steps"]))
            n = len(ref["collided"])
            kept = np.zeros((n, 3), bool) if before is None else before["info"][w, :n, 0:3] != 0
            want = dict(collided=ref["collided"], info=(ref["info"] != 0) | kept, done_at_least=np.zeros(n, bool), padded=np.zeros(n, bool))
        else:
            ref = CR.collision_reference(inp, w, case.band, CR.seen_in_step(before, behaviour))
            want = CR.expected_after_step(CR.world_slice(before, w), ref, behaviour)
        n = len(ref["collided"])
        ok = ~ref["margin"]
        bad = ok & ((got["collided"][w, :n] != want["collided"]) | (got["self_obs"][w, :n] != want["collided"]) |
                    ((got["info"][w, :n] != 0) != (np.asarray(want["info"]) != 0)).any(-1))
        if bad.any():
            a = int(np.nonzero(bad)[0][0])
            near = np.argsort(np.abs(np.where(ref["pairs"][a], ref["sep"][a], np.inf)))[:3]
            raise AssertionError("%s: world %d: %d non-marginal agents differ from the reference; first agent %d: got collided %s "
                                 "(self obs %s) info %s, reference %s %s; its nearest pairs (row: sep) %s" %
                                 (what, w, int(bad.sum()), a, got["collided"][w, a], got["self_obs"][w, a], got["info"][w, a].tolist(),
                                  bool(want["collided"][a]), np.asarray(want["info"])[a].astype(int).tolist(),
                                  ", ".join("%d: %.4g" % (j, ref["sep"][a, j]) for j in near)))
        assert (got["done"][w, :n] | ~want["done_at_least"]).all(), "%s: world %d: a collided agent is not done" % (what, w)
        assert (got["z"][w, :n][want["padded"]] == CR.PAD_Z).all(), "%s: world %d: a removed agent is not at the padding position" % (what, w)
        assert not ref["active"][want["padded"]].any()
        out["agents"] += n
        out["colliding"] += int(np.asarray(want["collided"]).sum())
        out["marginal"] += int(ref["margin"].sum())
    return out


def marginal_differences(case, sim_a, sim_b):
    """For a failure text: where two simulators' flags differ, and whether the reference calls those agents marginal."""
    inp = CR.read_inputs(sim_b)
    a, b = flags_of(sim_a), flags_of(sim_b)
    lines = []
    for w in range(len(case.worlds)):
        ref = CR.collision_reference(inp, w, case.band)
        n = len(ref["collided"])
        d = (a["collided"][w, :n] != b["collided"][w, :n]) | (a["info"][w, :n] != b["info"][w, :n]).any(-1)
        if d.any():
            lines.append("world %d: %d agents differ, %d of them marginal" % (w, int(d.sum()), int((d & ref["margin"]).sum())))
    return "; ".join(lines) or "no agent differs in collided / info[0:3]"
