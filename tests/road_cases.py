"""Constructed, MOVING worlds for the road-row reference (tests/road_reference.py): each case aims a handful of agents at one rule
or one code path of the road selection that the Waymo and bench scenes under seeded actions never reach -- a road exactly on
the radius, K - 1 / K / K + 1 roads, 33 roads with one key, a candidate list one below, on and one above a tile or a limit, an
agent that jumps 500 m, swaps places with another or comes back from the padding position -- on worlds large enough to leave
the fallback, and asserts its own premise FROM THE REFERENCE'S INTERMEDIATE VALUES (and, where the premise is which path ran,
from debug_road_path()) so that it cannot quietly stop exercising that rule.

Scenes are built with the helpers of tests/geom_cases.py and tests/step_cases.py.  All cases: polylineReductionThreshold = 0,
initOnlyValidAgentsAtFirstStep = 0, isStaticAgentControlled = 0, collisionBehaviour = Ignore unless the case says otherwise,
observationRadius = 50.

TOLERANCES.  Every bound on a float column, the key margin and the radius band are ORACLE_ROAD_MAX[span][column]: the largest
distance of the ORACLE (float32, host libm) from the reference over every road of every agent on every pass of every run of
tests/test_road_reference.py, per coordinate span of the world.  That suite asserts that the oracle stays within each constant
and that no constant is more than twice what is measured.  The GPU suite allows GPU_FACTOR times the constant -- the factor and
the reason of tests/step_cases.py: the device's double-then-round transcendentals differ from glibc's float ones by about an
ulp -- and no bound is ever taken from a kernel's output.  Scale, type, id, mapType and every padding row are exact."""
import math

import numpy as np

from tests import collision_cases as CC
from tests import collision_reference as CR
from tests import geom_cases as GC
from tests import geom_reference as GR
from tests import parity as P
from tests import road_reference as RR
from tests import step_cases as SC
from tests import step_reference as SR

f32 = np.float32
f64 = np.float64
PI = GC.PI
K = RR.K
GPU_FACTOR = 2.0
MARGIN_AGENTS = CC.MARGIN_AGENTS
RADIUS = 50.0
COLUMNS = ("x", "y", "heading", "key", "dist")

# span: column: the largest |oracle - reference| (metres, radians; key on the scale of RR.gap), rounded up; the measured value in
# the comment.  x / y / heading / dist over the roads within radius + 1 m, key over every road.
ORACLE_ROAD_MAX = {
    # measured: x 1.487e-05 (road_tiles_b), y 1.432e-05 (road_slots128), heading 6.200e-07 (road_tiles_a), key 8.458e-07
    # (road_slots128), dist 1.660e-05 (road_ties)
    150.0: dict(x=1.5e-5, y=1.5e-5, heading=6.3e-7, key=8.5e-7, dist=1.7e-5),
    # measured: x 1.321e-05, y 1.126e-05 (road_fast), heading 3.832e-07, key 6.069e-07 (road_fast), dist 1.516e-05 (x, heading,
    # dist: road_cells)
    1500.0: dict(x=1.4e-5, y=1.2e-5, heading=3.9e-7, key=6.1e-7, dist=1.6e-5),
}

# road selection: (reference mode, knn_order, roadObservationAlgorithm, environment of the HIP engine)
MODES = {
    "ref_order_rank": (RR.KNN, 0, 0, {"GPUDRIVE_RANK_MIN_ROADS": "200"}),
    "ref_order_history": (RR.KNN, 0, 0, {"GPUDRIVE_NO_RANK_REPLAY": "1"}),
    "set_order_fused": (RR.SET, 1, 0, {"GPUDRIVE_SET_FUSED_ROWS": "1"}),
    "set_order_row_kernel": (RR.SET, 1, 0, {"GPUDRIVE_SET_FUSED_ROWS": "0"}),
    "linear": (RR.LINEAR, 0, 1, {}),
}
KNN_MODES = ("ref_order_rank", "ref_order_history", "set_order_fused", "set_order_row_kernel")
CPU_MODES = {RR.KNN: 0, RR.SET: 0, RR.LINEAR: 1}     # the oracle has one k-NN: its rows are a set-order answer too


def key_margin(span, factor):
    return factor * ORACLE_ROAD_MAX[span]["key"]


def band_of(span, factor):
    return factor * ORACLE_ROAD_MAX[span]["dist"]


# ------------------------------------------------------------------------------------------------------------------
# scene building
# ------------------------------------------------------------------------------------------------------------------
KINDS = ("road_edge", "lane", "road_line")


def short_roads(centres, first=0, half=0.5, kinds=KINDS):
    """One two-point polyline (one road row) per centre, turned by an angle of its own."""
    return [GC.road(first + i, kinds[i % len(kinds)], GC.segment(cx, cy, 0.37 * (first + i), half)) for i, (cx, cy) in enumerate(centres)]


def chain_roads(points, first=0, per=60, kinds=KINDS):
    """Polylines through `points`, `per` road rows each (consecutive polylines share an end point: one row per pair of
    consecutive points is what the world gets, len(points) - 1 in all, in this order)."""
    roads, i = [], 0
    while i < len(points) - 1:
        j = min(i + per, len(points) - 1)
        roads.append(GC.road(first + len(roads), kinds[len(roads) % len(kinds)], points[i:j + 1]))
        i = j
    return roads


def spiral(n, r0, dr, turn=2.39996323, x0=0.0, y0=0.0):
    return [(x0 + (r0 + dr * i) * math.cos(turn * i), y0 + (r0 + dr * i) * math.sin(turn * i)) for i in range(n)]


def line_points(n, s, x0=0.0, y0=0.0, angle=0.0, first=0.0):
    """n points s apart on a straight line through (x0, y0), centred on it (`first`: the line parameter of point 0 instead).
    Seen from anywhere, keys along ONE line are (t_i - t)^2 + h^2: two of them come close only in the pairs mirrored about the
    agent's foot point, all by the same fraction of s^2, so an agent is order-decided wherever it stands or moves (almost
    surely); roads scattered over the plane leave one agent in ten undecided at 800 roads."""
    t0 = first if first else -0.5 * s * (n - 1)
    return [(x0 + (t0 + s * i) * math.cos(angle), y0 + (t0 + s * i) * math.sin(angle)) for i in range(n)]


def line_roads(n, s, seed, x0=0.0, y0=0.0, angle=0.0, per=40, kinds=KINDS):
    """n road rows s apart along a straight line, as polylines of `per` rows each in a shuffled order."""
    pts = line_points(n + 1, s, x0, y0, angle)
    chains = [pts[i:min(i + per, n) + 1] for i in range(0, n, per)]
    return [GC.road(j, kinds[j % len(kinds)], c) for j, c in enumerate(shuffled(chains, seed))]


def on_line(t, h, angle=0.0, x0=0.0, y0=0.0):
    """The point t along and h to the left of the line of line_points."""
    return x0 + t * math.cos(angle) - h * math.sin(angle), y0 + t * math.sin(angle) + h * math.cos(angle)


def shuffled(items, seed):
    items = list(items)
    np.random.default_rng(seed).shuffle(items)
    return items


class Case:
    def __init__(self, name, worlds, model, actions, premise, steps, slots=64, radius=RADIUS, modes=tuple(MODES), behaviour=CR.IGNORE,
                 events=None, gpu_premise=None, extra=None, threshold=2.0):
        self.name, self.worlds, self.model, self.actions, self.premise, self.steps = name, worlds, model, actions, premise, steps
        self.slots, self.radius, self.modes, self.behaviour, self.events = slots, radius, modes, behaviour, events or {}
        self.gpu_premise, self.extra, self.threshold, self.heads_for = gpu_premise, extra or {}, threshold, None
        assert len(worlds) <= 8 and steps + 1 + len(self.events) <= 12, name
        for wd in worlds:
            assert wd.n <= slots, name

    write = GC.Case.write

    def params(self, algo):
        kw = dict(polylineReductionThreshold=0.0, collisionBehaviour=self.behaviour, dynamicsModel=self.model, observationRadius=self.radius,
                  initOnlyValidAgentsAtFirstStep=0, isStaticAgentControlled=0, rewardType=SR.ON_GOAL, distanceToGoalThreshold=self.threshold,
                  roadObservationAlgorithm=algo)
        kw.update(self.extra)
        return kw


class Run:
    """One scripted run of a case in one mode on one or more simulators that are given the same actions (the first one's
    tensors are the template).  passes: dict(tag, reset, snaps: one RR.snapshot per simulator, state) per pass."""

    def __init__(self, case, sims, mode):
        self.case, self.sims, self.mode = case, list(sims), mode
        self.yaw = np.zeros((len(case.worlds), case.slots), f32)     # the yaw the State model last handed every agent
        for w, wd in enumerate(case.worlds):
            self.yaw[w, :wd.n] = wd.yaw
        self.passes, self._refs = [], {}

    def _record(self, tag, reset):
        self.passes.append(dict(tag=tag, reset=reset, snaps=[RR.snapshot(s) for s in self.sims], state=SC._get_state(self.sims[0])))
        return self.passes[-1]

    def place(self):
        GC.place(self.case, self.sims)
        if any(wd.vel is not None for wd in self.case.worlds):
            st = SC._get_state(self.sims[0])
            for w, wd in enumerate(self.case.worlds):
                if wd.vel is not None:
                    st[w, :wd.n, 7:10] = wd.vel
            for s in self.sims:
                SC._set_state(s, st)
                s.reset([])
        return self._record("reset pass", True)

    def step(self, k):
        before = dict(state=SC._get_state(self.sims[0]), map_obs=self.passes[-1]["snaps"][0]["map_obs"], shape=self.passes[-1]["snaps"][0]["shape"])
        act = self.case.actions(self, k, before)
        for s in self.sims:
            P.write_actions(s, act)
            s.step()
        return self._record("step %d" % (k + 1), False)

    def hold_pose(self, before):
        """State-model actions that hand every agent back the pose it has (the yaw as the host last gave it: bit for bit)."""
        st = before["state"]
        act = np.zeros(st.shape[:2] + (10,), f32)
        act[..., 0:3] = st[..., 0:3]
        act[..., 3] = self.yaw
        act[..., 4:7] = st[..., 7:10]
        return act

    def put(self, act, w, a, x=None, y=None, yaw=None):
        """Into State-model actions: agent (w, a) at (x, y) turned to yaw (the nearest yaw both sides rotate alike by)."""
        if x is not None:
            act[w, a, 0] = f32(x)
        if y is not None:
            act[w, a, 1] = f32(y)
        if yaw is not None:
            act[w, a, 3] = self.yaw[w, a] = P.agreeing_yaw(f32(yaw))

    def ref(self, p, w, a, mode=None, factor=GPU_FACTOR, variant=None, sim=0):
        """The reference of agent (w, a) from simulator `sim`'s own tensors after pass p."""
        mode = mode or MODES[self.mode][0]
        key = (p, w, a, mode, variant, sim)
        if key not in self._refs:
            self._refs[key] = RR.road_core(self.passes[p]["snaps"][sim], w, a, self.case.radius, mode, variant)
        span = self.case.worlds[w].span
        return RR.road_reference(None, w, a, self.case.radius, mode, key_margin(span, factor), band_of(span, factor), variant, core=self._refs[key])

    def agents(self):
        return [(w, a) for w, wd in enumerate(self.case.worlds) for a in range(wd.n)]


def script(run, check):
    """The whole scripted run of run.case: place, every step, and the case's events (after step k: a partial reset, a set_maps);
    check(pass index) is called after every pass."""
    run.place()
    check(0)
    for k in range(run.case.steps):
        run.step(k)
        check(len(run.passes) - 1)
        if k in run.case.events:
            tag = run.case.events[k](run)
            run._record(tag, True)
            check(len(run.passes) - 1)


def _blank(run):
    return np.zeros((len(run.case.worlds), run.case.slots, 10), f32)


def _world(name, cars, roads, span=150.0, vel=None):
    return SC.world(name, cars, roads, span=span, vel=vel)


def _shift_actions(run, k, before):
    """State model: every agent is handed back its pose; agent a of every world is shifted by 0.5 m on step k when (a + k) is even
    and turned by 0.05 when (a + k) % 3 == 0."""
    act = run.hold_pose(before)
    for w, a in run.agents():
        if (a + k) % 2 == 0:
            run.put(act, w, a, x=before["state"][w, a, 0] + f32(0.4), y=before["state"][w, a, 1] - f32(0.3))
        if (a + k) % 3 == 0:
            run.put(act, w, a, yaw=run.yaw[w, a] + f32(0.05))
    return act


def in_reach(ref, radius=RADIUS):
    return int((ref["dist"] <= radius).sum())


# ------------------------------------------------------------------------------------------------------------------
# road_counts
# ------------------------------------------------------------------------------------------------------------------
def _counts_worlds():
    cars = lambda pts: [GC.car(i, x, y, 0.3 + 1.1 * i) for i, (x, y) in enumerate(pts)]
    far = [(300.0, 300.0)]
    inner200 = spiral(200, 3.0, 0.18)                                       # all within 39 m of the origin
    k201 = shuffled(short_roads(inner200[:57] + far + inner200[57:]), 11)
    return [
        _world("c199", cars([(0.4, 0.3), (20.0, -10.0), (-70.0, 0.0)]), shuffled(short_roads(spiral(199, 6.0, 0.3)), 1)),
        _world("c200", cars([(0.4, 0.3), (20.0, -10.0), (-70.0, 0.0)]), shuffled(short_roads(spiral(200, 6.0, 0.3)), 2)),
        _world("c201k", cars([(0.4, 0.3), (30.0, 5.0), (0.0, -8.0)]), k201, span=1500.0),
        _world("c200k", cars([(0.4, 0.3), (30.0, 5.0)]), shuffled(short_roads(inner200), 12)),
        _world("c260", cars([(0.4, 0.3), (15.0, 25.0), (130.0, 0.0)]), shuffled(short_roads(spiral(260, 3.0, 0.16)), 3)),
        _world("cfar", cars([(0.4, 0.3), (10.0, -30.0)]), shuffled(short_roads(spiral(230, 1.0, 0.08, x0=400.0)), 4), span=1500.0),
    ]


def _counts_premise(run):
    shape = run.passes[0]["snaps"][0]["shape"]
    assert shape[:, 1].tolist() == [K - 1, K, K + 1, K, 260, 230], shape[:, 1]
    seen = dict(front=0, middle=0, end=0)
    reach = {}
    for p in range(len(run.passes)):
        for w, a in run.agents():
            ref = run.ref(p, w, a, RR.KNN)
            reach.setdefault(w, set()).add(in_reach(ref))
            if ref["heap"] is not None and len(ref["heap"]) > 0:
                out = ref["dist"][ref["heap"]] > RADIUS
                if out.any() and not out.all():
                    seen["front"] += bool(out[0])
                    seen["end"] += bool(out[-1])
                    seen["middle"] += bool(out[1:-1].any())
    assert K in reach[2] and K in reach[3], "exactly K roads in reach (of K + 1 and of K): %s" % reach
    assert any(v < K for v in reach[0]) and any(v > K for v in reach[4]) and reach[5] == {0}, reach
    assert 0 in reach[4], "the agent outside c260's road box"
    assert all(v > 0 for v in seen.values()), "out-of-radius rows at the front, in the middle and at the end of the heap array: %s" % seen
    return "roads per world %s; in reach per world %s; heap arrays with out-of-radius rows at the front / in the middle / at the end: %s" % (
        shape[:, 1].tolist(), {w: sorted(v) for w, v in reach.items()}, seen)


def _counts_gpu_premise(run, paths):
    if run.mode != "ref_order_rank":
        return ""
    last = paths[-1]
    assert (last[0, :3] == -10).all(), "a world of K - 1 roads is not ranked: %s" % last[0, :3]
    assert last[4, 2] == -3 and (last[5, :2] == -3).all(), "agents out of reach of every road: %s %s" % (last[4, :3], last[5, :2])
    assert (last[1, :3] > 0).all() and (last[4, :2] > 0).all(), (last[1, :3], last[4, :3])
    return "K - 1 roads: -10; out of reach: -3; K, K + 1 and 260 roads ranked"


# ------------------------------------------------------------------------------------------------------------------
# road_radius
# ------------------------------------------------------------------------------------------------------------------
UP50, DOWN50 = float(np.nextafter(f32(50), f32(100))), float(np.nextafter(f32(50), f32(0)))
# agent a aims at target a: its offset from the agent (float32 arithmetic on these is exact)
RADIUS_AIMS = ((30.0, 40.0), (0.0, 50.0), (0.0, UP50), (0.0, DOWN50), (50.0, 0.0), (14.0, 48.0), (UP50, 0.0), (DOWN50, 0.0))
RADIUS_WANT = (True, True, False, True, True, True, False, True)


def _radius_world():
    targets = [(40.0 + 1.7 * j, 55.0 + 0.9 * j) for j in range(8)]
    filler = spiral(150, 0.5, 0.07, x0=25.0, y0=10.0) + line_points(65, 0.5, x0=-120.0, y0=-90.0, angle=0.6435)      # 65 of them out of every reach, on a line through the agents' corner
    roads = [GC.road(j, "stop_sign", [t]) for j, t in enumerate(targets)] + short_roads(filler, first=8)
    cars = [GC.car(a, tx - dx + 1.0, ty - dy - 1.0, 0.0) for a, ((tx, ty), (dx, dy)) in enumerate(zip(targets, RADIUS_AIMS))]
    return _world("radius", cars, roads)


def _radius_actions(run, k, before):
    """Step 1 puts agent a at target a minus its offset, computed from the exported road rows; step 2 hands the poses back; step
    3 moves every agent on to the next agent's target."""
    act = run.hold_pose(before)
    if k in (0, 2):
        for a, (dx, dy) in enumerate(RADIUS_AIMS):
            t = before["map_obs"][0, (a + (k == 2)) % 8, 0:2]
            run.put(act, 0, a, x=f32(t[0]) - f32(dx), y=f32(t[1]) - f32(dy), yaw=0.0)
    return act


def _radius_premise(run):
    texts = []
    for p, shift in ((1, 0), (2, 0), (3, 1)):
        got = []
        for a in range(8):
            ref = run.ref(p, 0, a, RR.KNN)
            t = (a + shift) % 8
            snap = run.passes[p]["snaps"][0]
            exact = RR.exact_verdict(snap["map_obs"][0, :ref["R"]], snap["abs_obs"][0, a, 0], snap["abs_obs"][0, a, 1], snap["abs_obs"][0, a, 3:7])
            want = math.hypot(*RADIUS_AIMS[a])
            assert exact[t] and ref["dist"][t] == want, "pass %d agent %d: offset %r is not exact (distance %r)" % (p, a, RADIUS_AIMS[a], ref["dist"][t])
            assert (t in ref["required"]) == RADIUS_WANT[a] and t not in ref["optional"] and not ref["near_radius"][t], (p, a, t in ref["required"], t in ref["optional"], ref["near_radius"][t], sorted(ref["optional"]))
            got.append("%+.1f" % ((want - RADIUS) / float(np.spacing(f32(50)))))
        texts.append("pass %d: targets at radius %s ulp" % (p, " ".join(got)))
    assert run.passes[0]["snaps"][0]["shape"][0, 1] == 223
    return "; ".join(texts)


# ------------------------------------------------------------------------------------------------------------------
# road_rows
# ------------------------------------------------------------------------------------------------------------------
HEADINGS = SC.HEADINGS
LENGTHS = (0.0, 0.005, 0.5, 6.0, 35.0)
BIG_ID = 2 ** 31 - 1


def _rows_world():
    """Segments of every polyline type along every heading of the step_wrap set (a segment along -y has the heading -pi / 2
    exactly, one along -x the heading pi), half lengths from a point to 35 m, two crosswalks, two speed bumps, three stop signs;
    ids 0 ... 2^31 - 1 and map_element_ids -1 ... 20 (and 4, 21 and -2, which the parser turns into -1)."""
    roads = []
    for i in range(27):
        cx, cy = SC.grid(i, 6, 11.0, 5)
        h, half = HEADINGS[i % 9], LENGTHS[(i // 2) % 5]
        if i % 9 == 5:                       # -pi / 2: straight down, dx exactly 0
            pts = [(cx, cy + half), (cx, cy - half)]
        elif i % 9 == 1:                     # pi: straight back, dy exactly 0
            pts = [(cx + half, cy), (cx - half, cy)]
        else:
            pts = GC.segment(cx, cy, h, half)
        roads.append(GC.road(i, KINDS[i % 3], pts))
    box = lambda cx, cy, lx, ly: [(cx - lx, cy - ly), (cx + lx, cy - ly), (cx + lx, cy + ly), (cx - lx, cy + ly)]
    roads += [GC.road(27, "crosswalk", box(-20.0, 31.0, 6.0, 2.0)), GC.road(28, "crosswalk", box(20.0, -31.0, 0.5, 9.0)),
              GC.road(29, "speed_bump", [(14.0, 30.0), (17.0, 31.0), (16.5, 32.5), (13.5, 31.5)]), GC.road(30, "speed_bump", box(0.0, 33.0, 0.2, 0.2)),
              GC.road(31, "stop_sign", [(-3.0, -29.0)]), GC.road(32, "stop_sign", [(33.0, 3.0)]), GC.road(33, "stop_sign", [(-36.0, 2.0)])]
    ids = (0, 1, 7, 255, 65536, 16777216, 16777217, BIG_ID)
    maps = (-1, 0, 1, 2, 3, 4, 5, 15, 19, 20, 21, -2)
    for i, r in enumerate(roads):
        r["id"], r["map_element_id"] = ids[i % len(ids)], maps[i % len(maps)]
    cars = [GC.car(a, SC.grid(a, 3, 17.0, 3)[0] + 1.3 + 0.21 * a, SC.grid(a, 3, 17.0, 3)[1] - 2.1 + 0.17 * a, HEADINGS[a]) for a in range(9)]
    return _world("rows", cars, roads)


def _rows_actions(run, k, before):
    """Step k turns agent a to heading (a + 3 (k + 1)) % 9 of the set and shifts it by 0.7 m."""
    act = run.hold_pose(before)
    for a in range(9):
        run.put(act, 0, a, x=before["state"][0, a, 0] + f32(0.7), y=before["state"][0, a, 1] + f32(0.2), yaw=HEADINGS[(a + 3 * (k + 1)) % 9])
    return act


def _rows_premise(run):
    snap = run.passes[0]["snaps"][0]
    R = int(snap["shape"][0, 1])
    m = snap["map_obs"][0, :R]
    assert R == 34 and set(m[:, 6].astype(int)) == {1, 2, 3, 4, 5, 6}
    assert m[:, 2].min() == 0 and m[:, 2].max() >= 34.9 and {0.0, float(f32(BIG_ID)), 16777216.0} <= set(m[:, 7].tolist())
    assert {-1.0, 0.0, 20.0} <= set(m[:, 8].tolist()) and m[:, 8].max() == 20 and m[:, 8].min() == -1
    assert (np.abs(m[:, 5] + PI / 2) < 1e-6).any() and (np.abs(np.abs(m[:, 5]) - PI) < 1e-6).any(), "headings -pi / 2 and +-pi: %s" % m[:, 5]
    seam = opposite = 0
    yaws = set()
    for p in range(len(run.passes)):
        for a in range(9):
            ref = run.ref(p, 0, a, RR.KNN)
            yaws.add(round(float(run.passes[p]["snaps"][0]["abs_obs"][0, a, 7]), 3))
            raw = m[:, 5].astype(f64) - float(GR.yaw_of(run.passes[p]["snaps"][0]["abs_obs"][0, a, 3:7]))
            seam += int((np.abs(raw) > PI).sum())
            opposite += int((np.abs(np.abs(ref["obs"][:, 5]) - PI) < 1e-6).sum())
            assert in_reach(ref) >= 24, in_reach(ref)
    assert seam >= 50 and opposite >= 4 and len(yaws) >= 7, (seam, opposite, yaws)
    return "34 roads of every type; %d heading differences beyond +-pi, %d exactly opposite; agent yaws %s" % (seam, opposite, sorted(yaws))


# ------------------------------------------------------------------------------------------------------------------
# road_ties
# ------------------------------------------------------------------------------------------------------------------
TIE_SIZES = (2, 16, 17, 31, 32, 33)


def _ties_world(g):
    """Three groups of g identical roads around an agent at the origin: one among the first K roads (3 m away), one among the
    later roads (4 m away: every member but the equal ones is an insert), one that straddles the K-th key (K - ceil(g / 2) roads are nearer), last in the
    index order -- and 300 roads on a straight line 10 ... 40 m out."""
    dup = lambda first, x, y: [GC.road(first + j, KINDS[j % 3] if g % 2 else "lane", GC.segment(x, y, 0.6, 0.5)) for j in range(g)]
    step = 0.13
    filler = line_points(300, step, x0=0.0, y0=10.0, first=1e-9)         # 10 ... 40.3 m from the origin, nearer first
    nearer = K - (g + 1) // 2 - 2 * g          # fillers nearer than the third group
    r3 = math.hypot(10.0, step * (nearer - 0.5))
    head = short_roads(filler[:150], first=1000)
    tail = short_roads(filler[150:], first=1150)
    # (the third group comes last: no insert follows it, so the heap keeps its members of the lowest indices, like set order)
    roads = head[:60] + dup(0, 3.0, 0.0) + head[60:] + tail[:60] + dup(100, 0.0, 4.0) + tail[60:] + dup(200, -r3 * 0.6, r3 * 0.8)
    cars = [GC.car(0, 0.02, 0.01, 0.4), GC.car(1, 3.0, -2.0, -1.0), GC.car(2, -20.0, 8.0, 2.5)]
    return _world("ties%d" % g, cars, roads)


def _ties_premise(run):
    texts = []
    for w, g in enumerate(TIE_SIZES):
        snap = run.passes[0]["snaps"][0]
        R = int(snap["shape"][w, 1])
        assert R == 300 + 3 * g
        ref = run.ref(0, w, 0, RR.KNN)
        keys = ref["keys"]
        uniq, counts = np.unique(keys, return_counts=True)
        assert sorted(counts[counts > 1].tolist()) == [g, g, g], (g, counts[counts > 1])
        kth = np.sort(keys)[K - 1]
        at_cut = int((keys == kth).sum())
        below = int((keys < kth).sum())
        assert at_cut == g and below < K < below + g, "the third group must straddle the K-th key: %d below, %d equal" % (below, at_cut)
        first = np.nonzero(keys == uniq[counts > 1][0])[0]
        assert first.max() < K and np.nonzero(keys == uniq[counts > 1][1])[0].min() >= K
        texts.append("%d-fold: %d nearer than the cut, %d of the group taken" % (g, below, K - below))
    return "; ".join(texts)


def _ties_gpu_premise(run, paths):
    if run.mode != "ref_order_rank":
        return ""
    seen = {g: sorted({int(v) for p in paths[1:] for v in p[w, :3]}) for w, g in enumerate(TIE_SIZES)}
    assert any(-12 in [int(v) for v in p[5, :3]] for p in paths), "33 roads with one key must raise -12: %s" % seen
    for w, g in enumerate(TIE_SIZES[:5]):
        assert all((p[w, :3] > 0).all() for p in paths[1:]), "%d equal keys must be ranked: %s" % (g, seen)
    return "paths per tie size %s" % seen


LONG_TIES = (16, 17)


def _long_ties_world(g):
    """The spiral of road_tiles with 1,400 roads -- every one an insert, a LONG candidate list -- and behind them g identical
    roads 2 m from the centre, nearer than all: g more inserts with one key.  A long list's rank counts 16 equal keys."""
    wd = _tiles_world(1400)
    dup = [GC.road(5000 + j, KINDS[j % 3], GC.segment(1.6, 1.2, 0.6, 0.5)) for j in range(g)]
    return _world("long_ties%d" % g, wd.scene["objects"], wd.scene["roads"] + dup)


def _long_ties_premise(run):
    texts = []
    for w, g in enumerate(LONG_TIES):
        for p in range(len(run.passes)):
            for a in range(2):
                ref = run.ref(p, w, a, RR.KNN)
                assert ref["R"] == 1400 + g and ref["inserts"] == 1400 + g - K, (p, w, a, ref["inserts"])
                uniq, counts = np.unique(ref["keys"], return_counts=True)
                assert counts.max() == g and (counts > 1).sum() == 1 and uniq[counts.argmax()] == ref["keys"].min(), "one %d-fold tie, the nearest key" % g
        texts.append("%d roads, all inserts, the nearest %d with one key" % (1400 + g, g))
    return "; ".join(texts)


def _long_ties_gpu_premise(run, paths):
    if run.mode != "ref_order_rank":
        return ""
    seen = {g: sorted({int(v) for p in paths[1:] for v in p[w, :2]}) for w, g in enumerate(LONG_TIES)}
    assert all((p[0, :2] == 1416).all() for p in paths[1:]), "16 equal keys on a long list are ranked: %s" % seen
    assert any((p[1, :2] == -12).any() for p in paths), "17 equal keys on a long list must raise -12: %s" % seen
    assert all(((p[1, :2] == -12) | (p[1, :2] == -13) | (p[1, :2] == -1)).all() for p in paths[1:]), seen
    return "paths per tie size on a long list %s" % seen


# ------------------------------------------------------------------------------------------------------------------
# road_tiles
# ------------------------------------------------------------------------------------------------------------------
TILES_A = (K + 32 * 3 - 1, K + 32 * 3, K + 32 * 3 + 1, 1271, 1272, 1273)
TILES_B = (K + 64 * 20 - 1, K + 64 * 20, K + 64 * 20 + 1, 2551, 2552, 2553)


def _tiles_world(n):
    """n roads along an inward spiral, ordered by DECREASING distance from the centre: for an agent near the centre every road
    behind the first K is an insert, so its candidate list holds all n."""
    pts = [((4.0 + 44.0 * (n - i) / n) * math.cos(0.045 * i), (4.0 + 44.0 * (n - i) / n) * math.sin(0.045 * i)) for i in range(n + 1)]
    cars = [GC.car(0, 0.05, 0.02, 0.3), GC.car(1, -0.06, 0.04, -2.0)]      # (0.045 rad a road: within 0.19 m of the centre the distances fall road by road)
    return _world("tiles%d" % n, cars, chain_roads(pts, per=97))


def _tiles_actions(run, k, before):
    act = run.hold_pose(before)
    for w, a in run.agents():
        s = f32(0.04) if (a + k) % 2 == 0 else f32(-0.03)
        run.put(act, w, a, x=before["state"][w, a, 0] + s, y=before["state"][w, a, 1] - s, yaw=run.yaw[w, a] + f32(0.02))
    return act


def _tiles_premise(sizes):
    def premise(run):
        shape = run.passes[0]["snaps"][0]["shape"]
        assert shape[:, 1].tolist() == list(sizes), shape[:, 1]
        for p in range(len(run.passes)):
            for w, a in run.agents():
                ref = run.ref(p, w, a, RR.KNN)
                assert ref["inserts"] == ref["R"] - K, "pass %d world %d agent %d: %d of %d later roads are inserts" % (p, w, a, ref["inserts"], ref["R"] - K)
        moved = min(np.abs(b["state"][:, :2, 0:2] - a["state"][:, :2, 0:2]).max(-1).min() for a, b in zip(run.passes, run.passes[1:]))
        assert moved >= 0.029, moved
        return "roads per world %s: every later road is an insert for every agent on every pass; the agents move" % (list(sizes),)
    return premise


def _tiles_gpu_premise(sizes):
    def premise(run, paths):
        if run.mode != "ref_order_rank":
            return ""
        seen = {n: sorted({int(v) for p in paths[1:] for v in p[w, :2]}) for w, n in enumerate(sizes)}
        for w, n in enumerate(sizes):
            for p in paths[1:]:
                if n <= 2552:
                    assert (p[w, :2] == n).all(), "world of %d roads: candidate counts %s" % (n, seen)
                else:
                    assert ((p[w, :2] == -11) | (p[w, :2] == -13)).all(), "world of %d roads: %s" % (n, seen)
        assert any(n > 2552 for n in sizes) == any(-11 in v for v in seen.values())
        return "candidate counts / paths per world %s" % seen
    return premise


# ------------------------------------------------------------------------------------------------------------------
# road_jump
# ------------------------------------------------------------------------------------------------------------------
def _scatter(n, half_x, half_y, seed, x0=0.0, y0=0.0):
    rng = np.random.default_rng(seed)
    pts, (x, y, th) = [], (x0, y0, 0.0)
    while len(pts) < n + 1:
        if len(pts) % 40 == 0:
            x, y, th = x0 + rng.uniform(-half_x, half_x), y0 + rng.uniform(-half_y, half_y), rng.uniform(-PI, PI)
        th += rng.normal(0.0, 0.4)
        step = rng.uniform(1.5, 4.0)
        x, y = min(max(x + step * math.cos(th), x0 - half_x), x0 + half_x), min(max(y + step * math.sin(th), y0 - half_y), y0 + half_y)
        pts.append((x, y))
    return pts


JUMP_ANGLE = 0.3
JUMP_START = ((-60.0, 5.0), (-58.0, -8.0), (70.0, 10.0), (0.0, 3.0), (30.0, -20.0), (-30.0, 25.0), (90.0, 15.0))      # (along, left of) the line


def _jump_world():
    cars = [GC.car(a, *on_line(t + 0.071 + 0.013 * a, h - 0.007 * a, JUMP_ANGLE), 0.5 * a - 1.5) for a, (t, h) in enumerate(JUMP_START)]
    return _world("jump", cars, line_roads(900, 0.25, 21, angle=JUMP_ANGLE), span=1500.0)


def _jump_moves(k):
    """Per step, agent: (dx, dy).  0: 0.5 m a step.  1: 30 m a step along the roads.  2: 500 m out of the road box and back.  3 and 4
    swap places.  5 jumps onto a spot 2 m from where agent 3 stood (whose checkpoints it must borrow), 6: 130 m to where nobody was."""
    along = on_line(30.0, 2.0 if k % 2 == 0 else -2.0, JUMP_ANGLE)
    return {0: (0.5, 0.0), 1: along, 2: (500.0 if k % 2 == 0 else -500.0, 0.0)}


def _jump_actions(run, k, before):
    act = run.hold_pose(before)
    st = before["state"]
    for a, (dx, dy) in _jump_moves(k).items():
        run.put(act, 0, a, x=st[0, a, 0] + f32(dx), y=st[0, a, 1] + f32(dy), yaw=run.yaw[0, a] + f32(0.1))
    run.put(act, 0, 3, x=st[0, 4, 0], y=st[0, 4, 1])
    run.put(act, 0, 4, x=st[0, 3, 0], y=st[0, 3, 1])
    if k == 1:
        run.put(act, 0, 5, x=st[0, 3, 0] + f32(1.5), y=st[0, 3, 1] - f32(1.0))
    if k == 2:
        run.put(act, 0, 6, x=st[0, 6, 0] - f32(125.0), y=st[0, 6, 1] - f32(45.0))
    return act


def bound_source(run, p, w, a, reach=6.0):
    """Which bound the rank path's rule gives agent (w, a) in step pass p: "own" (it moved at most `reach` from where its
    previous selection was made, or from the episode's first), "borrowed" (another agent's previous selection was made within
    `reach` of where it is now) or "fresh"."""
    now = run.passes[p]["state"][w, a, 0:2].astype(f64)
    prev, first = run.passes[p - 1]["state"][w, :, 0:2].astype(f64), run.passes[0]["state"][w, :, 0:2].astype(f64)
    if min(np.hypot(*(now - prev[a])), np.hypot(*(now - first[a]))) <= reach:
        return "own"
    others = np.hypot(prev[:run.case.worlds[w].n, 0] - now[0], prev[:run.case.worlds[w].n, 1] - now[1])
    return "borrowed" if others.min() <= reach else "fresh"


def _jump_premise(run):
    seen = {}
    for p in range(1, len(run.passes)):
        for a in range(7):
            seen.setdefault(bound_source(run, p, 0, a), []).append((p, a))
    moved = [float(np.hypot(*(run.passes[1]["state"][0, a, 0:2] - run.passes[0]["state"][0, a, 0:2]))) for a in range(3)]
    assert abs(moved[0] - 0.5) < 1e-3 and 30 <= moved[1] < 30.2 and abs(moved[2] - 500) < 1e-2, moved
    assert in_reach(run.ref(1, 0, 2, RR.KNN)) == 0 and in_reach(run.ref(2, 0, 2, RR.KNN)) > K, "out of the road box and back"
    assert np.array_equal(run.passes[1]["state"][0, 3, 0:2], run.passes[0]["state"][0, 4, 0:2]), "agents 3 and 4 swap places"
    assert (2, 5) in seen.get("borrowed", []) and (3, 6) in seen.get("fresh", []) and len(seen.get("own", [])) >= 3, seen
    assert run.passes[0]["snaps"][0]["shape"][0, 1] == 900
    return "moves of %.1f, %.1f and %.1f m a step; bounds: %s" % (moved[0], moved[1], moved[2], {k: len(v) for k, v in seen.items()})


def _jump_gpu_premise(run, paths):
    if run.mode != "ref_order_rank":
        return ""
    assert paths[1][0, 2] == -3 and paths[2][0, 2] > 0, "agent 2 leaves the road box and comes back: %s" % [p[0, 2] for p in paths]
    for p in range(1, len(paths)):
        live = [a for a in range(7) if not (a == 2 and p % 2 == 1)]
        assert (paths[p][0, live] > 0).all(), "step %d: every agent in reach is ranked, whatever its bound: %s" % (p, paths[p][0, :7])
    return "paths per pass %s" % [p[0, :7].tolist() for p in paths]


# ------------------------------------------------------------------------------------------------------------------
# road_fast
# ------------------------------------------------------------------------------------------------------------------
def _fast_world(parked):
    """Agents at 60 m/s under the Classic model (zero action: they keep their speed and heading) along and across a dense line of
    roads, alone or next to parked cars."""
    cars, vel = [], []
    for a, (x, y, h) in enumerate(((-45.0, -20.0, 0.0), (40.0, 25.0, PI), (-20.0, -40.0, 1.2), (10.0, 45.0, -1.9))):
        cars.append(SC.with_goal(GC.car(a, x, y, h), x + 600.0 * math.cos(h), y + 600.0 * math.sin(h)))
        vel.append((60.0 * math.cos(h), 60.0 * math.sin(h), 0.0))
    if parked:
        for a, (x, y) in enumerate(((-30.0, -17.0), (0.0, 3.0), (25.0, 22.0), (5.0, -30.0))):
            cars.append(CC.parked(4 + a, x, y, 0.7 * a))
            vel.append((0.0, 0.0, 0.0))
    return _world("fast_parked" if parked else "fast", cars, line_roads(1200, 0.25, 31 + parked, angle=0.05), span=1500.0, vel=vel)


def _fast_actions(run, k, before):
    return _blank(run)


def _fast_premise(run):
    for w, wd in enumerate(run.case.worlds):
        first, last = run.passes[0]["state"][w, :4, 0:2], run.passes[-1]["state"][w, :4, 0:2]
        d = np.hypot(*(last - first).T)
        assert (np.abs(d - 60.0) < 0.1).all(), "60 m/s for 10 steps: %s" % d
        step = np.hypot(*(run.passes[2]["state"][w, :4, 0:2] - run.passes[1]["state"][w, :4, 0:2]).T)
        assert (np.abs(step - 6.0) < 0.01).all(), step
        assert in_reach(run.ref(1, w, 0, RR.KNN)) > K
        if wd.n > 4:
            assert np.array_equal(run.passes[0]["state"][w, 4:8, 0:2], run.passes[-1]["state"][w, 4:8, 0:2]), "the parked cars stay"
    return "4 agents at 6 m a step along and across 1200 roads, alone and next to 4 parked cars"


def _fast_gpu_premise(run, paths):
    if run.mode != "ref_order_rank":
        return ""
    assert all((p[:, :4] > 0).all() for p in paths[1:]), [p[:, :4].tolist() for p in paths]
    return "candidate counts %d ... %d" % (min(int(p[:, :4].min()) for p in paths[1:]), max(int(p[:, :4].max()) for p in paths[1:]))


# ------------------------------------------------------------------------------------------------------------------
# road_stamp
# ------------------------------------------------------------------------------------------------------------------
def _stamp_world(name, seed, angle, y0):
    cars = [GC.car(0, -20.0, -10.0, 0.4), GC.car(1, 15.0, 12.0, -2.2), CC.parked(2, 0.0, 0.0, 1.0), CC.parked(3, 30.0, -25.0, 2.0), GC.car(4, -35.0, 30.0, 0.0)]
    return _world(name, cars, line_roads(500, 0.25, seed, angle=angle, x0=0.07, y0=y0))


def _stamp_actions(run, k, before):
    """Agent 0 leaves at step 1 and is handed its first pose back, bit for bit, at step 2; agent 1 is handed its pose back all
    along; agent 4 moves every step; the parked cars are nobody's to move."""
    act = run.hold_pose(before)
    st = before["state"]
    if k == 0:
        run.home = (st[0, 0, 0], st[0, 0, 1], run.yaw[0, 0])
        run.put(act, 0, 0, x=st[0, 0, 0] + f32(17.0), y=st[0, 0, 1] - f32(9.0), yaw=1.3)
    if k == 1:
        act[0, 0, 0], act[0, 0, 1], act[0, 0, 3] = run.home
        run.yaw[0, 0] = run.home[2]
    run.put(act, 0, 4, x=st[0, 4, 0] + f32(0.6), y=st[0, 4, 1] - f32(0.1))
    return act


def _stamp_set_maps(run):
    """The same poses, another world's roads: no row may be left in place."""
    st = run.passes[-1]["state"]
    for s in run.sims:
        s.set_maps([run.scene_paths[1]])
        SC._set_state(s, st)
        s.reset([])
    return "set_maps behind step 3"


def _stamp_premise(run):
    s = [p["state"][0] for p in run.passes]
    assert np.array_equal(s[0][0, :7].view(np.uint32), s[2][0, :7].view(np.uint32)) and not np.array_equal(s[0][0, :2], s[1][0, :2]), "agent 0 leaves and comes back"
    assert all(np.array_equal(s[0][[1, 2, 3], :7].view(np.uint32), v[[1, 2, 3], :7].view(np.uint32)) for v in s[1:4]), "agents 1, 2, 3 keep their pose bits"
    a, b = run.passes[3]["snaps"][0], run.passes[4]["snaps"][0]
    assert np.array_equal(a["abs_obs"][0, :5, 0:7].view(np.uint32), b["abs_obs"][0, :5, 0:7].view(np.uint32)), "set_maps keeps the poses"
    assert not np.array_equal(a["map_obs"], b["map_obs"]) and not np.array_equal(a["rows"][0, 1], b["rows"][0, 1])
    return "agent 0 back on the bit-identical pose at step 2; agents 1-3 never move; set_maps swaps the roads under the same poses"


def _stamp_gpu_premise(run, paths):
    left = run.sims[1].stat(30)
    assert left > 0, "no road rows were left in place: the pose stamps did not take"
    return "%d agent rows left in place (gd_stat 30)" % left


# ------------------------------------------------------------------------------------------------------------------
# road_blocks (linear)
# ------------------------------------------------------------------------------------------------------------------
def _blocks_worlds():
    """Linear mode culls blocks of 16 roads by their bounding circles.  b15 / b16 / b17: that many roads.  bcut: 16-road blocks of
    which the agent at the origin reaches 12 whole ones and, of the 13th, the first 8 (K binds in the middle of a block: agent 0),
    all 16 (the K-th road in reach is the last of a block: agent 1, who reaches one road less before it) ... ; every 5th block
    spans the end of one polyline near the agents and the start of one 3 km away."""
    cars = lambda: [GC.car(0, 0.3, 0.2, 0.5), GC.car(1, 6.0, -4.0, -1.0), GC.car(2, -9.0, 7.0, 2.0)]
    near = spiral(400, 2.0, 0.1)
    worlds = [_world("b%d" % n, cars(), short_roads(spiral(n, 5.0, 2.5))) for n in (15, 16, 17)]
    roads = []
    for b in range(25):
        block = near[16 * b:16 * b + 16]
        if b % 5 == 4:                  # half near, half kilometres away
            block = block[:8] + [(3000.0 + x, 2000.0 + y) for x, y in block[8:]]
        roads += short_roads(block, first=16 * b)
    worlds.append(_world("bcut", cars(), roads, span=1500.0))
    # an agent for whom the K-th road in reach is the first / the last road of a block: 13 roads out of reach at the front
    front = [(70.0 + x, 0.0 + y) for x, y in spiral(13, 1.0, 0.3)]
    worlds.append(_world("blast", cars(), short_roads(front[:8] + near[:392])))       # in reach: roads 8 ..., the 200th is road 207 = 12 * 16 + 15
    worlds.append(_world("bfirst", cars(), short_roads(front[:9] + near[:391])))      # the 200th is road 208 = 13 * 16 + 0
    return worlds


def _blocks_premise(run):
    shape = run.passes[0]["snaps"][0]["shape"]
    assert shape[:, 1].tolist() == [15, 16, 17, 400, 400, 400]
    cut = {}
    for w in (3, 4, 5):
        for a in range(3):
            ref = run.ref(0, w, a, RR.LINEAR)
            order = ref["order"]
            assert (order >= 0).all(), "K binds: world %d agent %d has %d rows" % (w, a, int((order >= 0).sum()))
            cut[(w, a)] = int(order[-1]) % 16
            assert int((ref["dist"] <= RADIUS).sum()) > K
    assert cut[(4, 0)] == 15 and cut[(5, 0)] == 0 and 0 < cut[(3, 0)] < 15, cut
    m = run.passes[0]["snaps"][0]["map_obs"][3, :400]
    spans = [b for b in range(25) if np.ptp(m[16 * b:16 * b + 16, 0]) > 1000]
    assert len(spans) == 5
    return "15 / 16 / 17 roads; the K-th road in reach is road %% 16 = %s; blocks %s span polylines 3 km apart" % (cut, spans)


# ------------------------------------------------------------------------------------------------------------------
# road_cells (set order)
# ------------------------------------------------------------------------------------------------------------------
def _cells_worlds():
    cars = lambda: [GC.car(0, 0.0, 0.0, 0.3), GC.car(1, 16.0, 16.0, -1.2), GC.car(2, -32.0, 8.0, 2.2), GC.car(3, 40.0, -24.0, 0.9)]
    base = chain_roads(_scatter(700, 80.0, 60.0, 41), per=40)
    outlier = base + [GC.road(900, "stop_sign", [(5000.0, -4000.0)])]
    point = [GC.road(j, "stop_sign", [(12.0, 9.0)]) for j in range(260)]
    return [_world("cells", cars(), base), _world("cells_outlier", cars(), outlier, span=1500.0), _world("cells_point", cars(), point)]


def _cells_actions(run, k, before):
    """Steps 1 and 2: small moves (bounded selections); step 3: agent 0 of every world jumps 90 m; step 4: small moves again."""
    act = run.hold_pose(before)
    st = before["state"]
    for w, a in run.agents():
        if k == 2 and a == 0:
            run.put(act, w, a, x=st[w, a, 0] + f32(64.0), y=st[w, a, 1] - f32(48.0))
        elif a != 3:
            run.put(act, w, a, x=st[w, a, 0] + f32(0.3), y=st[w, a, 1] + f32(0.2), yaw=run.yaw[w, a] + f32(0.03))
    if k == 0:      # agent 3 of world 0 goes onto a corner of the 16 m grid the set-order kernel lays over the roads
        R = int(before["shape"][0, 1])
        lo = before["map_obs"][0, :R, 0:2].min(0)
        run.put(act, 0, 3, x=f32(lo[0] + f32(80.0)), y=f32(lo[1] + f32(48.0)))
    return act


def _cells_premise(run):
    shape = run.passes[0]["snaps"][0]["shape"]
    assert shape[:, 1].tolist() == [700, 701, 260]
    m = run.passes[0]["snaps"][0]["map_obs"]
    assert np.abs(m[1, :701, 0]).max() > 4000 and np.ptp(m[2, :260, 0]) == 0 and np.ptp(m[2, :260, 1]) == 0
    ref = run.ref(0, 2, 0, RR.SET)
    assert sorted(ref["required"]) == list(range(K)), "every road at one point: the K lowest indices"
    lo = m[0, :700, 0:2].min(0)
    cell = (run.passes[1]["state"][0, 3, 0:2] - lo) * f32(1.0 / 16.0)          # (float32, like the kernel's own cell index)
    assert cell.dtype == f32 and cell.tolist() == [5.0, 3.0], "agent 3 must stand on a grid corner: %s" % cell
    jump = np.hypot(*(run.passes[3]["state"][:, 0, 0:2] - run.passes[2]["state"][:, 0, 0:2]).T)
    assert (np.abs(jump - 80.0) < 1e-3).all(), jump
    return "700 roads, the same with an outlier 6 km away, 260 roads at one point (the K lowest indices are taken); a jump of 80 m at step 3"


# ------------------------------------------------------------------------------------------------------------------
# road_return
# ------------------------------------------------------------------------------------------------------------------
def _return_world(name, seed):
    """0: a logged agent (expert) whose log is invalid at index 1 and goes on 75 m away at index 2 (step 3).  1, 2: within their goal thresholds at
    step 1 (they arrive, go to the padding position at step 2 and come back with the world's reset).  3: driven onto the parked 4
    at step 1 (AgentRemoved: both go to the padding position).  5: drives on."""
    k = np.arange(91)
    valid = np.ones(91, bool)
    valid[1] = False
    xs = np.where(k < 2, -40.0 + 0.5 * k, 20.0 + 0.5 * k)
    logged = SC.moving_car(0, xs, np.where(k < 2, -20.0, 25.0) + 0.0 * k, [0.2] * 91, [5.0] * 91, [0.0] * 91, valid=valid, expert=True)
    cars = [logged, SC.with_goal(GC.car(1, 10.0, 10.0, 0.5), 11.0, 10.0), SC.with_goal(GC.car(2, -15.0, 30.0, -2.0), -15.5, 30.5),
            GC.car(3, 30.0, -30.0, 1.0), CC.parked(4, 30.0, -22.0, 0.3), GC.car(5, -45.06, 40.0, 2.8)]
    return _world(name, cars, line_roads(600, 0.25, seed, angle=0.1, kinds=("lane", "road_line")))      # (no edge to hit)


def _return_cluster_world():
    """260 roads 3 cm apart on a line through the origin, and three agents about 40 m out on its extension: every key lies
    between 36^2 and 47^2, less than 1.5 times any K-th key a bound can have been recorded with (`jumped_for_certain`).  0 is
    shifted every step; 1 is logged and goes on 81 m away, on the other side, at index 2; 2 stands."""
    k = np.arange(91)
    valid = np.ones(91, bool)
    valid[1] = False
    logged = SC.moving_car(1, np.where(k < 2, -40.0, 41.0) + 0.1 * k, np.where(k < 2, 5.0, -6.0) + 0.0 * k, [2.9] * 91, [1.0] * 91, [0.0] * 91,
                           valid=valid, expert=True)
    cars = [GC.car(0, 40.0, 3.0, 0.4), logged, GC.car(2, -41.0, -4.0, -0.7)]
    return _world("return_c", cars, line_roads(260, 0.03, 63, kinds=("lane", "road_line")))


def _return_actions(run, k, before):
    act = run.hold_pose(before)
    st = before["state"]
    run.put(act, 2, 0, x=st[2, 0, 0] + f32(0.5), y=st[2, 0, 1] - f32(0.2))
    for w in range(2):
        if k == 0:
            act[w, 3, 0:3] = st[w, 4, 0:3]
            act[w, 3, 3] = run.yaw[w, 3] = run.yaw[w, 4]
        if st[w, 5, 2] != CR.PAD_Z:
            run.put(act, w, 5, x=st[w, 5, 0] + f32(0.8), y=st[w, 5, 1] - f32(0.4))
    return act


def _return_reset(run):
    """World 0 is reset; world 1 keeps stepping."""
    for s in run.sims:
        s.reset([0])
    for w in (0,):
        run.yaw[w, :run.case.worlds[w].n] = run.case.worlds[w].yaw
    return "reset of world 0 behind step 3"


def kth_key(run, p, w, x, y, k=K):
    """The K-th smallest squared distance from (x, y) to the roads world w exports in pass p."""
    snap = run.passes[p]["snaps"][0]
    m = snap["map_obs"][w, :int(snap["shape"][w, 1]), 0:2].astype(f64)
    return float(np.sort((m[:, 0] - x) ** 2 + (m[:, 1] - y) ** 2)[k - 1])


def jumped_for_certain(run, p, w, a):
    """k_knn_rank lays its ranking buckets between the smallest and the largest candidate key -- its `jumped` rule -- when fewer
    than a quarter of the candidates, or ALL of them, lie below 1.5 x t_last, the last K-th key of the checkpoints that bound the
    selection.  Which checkpoints those are (the agent's own of the previous selection or of the episode's first, a neighbour's, a
    fresh bound) and the candidate list are the engine's own; but t_last is never below the K-th key at the place its checkpoints
    were recorded, and a candidate is a road.  So the rule is taken FOR CERTAIN when every road's key now lies below 1.5 x the
    smallest K-th key over every place a bound can come from: where the agent is, and where any agent of the world stood in the
    previous and in the first pass (1 % apart, for the kernel's float32)."""
    n = run.case.worlds[w].n
    now = run.passes[p]["state"][w, a, 0:2].astype(f64)
    snap = run.passes[p]["snaps"][0]
    m = snap["map_obs"][w, :int(snap["shape"][w, 1]), 0:2].astype(f64)
    largest = float(((m[:, 0] - now[0]) ** 2 + (m[:, 1] - now[1]) ** 2).max())
    places = [now] + [run.passes[q]["state"][w, b, 0:2].astype(f64) for q in (p - 1, 0) for b in range(n)]
    return largest * 1.01 < 1.5 * min(kth_key(run, p, w, x, y) for x, y in places if x > -10000)


def _return_premise(run):
    pad = lambda p, w: (run.passes[p]["state"][w, :6, 2] == CR.PAD_Z)
    # passes: 0 reset pass, 1-3 steps, 4 the reset of world 0, 5-6 steps
    assert pad(2, 0)[[1, 2, 3, 4]].all() and pad(2, 1)[[1, 2, 3, 4]].all(), "arrived and removed agents stand at the padding position: %s" % pad(2, 0)
    assert not pad(4, 0).any() and pad(4, 1)[[1, 2, 3, 4]].all() and pad(6, 1)[[1, 2]].all(), "the reset brings world 0 back, world 1 keeps stepping"
    x = [float(p["state"][1, 0, 0]) for p in run.passes]
    jumps = [abs(b - a) for a, b in zip(x, x[1:])]
    assert max(jumps) > 50, "the logged agent comes back elsewhere: %s" % x
    assert in_reach(run.ref(2, 0, 1, RR.KNN)) == 0 and in_reach(run.ref(4, 0, 1, RR.KNN)) > K
    certain = [(p, a) for p in range(1, len(run.passes)) if not run.passes[p]["reset"] for a in range(3) if jumped_for_certain(run, p, 2, a)]
    assert len(certain) >= 10 and (3, 1) in certain, "the `jumped` rule is certain for %s" % certain
    hop = float(np.hypot(*(run.passes[3]["state"][2, 1, 0:2] - run.passes[2]["state"][2, 1, 0:2])))
    assert hop > 80, hop
    return "4 agents per world at the padding position after step 2, back after the reset of world 0 alone; the logged agent's x: %s; " \
        "beside the cluster of 260 roads the `jumped` bucket rule is certain on %d agent-steps, the logged agent's %.0f m hop among them" % (
            [round(v, 1) for v in x], len(certain), hop)


def _return_gpu_premise(run, paths):
    """passes: 0 reset pass, 1-3 steps, 4 the reset of world 0, 5-6 steps."""
    if run.mode != "ref_order_rank":
        return ""
    assert (paths[2][:2, 1:5] == -3).all(), "at the padding position: %s" % paths[2][:2, :6]
    for p in (4, 5, 6):
        back = [0, 3, 4, 5] if p == 6 else range(6)        # (1 and 2 arrive again at step 4 and are gone again after step 5)
        assert (paths[p][0, back] > 0).all(), "pass %d: the agents the reset brought back are ranked: %s" % (p, paths[p][0, :6])
        assert (paths[p][1, 1:5] == -3).all() and paths[p][1, 0] > 0, paths[p][1, :6]
    assert (paths[6][0, 1:3] == -3).all(), paths[6][0, :6]
    assert paths[3][0, 0] > 0 and paths[3][1, 0] > 0, "the logged agent is ranked where it comes back"
    for p in (1, 2, 3, 5, 6):
        assert (paths[p][2, :3] > 0).all(), "pass %d: ranked where the `jumped` rule is certain: %s" % (p, paths[p][2, :3])
    return "returned agents ranked: world 0 %s after its reset; beside the cluster %s" % (paths[4][0, :6].tolist(), [paths[p][2, :3].tolist() for p in (1, 3, 6)])


# ------------------------------------------------------------------------------------------------------------------
# road_slots128
# ------------------------------------------------------------------------------------------------------------------
def _slots_worlds():
    cars = [GC.car(i, SC.grid(i, 16, 9.0, 8)[0] + 0.013 * i, SC.grid(i, 16, 9.0, 8)[1] - 0.007 * i, 0.37 * i - 3.0) for i in range(128)]
    small = [GC.car(i, -5.0 + 5.0 * i, 2.0 * i, 0.8 * i) for i in range(3)]
    return [_world("slots128", cars, line_roads(480, 0.3, 51, angle=0.02)), _world("ragged", small, line_roads(240, 0.3, 52, angle=1.0))]


def _slots_premise(run):
    shape = run.passes[0]["snaps"][0]["shape"]
    assert shape.tolist() == [[128, 480], [3, 240]]
    return "128 live slots and 480 roads beside 3 agents and 240 roads"


# ------------------------------------------------------------------------------------------------------------------
CASE_LIST = [
    Case("road_counts", _counts_worlds(), SR.STATE, _shift_actions, _counts_premise, steps=2, gpu_premise=_counts_gpu_premise),
    Case("road_radius", [_radius_world()], SR.STATE, _radius_actions, _radius_premise, steps=3),
    Case("road_rows", [_rows_world()], SR.STATE, _rows_actions, _rows_premise, steps=2),
    Case("road_ties", [_ties_world(g) for g in TIE_SIZES], SR.STATE, _shift_actions, _ties_premise, steps=4, modes=KNN_MODES, gpu_premise=_ties_gpu_premise),
    Case("road_tiles_a", [_tiles_world(n) for n in TILES_A], SR.STATE, _tiles_actions, _tiles_premise(TILES_A), steps=2,
         modes=("ref_order_rank", "ref_order_history"), gpu_premise=_tiles_gpu_premise(TILES_A)),
    Case("road_tiles_b", [_tiles_world(n) for n in TILES_B], SR.STATE, _tiles_actions, _tiles_premise(TILES_B), steps=4,
         modes=("ref_order_rank", "ref_order_history"), gpu_premise=_tiles_gpu_premise(TILES_B)),
    Case("road_ties_long", [_long_ties_world(g) for g in LONG_TIES], SR.STATE, _tiles_actions, _long_ties_premise, steps=2,
         modes=("ref_order_rank", "ref_order_history"), gpu_premise=_long_ties_gpu_premise),
    Case("road_jump", [_jump_world()], SR.STATE, _jump_actions, _jump_premise, steps=4, gpu_premise=_jump_gpu_premise),
    Case("road_fast", [_fast_world(False), _fast_world(True)], SR.CLASSIC, _fast_actions, _fast_premise, steps=10, gpu_premise=_fast_gpu_premise),
    Case("road_return", [_return_world("return_a", 61), _return_world("return_b", 61), _return_cluster_world()], SR.STATE, _return_actions, _return_premise, steps=5,
         gpu_premise=_return_gpu_premise,
         behaviour=CR.AGENT_REMOVED, events={2: _return_reset}),
    Case("road_stamp", [_stamp_world("stamp", 71, 0.2, 1.3)], SR.STATE, _stamp_actions, _stamp_premise, steps=5, events={2: _stamp_set_maps},
         gpu_premise=_stamp_gpu_premise),
    Case("road_blocks", _blocks_worlds(), SR.STATE, _shift_actions, _blocks_premise, steps=2, modes=("linear",)),
    Case("road_cells", _cells_worlds(), SR.STATE, _cells_actions, _cells_premise, steps=4, modes=("set_order_fused", "set_order_row_kernel")),
    Case("road_slots128", _slots_worlds(), SR.STATE, _shift_actions, _slots_premise, steps=1, slots=128),
]
CASES = {c.name: c for c in CASE_LIST}
STAMP_OTHER = _stamp_world("stamp_other", 72, -0.4, 6.0)          # the world road_stamp's set_maps loads under the same poses
PACKED = ("road_counts", "road_jump", "road_ties")      # run once more with the direct pack attached (reference order, rank path)
ALL_RUNS = [(c.name, m) for c in CASE_LIST for m in c.modes]


def write_scenes(case, directory):
    """The case's scene files; for road_stamp also the world its set_maps loads."""
    paths = case.write(directory)
    if case.name == "road_stamp":
        import json
        import os
        other = os.path.join(str(directory), "stamp_other.json")
        with open(other, "w") as f:
            json.dump(STAMP_OTHER.scene, f)
        paths = paths + [other]
    return paths


# ------------------------------------------------------------------------------------------------------------------
# comparison with the reference
# ------------------------------------------------------------------------------------------------------------------
EXACT_COLS = [2, 3, 4, 6, 7, 8]


def _match(got, obs, allowed, bx, by, bh):
    """Each row of got [n, 9] to a distinct road of `allowed` whose reference row it is: exact columns equal, x, y and heading
    within the bounds; the lowest free index (identical rows are interchangeable).  -1 where there is none."""
    allowed = np.asarray(sorted(allowed), np.int64)
    out = np.full(len(got), -1, np.int64)
    if not len(allowed) or not len(got):
        return out
    cand = obs[allowed]
    ok = (np.abs(got[:, None, 0] - cand[None, :, 0]) <= bx) & (np.abs(got[:, None, 1] - cand[None, :, 1]) <= by)
    ok &= (got[:, None, EXACT_COLS] == cand[None, :, EXACT_COLS].astype(f32).astype(f64)).all(-1)
    ok &= RR.angular_distance(got[:, None, 5], cand[None, :, 5]) <= bh
    used = np.zeros(len(allowed), bool)
    for i in range(len(got)):
        free = np.nonzero(ok[i] & ~used)[0]
        if len(free):
            used[free[0]] = True
            out[i] = allowed[free[0]]
    return out


def _rows_in_order(ref, n):
    """The order comparison: row i is the reference's row i.  Returns (road index per row, what is wrong or None)."""
    idx = ref["order"][ref["order"] >= 0]
    return idx, None if len(idx) == n else "%d rows, the reference has %d" % (n, len(idx))


def _rows_as_set(got, ref, loose, b, exact_count):
    """The set comparison: every row is a distinct selected road's row, every required road has one, and -- for an agent
    without a marginal road -- there is no row more.  loose: roads that may stand in for each other (a tie across the cut)."""
    idx = _match(got, ref["obs"], ref["required"] | ref["optional"] | loose, b["x"], b["y"], b["heading"])
    if (idx < 0).any():
        return idx, "row %d is no selected road's row" % int(np.nonzero(idx < 0)[0][0])
    missing = ref["required"] - loose - set(idx.tolist())
    if missing or (exact_count and len(got) != len(ref["required"])):
        return idx, "%d rows; selected roads %s are missing" % (len(got), sorted(missing)[:6])
    return idx, None


def errors(run, p, factor, mode=None, variant=None, sim=0, heap_rows=False, only=None):
    """Simulator `sim`'s rows after pass p against the reference of its own tensors.  Returns dict(err: {(span, column): largest
    float difference}, bad: [texts of what differs beyond the floats], agents, marginal, undecided).  heap_rows: the rows are a
    reference-order simulator's, compared as a set with the set-order reference: where a tie straddles the K-th key the heap
    keeps the members its history left, not those of the lowest indices (the one documented difference), and
    any of them is taken.  only: the (world, agent) pairs to look at."""
    case = run.case
    mode = mode or MODES[run.mode][0]
    out = dict(err={}, bad=[], agents=0, marginal=0, undecided=0)
    snap = run.passes[p]["snaps"][sim]
    for w, a in run.agents():
        if only is not None and (w, a) not in only:
            continue
        span = case.worlds[w].span
        b = {c: factor * v for c, v in ORACLE_ROAD_MAX[span].items()}
        ref = run.ref(p, w, a, mode, factor, variant, sim)
        base = ref if variant is None else run.ref(p, w, a, mode, factor, None, sim)     # (margins are the true rule's)
        got = snap["rows"][w, a].astype(f64)
        out["agents"] += 1
        out["marginal"] += base["marginal"]
        undecided = mode == RR.KNN and not base["decided"]
        out["undecided"] += undecided and not base["marginal"]
        real = got[:, 6] != 0
        n = int(real.sum())
        where = "world %d agent %d" % (w, a)
        if not real[:n].all():
            out["bad"].append("%s: padding rows among the real rows" % where)
            continue
        if not np.array_equal(got[n:], np.tile(ref["pad"], (RR.K - n, 1))):
            out["bad"].append("%s: the padding rows are not %s" % (where, ref["pad"].tolist()))
            continue
        if mode != RR.SET and not base["marginal"] and not undecided:
            idx, bad = _rows_in_order(ref, n)
        else:
            loose = ref["cut_ties"] if heap_rows and mode == RR.SET else set()
            idx, bad = _rows_as_set(got[:n], ref, loose, b, exact_count=not base["marginal"])
        if bad:
            out["bad"].append("%s: %s" % (where, bad))
            continue
        want = ref["obs"][idx]
        exact = got[:n][:, EXACT_COLS] != want[:, EXACT_COLS].astype(f32).astype(f64)
        if exact.any():
            out["bad"].append("%s: row %d: scale / type / id / mapType differ from road %d's" % (where, int(np.nonzero(exact.any(-1))[0][0]), int(idx[np.nonzero(exact.any(-1))[0][0]])))
            continue

        def put(col, v):
            if len(v):
                out["err"][(span, col)] = max(out["err"].get((span, col), 0.0), float(np.max(v)))
        put("x", np.abs(got[:n, 0] - want[:, 0]))
        put("y", np.abs(got[:n, 1] - want[:, 1]))
        put("heading", np.abs(got[:n, 5] - want[:, 5]) if variant == "no_heading_wrap" else RR.angular_distance(got[:n, 5], want[:, 5]))
        g32 = snap["rows"][w, a, :n]
        key32 = (g32[:, 0] * g32[:, 0] + g32[:, 1] * g32[:, 1])
        put("key", RR.gap(key32.astype(f64), ref["keys"][idx]))
        put("dist", np.abs(np.sqrt(key32).astype(f64) - ref["dist"][idx]))
    return out


def measure_oracle(run, orc, p):
    """The oracle's observationOf of EVERY road of every agent (its state is that of pass p) against the reference's:
    {(span, column): largest difference}; x, y, heading and dist over the roads within radius + 1 m, key over all."""
    out = {}
    for w, a in run.agents():
        ref = run.ref(p, w, a)
        o = orc.road_obs_of(w, a)
        o64 = o.astype(f64)
        span = run.case.worlds[w].span
        near = ref["dist"] <= run.case.radius + 1.0
        key32 = o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]
        vals = dict(x=np.abs(o64[near, 0] - ref["obs"][near, 0]), y=np.abs(o64[near, 1] - ref["obs"][near, 1]),
                    heading=RR.angular_distance(o64[near, 5], ref["obs"][near, 5]), key=RR.gap(key32.astype(f64), ref["keys"]),
                    dist=np.abs(np.sqrt(key32).astype(f64)[near] - ref["dist"][near]))
        for c, v in vals.items():
            if len(v):
                out[(span, c)] = max(out.get((span, c), 0.0), float(v.max()))
    return out


def ratios(err, factor=1.0):
    return {(span, col): v / (factor * ORACLE_ROAD_MAX[span][col]) for (span, col), v in err.items()}


def hold(run, p, factor, sim=0):
    """Raises unless simulator `sim`'s rows after pass p meet the reference: structure and exact columns exact, float columns
    within factor * ORACLE_ROAD_MAX.  Returns errors() with the ratios added."""
    e = errors(run, p, factor, sim=sim)
    e["ratio"] = ratios(e["err"], factor)
    over = {k: v for k, v in e["ratio"].items() if v > 1.0}
    if e["bad"] or over:
        raise AssertionError("%s (%s), %s: %s%s [%d of %d agents marginal, %d undecided]" % (
            run.case.name, run.mode, run.passes[p]["tag"], "; ".join(e["bad"][:4]),
            "; ".join("%s at +-%g m: %.3g is %.2f times its bound" % (c, s, e["err"][(s, c)], v) for (s, c), v in over.items()),
            e["marginal"], e["agents"], e["undecided"]))
    return e
