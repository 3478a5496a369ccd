"""CPU suite: the float64 collision reference (tests/collision_reference.py) against hand-worked answers, the oracle against
the reference on the constructed worlds of tests/collision_cases.py -- outside the margin, `collided` and info[0:3] are equal
without exception -- and the sweep that measures the margin band: near-touching pairs through the oracle's obb_collide."""
import math

import numpy as np
import pytest

from tests import collision_cases as CC
from tests import collision_reference as CR
from tests import geom_cases as GC
from tests import geom_reference as GR
from tests import parity as P

f32 = np.float32
VEH, PED, CYC = CR.ET_VEHICLE, CR.ET_PEDESTRIAN, CR.ET_CYCLIST


# ------------------------------------------------------------------------------------------------------------------
# the reference itself, against answers worked out by hand
# ------------------------------------------------------------------------------------------------------------------
def _inputs(agents, roads):
    """Reference inputs for one world written by hand.  agents: dicts with x, y, yaw, half (hx, hy), type and optionally z,
    static, controlled, done, valid; roads: (x, y, hx, hy, yaw, type)."""
    n, R = len(agents), len(roads)
    st = np.zeros((1, n, 11), f32)
    ab = np.zeros((1, n, 14), f32)
    info = np.zeros((1, n, 5), np.int32)
    resp = np.zeros((1, n), np.int32)
    ctl = np.zeros((1, n, 1), np.int32)
    done = np.zeros((1, n), np.int32)
    valid = np.ones((1, n, 91), f32)
    for i, ag in enumerate(agents):
        st[0, i, :3] = (ag["x"], ag["y"], ag.get("z", 1.0))
        st[0, i, 3], st[0, i, 6] = math.cos(ag.get("yaw", 0.0) / 2), math.sin(ag.get("yaw", 0.0) / 2)
        ab[0, i, 10:12] = (2 * ag["half"][0] / 0.7, 2 * ag["half"][1] / 0.7)   # the stored half extent is 0.7 * size / 2
        info[0, i, 4] = ag.get("type", VEH)
        resp[0, i] = CR.RESP_STATIC if ag.get("static") else 0
        ctl[0, i, 0] = ag.get("controlled", 1)
        done[0, i] = ag.get("done", 0)
        valid[0, i] = ag.get("valid", 1.0)
    mo = np.zeros((1, max(R, 1), 9), f32)
    for r, (x, y, hx, hy, yaw, t) in enumerate(roads):
        mo[0, r] = (x, y, hx, hy, 0.1, yaw, t, 0, 0)
    return dict(shape=np.asarray([[n, R]], np.int32), state=st, abs_obs=ab, info=info, controlled=ctl,
                action=np.zeros((1, n, 10), f32), map_obs=mo, resp=resp, done=done, steps=np.full((1, n), 91, np.int64), valid=valid)


def _box(x, y, yaw, hx, hy):
    return (x, y, yaw, hx, hy)


def test_separation_on_hand_worked_rectangles():
    """Two 2 x 2 squares side by side: centres 2 apart touch (separation 0, which counts as overlap), 2.001 apart are 1 mm
    apart.  A 2 x 2 square turned by 45 degrees has its corner sqrt(2) from its centre: with its centre at 1 + sqrt(2) + g on
    the x axis, the corner is g from the first square's face x = 1, and that face normal is the axis of the largest gap (along
    the turned square's own normals the gap is (1 + g) / sqrt(2) - 1 - sqrt(2) / 2... < 0).  A 1 x 1 square inside a 4 x 4 one,
    same centre: along either axis the projections overlap by 0.5 + 2, separation -2.5."""
    A = _box(0.0, 0.0, 0.0, 1.0, 1.0)
    assert CR.separation(A, _box(2.0, 0.0, 0.0, 1.0, 1.0)) == 0.0
    assert abs(CR.separation(A, _box(2.001, 0.0, 0.0, 1.0, 1.0)) - 1e-3) < 1e-12
    assert abs(CR.separation(A, _box(0.0, -2.001, math.pi / 2, 1.0, 1.0)) - 1e-3) < 1e-12
    for g in (0.01, -0.01, 0.0):
        assert abs(CR.separation(A, _box(1.0 + math.sqrt(2.0) + g, 0.0, math.pi / 4, 1.0, 1.0)) - g) < 1e-12
    assert CR.separation(_box(3.0, 4.0, 0.3, 2.0, 2.0), _box(3.0, 4.0, 0.3, 0.5, 0.5)) == -2.5
    # symmetric, and unchanged when both rectangles are moved and turned together
    B = _box(2.2, 1.7, 0.8, 1.4, 0.7)
    s = CR.separation(A, B)
    assert s == CR.separation(B, A)
    c, sn = math.cos(1.1), math.sin(1.1)
    moved = CR.separation(_box(50.0, -20.0, 1.1, 1.0, 1.0), _box(50.0 + c * 2.2 - sn * 1.7, -20.0 + sn * 2.2 + c * 1.7, 1.9, 1.4, 0.7))
    assert abs(moved - s) < 1e-12
    # vectorised over pairs
    out = CR.separation([np.zeros(2), np.zeros(2), np.zeros(2), np.ones(2), np.ones(2)], [np.asarray([2.0, 2.001]), np.zeros(2), np.zeros(2), np.ones(2), np.ones(2)])
    assert out.shape == (2,) and out[0] == 0.0 and abs(out[1] - 1e-3) < 1e-12


def test_reference_on_the_five_obb_cases_of_the_reference_suite():
    """The known-answer cases of the reference's own collision tests (two boxes given by centre, yaw and half extents): aligned
    and overlapping; apart; touching at a corner (overlap: touching counts); one inside the other; the same box turned through
    the circle in steps of 15 degrees about a point inside the first."""
    def verdict(pos_b, yaw_b, half_a, half_b):
        inp = _inputs([dict(x=0.0, y=0.0, half=half_a), dict(x=pos_b[0], y=pos_b[1], yaw=yaw_b, half=half_b)], [])
        ref = CR.collision_reference(inp, 0, 1e-3)
        assert ref["collided"][0] == ref["collided"][1] and ref["info"][0].tolist() == [0, int(ref["collided"][0]), 0]
        return bool(ref["collided"][0])
    assert verdict((1.0, 1.0), 0.0, (1.0, 1.0), (1.0, 1.0))
    assert not verdict((2.0, 2.0), 0.0, (0.5, 0.5), (0.5, 0.5))
    assert verdict((1.0, 1.0), 0.0, (0.5, 0.5), (0.5, 0.5))
    assert verdict((0.0, 0.0), 0.0, (1.0, 1.0), (0.5, 0.5))
    for deg in range(0, 360, 15):
        assert verdict((0.5, 0.5), math.radians(deg), (1.0, 1.0), (1.0, 1.0))


def test_reference_filter_table_and_info_columns():
    """Every (agent type, other type) combination, one overlapping pair per world: of the agent-on-road pairs only a vehicle
    on a road edge and anybody on a stop sign collide -- the 14 others are the filter table -- and every agent pair collides.
    The info column follows the OTHER's type: a road 0, a vehicle 1, a pedestrian or cyclist 2."""
    colliding_roads = {(VEH, CR.ET_ROAD_EDGE), (VEH, CR.ET_STOP_SIGN), (PED, CR.ET_STOP_SIGN), (CYC, CR.ET_STOP_SIGN)}
    seen = 0
    for at in (VEH, PED, CYC):
        for rt in range(CR.ET_ROAD_EDGE, CR.ET_STOP_SIGN + 1):
            ref = CR.collision_reference(_inputs([dict(x=0.2, y=0.1, half=(1.0, 0.5), type=at)], [(0.0, 0.0, 2.0, 0.2, 0.3, rt)]), 0, 1e-3)
            want = (at, rt) in colliding_roads
            assert bool(ref["collided"][0]) == want and ref["info"][0].tolist() == [int(want), 0, 0], (at, rt)
            seen += not want
        for bt in (VEH, PED, CYC):
            ref = CR.collision_reference(_inputs([dict(x=0.2, y=0.1, half=(1.0, 0.5), type=at), dict(x=0.0, y=0.0, half=(1.0, 0.5), type=bt)], []), 0, 1e-3)
            assert ref["collided"].all()
            assert ref["info"][0].tolist() == [0, int(bt == VEH), int(bt != VEH)] and ref["info"][1].tolist() == [0, int(at == VEH), int(at != VEH)]
    assert seen == 14 == len(CR.FILTERED_PAIRS)
    # two hits of different kinds set two columns
    ref = CR.collision_reference(_inputs([dict(x=0.0, y=0.0, half=(1.0, 0.5)), dict(x=0.5, y=0.0, half=(0.3, 0.3), type=PED)],
                                         [(0.0, 0.4, 2.0, 0.1, 0.0, CR.ET_ROAD_EDGE)]), 0, 1e-3)
    assert ref["info"].tolist() == [[1, 0, 1], [0, 1, 0]]


def test_reference_activity_rules():
    """Each rule on a pair of overlapping cars (and a road edge under the first)."""
    edge = [(0.0, 0.0, 3.0, 0.1, 0.0, CR.ET_ROAD_EDGE)]

    def run(a, b, roads=edge, seen=None):
        base = dict(half=(1.0, 0.5))
        inp = _inputs([dict(base, x=0.0, y=0.0, **a), dict(base, x=0.5, y=0.2, **b)], roads)
        ref = CR.collision_reference(inp, 0, 1e-3, seen(inp) if seen else None)
        return ref["collided"].tolist(), ref["info"].tolist()
    assert run({}, {}) == ([True, True], [[1, 1, 0], [1, 1, 0]])
    # parked on parked: no pair; and a parked car makes no pair with a road
    assert run(dict(static=1, controlled=0), dict(static=1, controlled=0)) == ([False, False], [[0, 0, 0], [0, 0, 0]])
    # controlled on parked: both collide, the road counts for the controlled one only
    assert run({}, dict(static=1, controlled=0)) == ([True, True], [[1, 1, 0], [0, 1, 0]])
    # an expert whose log is invalid at the current step is no partner; valid, it is
    assert run({}, dict(controlled=0, valid=0.0)) == ([True, False], [[1, 0, 0], [0, 0, 0]])
    assert run({}, dict(controlled=0)) == ([True, True], [[1, 1, 0], [1, 1, 0]])
    late = np.ones(91, f32)
    late[3] = 0
    at3 = lambda inp: dict(done=inp["done"] != 0, collided=np.zeros((1, 2), bool), step=np.full((1, 2), 3))
    assert run({}, dict(controlled=0, valid=late)) == ([True, True], [[1, 1, 0], [1, 1, 0]])
    assert run({}, dict(controlled=0, valid=late), seen=at3) == ([True, False], [[1, 0, 0], [0, 0, 0]])
    # at the padding height
    assert run(dict(z=CR.PAD_Z), {}) == ([False, True], [[0, 0, 0], [1, 0, 0]])
    # controlled and done, not collided: inactive; done because it collided: active
    assert run(dict(done=1), {}) == ([False, True], [[0, 0, 0], [1, 0, 0]])
    carried = lambda inp: dict(done=inp["done"] != 0, collided=np.asarray([[True, False]]), step=np.zeros((1, 2), np.int64))
    assert run(dict(done=1), {}, seen=carried) == ([True, True], [[1, 1, 0], [1, 1, 0]])
    # a done flag means nothing for an agent nobody controls
    assert run(dict(done=1, controlled=0), {}) == ([True, True], [[1, 1, 0], [1, 1, 0]])


def test_expected_after_step_keeps_or_forgets():
    prev = dict(state=np.zeros((3, 11), f32), info=np.zeros((3, 5), np.int32), resp=np.asarray([0, CR.RESP_STATIC, 0]), done=np.zeros(3, np.int32))
    prev["state"][:2, 10] = 1
    prev["info"][0, 1] = prev["info"][1, 1] = prev["info"][2, 0] = 1   # (agent 2: a column left by a pass without movement)
    fresh = dict(collided=np.asarray([False, True, True]), info=np.asarray([[0, 0, 0], [1, 0, 0], [0, 0, 1]]))
    out = CR.expected_after_step(prev, fresh, CR.IGNORE)
    assert out["collided"].tolist() == [False, True, True] and np.asarray(out["info"]).astype(int).tolist() == [[0, 0, 0], [1, 0, 0], [1, 0, 1]]
    assert not out["padded"].any() and not out["done_at_least"].any()
    out = CR.expected_after_step(prev, fresh, CR.AGENT_STOP)
    assert out["collided"].tolist() == [True, True, True] and np.asarray(out["info"]).astype(int).tolist() == [[0, 1, 0], [1, 1, 0], [1, 0, 1]]
    assert out["done_at_least"].tolist() == [True, True, False] and out["padded"].tolist() == [True, False, False]
    assert CR.expected_after_step(prev, fresh, CR.AGENT_REMOVED)["padded"].tolist() == [True, True, False]


# ------------------------------------------------------------------------------------------------------------------
# the margin band: the oracle's narrowphase on near-touching pairs
# ------------------------------------------------------------------------------------------------------------------
AGENT_SHAPES = ((1.4, 0.7), (7.7, 1.05), (1.05, 0.49), (0.315, 0.315), (0.63, 0.245))
ROAD_SHAPES = ((3.0, 0.1), (5.0, 0.1), (12.0, 0.1), (15.0, 0.1), (20.0, 0.1), (30.0, 0.1), (35.0, 0.1), (40.0, 0.1), (0.2, 0.2), (3.0, 1.5))
SWEEP_PAIRS = 20000


def _sweep(O, span, seed):
    """Pairs of the cases' own box shapes (an agent box against an agent box or a road box), the first anywhere within +-span,
    the second pushed along a random ray until the float64 separation is +-gap, gap log-uniform in 1e-6 ... 1e-1 m; then every
    coordinate, yaw and half extent is rounded to float32 and the separation of THOSE numbers is compared with the oracle's
    verdict.  Returns (largest |sep| at which the verdicts differ, number of differing pairs)."""
    rng = np.random.default_rng(seed)
    N = SWEEP_PAIRS
    A = np.asarray(AGENT_SHAPES)[rng.integers(0, len(AGENT_SHAPES), N)]
    other = np.concatenate([np.asarray(AGENT_SHAPES), np.asarray(ROAD_SHAPES)])
    B = other[rng.integers(0, len(other), N)]
    far = span - 90.0   # (the second box's centre stays within the span: the longest box is 80 m)
    ax, ay = rng.uniform(-far, far, N), rng.uniform(-far, far, N)
    ayaw, byaw, ray = rng.uniform(-np.pi, np.pi, N), rng.uniform(-np.pi, np.pi, N), rng.uniform(-np.pi, np.pi, N)
    quarter = rng.random(N) < 0.25    # a quarter of the pairs at relative yaws that are multiples of pi / 2
    byaw = np.where(quarter, ayaw + (np.pi / 2) * rng.integers(0, 4, N), byaw)
    gap = 10.0 ** rng.uniform(-6, -1, N) * rng.choice([-1.0, 1.0], N)
    lo, hi = np.zeros(N), np.full(N, 100.0)
    for _ in range(60):
        t = (lo + hi) / 2
        s = CR.separation((ax, ay, ayaw, A[:, 0], A[:, 1]), (ax + t * np.cos(ray), ay + t * np.sin(ray), byaw, B[:, 0], B[:, 1]))
        below = s < gap
        lo, hi = np.where(below, t, lo), np.where(below, hi, t)
    t = (lo + hi) / 2
    r32 = lambda v: np.asarray(v, f32)
    pa, pb = np.stack([r32(ax), r32(ay), np.ones(N, f32)], -1), np.stack([r32(ax + t * np.cos(ray)), r32(ay + t * np.sin(ray)), np.ones(N, f32)], -1)
    ya, yb, sa, sb = r32(ayaw), r32(byaw), r32(A), r32(B)
    # (the oracle stores the yaw as a rotation and reads it back: the reference is given that rotation's heading)
    sep = CR.separation((pa[:, 0], pa[:, 1], GR.yaw_of(GC.quat_of_yaw(ya)), sa[:, 0], sa[:, 1]),
                        (pb[:, 0], pb[:, 1], GR.yaw_of(GC.quat_of_yaw(yb)), sb[:, 0], sb[:, 1]))
    got = np.asarray([O.obb_collide(pa[i], ya[i], sa[i], pb[i], yb[i], sb[i]) for i in range(N)])
    flipped = got != (sep <= 0)
    return (float(np.abs(sep[flipped]).max()) if flipped.any() else 0.0), int(flipped.sum())


@pytest.mark.parametrize("span", sorted(CC.ORACLE_FLIP_MAX))
def test_the_oracles_narrowphase_flips_only_inside_the_recorded_band(oracle_mod, span):
    worst, count = _sweep(oracle_mod, span, int(span))
    print("COLL sweep: coordinates within +-%g m: %d of %d near-touching pairs flipped, largest |sep| %.3g m (recorded %.3g)" %
          (span, count, SWEEP_PAIRS, worst, CC.ORACLE_FLIP_MAX[span]))
    assert count > 0, "the sweep never reached the oracle's rounding: it measures nothing"
    assert worst <= CC.ORACLE_FLIP_MAX[span], "the oracle flipped a pair %.3g m from touching: ORACLE_FLIP_MAX[%g] is stale" % (worst, span)
    assert worst >= 0.8 * CC.ORACLE_FLIP_MAX[span], "ORACLE_FLIP_MAX[%g] = %.3g is far above what is measured (%.3g)" % (span, CC.ORACLE_FLIP_MAX[span], worst)


def test_every_case_uses_a_recorded_span_that_holds_its_coordinates(tmp_path, oracle_mod):
    for case in CC.CASE_LIST:
        orc = P.make_oracle_sim(oracle_mod, case.write(tmp_path), max_agents=case.slots, **case.params())
        inp = CR.read_inputs(orc)
        orc.close()
        for w in range(len(case.worlds)):
            e = GR.lidar_entities(inp, w)
            reach = np.hypot(e["hx"], e["hy"])
            assert np.maximum(np.abs(e["cx"]) + reach, np.abs(e["cy"]) + reach).max() <= case.span, case.name


# ------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
# ------------------------------------------------------------------------------------------------------------------
def _report(case, tag, got, premise=None):
    print("COLL %s %s: agents %d, colliding %d, marginal %d%s" % (case.name, tag, got["agents"], got["colliding"], got["marginal"],
                                                                  "" if premise is None else "; premise: " + premise))
    assert got["marginal"] <= CC.MARGIN_AGENTS * got["agents"], "%s: %d of %d agents are marginal: move the geometry" % \
        (case.name, got["marginal"], got["agents"])


@pytest.mark.parametrize("name", list(CC.CASES))
def test_oracle_meets_the_reference_on_constructed_worlds(oracle_mod, tmp_path, name):
    """Reset pass, then a State-model step under Ignore that moves two agents of every world: one from clear into contact, one
    from contact to clear."""
    case = CC.CASES[name]
    scenes = case.write(tmp_path)
    orc = P.make_oracle_sim(oracle_mod, scenes, max_agents=case.slots, **case.params(CR.IGNORE, 3))
    built, = CC.place(case, [orc])
    inp = CR.read_inputs(orc)
    _report(case, "reset pass", CC.compare_to_reference(case, orc, name + " (reset pass)", built), case.premise(case, inp))
    refs = [CR.collision_reference(inp, w, case.band) for w in range(len(case.worlds))]
    before, = CC.step_pass(case, [orc])
    _report(case, "step pass", CC.compare_to_reference(case, orc, name + " (step pass)", before, CR.IGNORE))
    after = CR.read_inputs(orc)
    CC.moved_flags(case, refs, [CR.collision_reference(after, w, case.band, CR.seen_in_step(before, CR.IGNORE)) for w in range(len(case.worlds))])
    if name == "coll_static_inactive":
        seen, = CC.done_rule_pass(case, [orc])
        now = CR.read_inputs(orc)
        ref = CR.collision_reference(now, 0, case.band, dict(done=seen["done"] != 0, collided=np.zeros(seen["done"].shape, bool),
                                                             step=CR.EPISODE - seen["steps"]))
        assert ref["sep"][9, 10] < -0.2 and not ref["active"][9] and not ref["collided"][9] and not ref["collided"][10]
        _report(case, "done rule", CC.compare_to_reference(case, orc, name + " (done rule)", seen))
    orc.close()


@pytest.mark.parametrize("behaviour", [0, 1, 2])
@pytest.mark.parametrize("name", CC.BEHAVIOUR_CASES)
def test_oracle_meets_the_reference_under_every_collision_behaviour(oracle_mod, tmp_path, name, behaviour):
    """The step pass and one more step (every agent handed back the pose it has): flags forgotten or kept, done set, removed
    agents at the padding position and colliding with nothing."""
    case = CC.CASES[name]
    orc = P.make_oracle_sim(oracle_mod, case.write(tmp_path), max_agents=case.slots, **case.params(behaviour, 3))
    GC.place(case, [orc])
    for k in (1, 2):
        before, = CC.step_pass(case, [orc]) if k == 1 else CC.hold_step(case, [orc])
        got = CC.compare_to_reference(case, orc, "%s (behaviour %d, step %d)" % (name, behaviour, k), before, behaviour)
        _report(case, "behaviour %d step %d" % (behaviour, k), got)
    if behaviour != CR.IGNORE:
        assert (CC.flags_of(orc)["z"][0] == CR.PAD_Z).sum() > 0
    orc.close()
