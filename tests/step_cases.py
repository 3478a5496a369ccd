"""Constructed worlds for the step reference (tests/step_reference.py): each case aims a few agents at one rule of the state
step that the Waymo scenes and the seeded lockstep actions never reach -- a yaw sum across +-pi, a negative mean speed, an
action outside the InvertibleBicycle clamps, a vertical velocity, an agent exactly on the goal threshold, the last step of an
episode, the done rules after a collision -- and asserts its own premise FROM THE REFERENCE'S INTERMEDIATE VALUES so that it
cannot quietly stop exercising that rule.

Scenes are built with the helpers of tests/geom_cases.py (`moving_car` adds a car whose 91-entry log moves).  All cases:
polylineReductionThreshold = 0, initOnlyValidAgentsAtFirstStep = 0, isStaticAgentControlled = 0 (a car whose goal is where it
stands is parked: Static and nobody's to control), observationRadius = 50.

TOLERANCES.  Every bound on a float output is ORACLE_STEP_MAX[span][column]: the largest distance of the ORACLE (float32, host
libm) from the reference on the cases below, over every pass of every run of tests/test_step_reference.py, per coordinate span
of the world (+-150 m, +-1500 m; PAD_SPAN for what is computed from the padding position at -11000 m).  That suite asserts
that the oracle stays within each constant and that no constant is more than twice what is measured.  The GPU suite allows
GPU_FACTOR times the constant -- the factor of GC.GPU_DEPTH_FACTOR and CC.GPU_BAND_FACTOR, for the same reason: the device's
double-then-round transcendentals differ from glibc's float ones by about an ulp -- and no bound is ever taken from the
kernel's output.  The goal-distance band (`band_of`) is GPU_FACTOR times the "reward" column: under the distance-based reward
that column IS the distance to the goal."""
import math

import numpy as np

from tests import collision_cases as CC
from tests import collision_reference as CR
from tests import geom_cases as GC
from tests import geom_reference as GR
from tests import parity as P
from tests import step_reference as SR

f32 = np.float32
f64 = np.float64
PI = GC.PI
GPU_FACTOR = 2.0
AIMED_FACTOR = CC.AIMED_FACTOR
MARGIN_AGENTS = CC.MARGIN_AGENTS
PAD_SPAN = 12000.0
COLUMNS = ("pos", "yaw", "vel", "speed", "goal", "reward")

# span: column: the largest |oracle - reference| (metres, radians, m/s), rounded up; measured value in the comment.
ORACLE_STEP_MAX = {
    # measured: pos 1.475e-05, yaw 1.256e-06, vel 9.220e-06, speed 7.674e-06, goal 2.151e-04, reward 2.185e-05 (yaw, vel and
    # goal in step_steer under Classic: steering 1.5 on a 0.5 m body turns it by 3.2 rad in one step)
    150.0: dict(pos=1.5e-5, yaw=1.3e-6, vel=9.3e-6, speed=7.7e-6, goal=2.2e-4, reward=2.2e-5),
    # measured: pos 8.767e-05, yaw 3.023e-07, vel 3.624e-06, speed 1.808e-06, goal 5.206e-04, reward 1.465e-04 (step_far)
    1500.0: dict(pos=8.8e-5, yaw=3.1e-7, vel=3.7e-6, speed=1.9e-6, goal=5.3e-4, reward=1.5e-4),
    # measured: goal 2.195e-03, reward 8.395e-04 (step_goal, the step after the arrival)
    PAD_SPAN: dict(goal=2.2e-3, reward=8.4e-4),
}


def band_of(span):
    return GPU_FACTOR * ORACLE_STEP_MAX[span]["reward"]


# ------------------------------------------------------------------------------------------------------------------
# scene building
# ------------------------------------------------------------------------------------------------------------------
def moving_car(i, xs, ys, headings, vxs, vys, valid=None, goal=None, **kw):
    """A car whose 91-entry log moves: position, heading, velocity and valid flag per step.  (GC.World keeps only the first
    heading of a log: `world` below puts these back.)"""
    c = GC.car(i, xs[0], ys[0], headings[0], **kw)
    assert len(xs) == len(ys) == len(headings) == len(vxs) == len(vys) == 91
    c["position"] = [{"x": float(x), "y": float(y), "z": 0.0} for x, y in zip(xs, ys)]
    c["velocity"] = [{"x": float(x), "y": float(y)} for x, y in zip(vxs, vys)]
    c["valid"] = [True] * 91 if valid is None else [bool(v) for v in valid]
    c["log_heading"] = [float(h) for h in headings]
    if goal is not None:
        c["goalPosition"] = {"x": float(goal[0]), "y": float(goal[1]), "z": 0.0}
    return c


def with_goal(c, gx, gy):
    c["goalPosition"] = {"x": float(gx), "y": float(gy), "z": 0.0}
    return c


def world(name, cars, roads=(), span=150.0, vel=None):
    """GC.World plus: the coordinate span, the velocities `place` writes, and the moving logs' headings (each one a yaw both
    sides turn into the same rotation, like GC.World's own)."""
    logs = [c.pop("log_heading", None) for c in cars]
    for c in cars:      # (GC.car's goal lies 1000 m east: here every goal stays within the span, >= 100 m from its car)
        x, y = c["position"][0]["x"], c["position"][0]["y"]
        if c["goalPosition"]["x"] == x + 1000.0:
            with_goal(c, -math.copysign(100.0, x), y)
    # (one short lane at the origin: a vehicle never collides with a lane, and no world is without roads)
    wd = GC.World(name, cars, list(roads) or [GC.road(0, "lane", GC.segment(0.0, 0.0, 0.1, 5.0))])
    for c, log, yaw0 in zip(wd.scene["objects"], logs, wd.yaw):
        if log is not None:
            c["heading"] = [float(yaw0)] + [float(P.agreeing_yaw(f32(h))) for h in log[1:]]
    wd.span = span
    wd.vel = None if vel is None else np.asarray(vel, f32).reshape(wd.n, 3)
    return wd


def grid(i, cols, pitch, rows):
    return ((i % cols) - (cols - 1) / 2) * pitch, ((i // cols) - (rows - 1) / 2) * pitch


class Case:
    def __init__(self, name, worlds, models, actions, premise, steps, slots=64, threshold=2.0, behaviours=(CR.IGNORE,),
                 reward_types=(SR.ON_GOAL,), extra=None):
        self.name, self.worlds, self.models, self.actions, self.premise, self.steps = name, worlds, models, actions, premise, steps
        self.slots, self.threshold, self.behaviours, self.reward_types = slots, threshold, behaviours, reward_types
        self.extra = extra or {}
        self.heads_for = None
        for wd in worlds:
            assert wd.n <= min(slots, 128) and len(wd.scene["roads"]) <= 8, name

    write = GC.Case.write

    def params(self, model, behaviour, reward_type):
        kw = dict(polylineReductionThreshold=0.0, collisionBehaviour=behaviour, dynamicsModel=model, observationRadius=50.0,
                  initOnlyValidAgentsAtFirstStep=0, isStaticAgentControlled=0, rewardType=reward_type,
                  distanceToGoalThreshold=self.threshold)
        kw.update(self.extra)
        return kw

    def runs(self):
        return [(self.name, m, b, r) for m in self.models for b in self.behaviours for r in self.reward_types]


class Run:
    """One scripted run of a case on one or more simulators that are given the same actions (the first one's tensors are the
    template).  history: one (before, after) pair of snapshot lists per pass, the reset pass of `place` first."""

    def __init__(self, case, sims, model, behaviour, reward_type):
        self.case, self.sims, self.model, self.behaviour, self.reward_type = case, list(sims), model, behaviour, reward_type
        self.yaw = np.zeros((len(case.worlds), case.slots), f32)     # the yaw the State model last handed every agent
        for w, wd in enumerate(case.worlds):
            self.yaw[w, :wd.n] = wd.yaw
        self.history = []

    def place(self):
        before = [SR.snapshot(s) for s in self.sims]
        GC.place(self.case, self.sims)
        if any(wd.vel is not None for wd in self.case.worlds):
            st = _get_state(self.sims[0])
            for w, wd in enumerate(self.case.worlds):
                if wd.vel is not None:
                    st[w, :wd.n, 7:10] = wd.vel
            for s in self.sims:
                _set_state(s, st)
                s.reset([])
        after = [SR.snapshot(s) for s in self.sims]
        for b, a in zip(before, after):    # (a pass that moves nothing: the poses it starts from are the ones it leaves)
            b["state"], b["action"] = a["state"].copy(), a["action"].copy()
        self.history.append((before, after, True))
        return before, after

    def step(self, k):
        before = [SR.snapshot(s) for s in self.sims]
        act = self.case.actions(self, k, before[0])
        for s in self.sims:
            P.write_actions(s, act)
        before = [dict(b, action=np.array(act, f32)) for b in before]
        for s in self.sims:
            s.step()
        after = [SR.snapshot(s) for s in self.sims]
        self.history.append((before, after, False))
        return before, after

    def recompute(self):
        """A pass that moves nothing and counts no step."""
        before = [SR.snapshot(s) for s in self.sims]
        for s in self.sims:
            s.reset([])
        after = [SR.snapshot(s) for s in self.sims]
        self.history.append((before, after, True))
        return before, after

    def ref(self, before, after, w, reset_pass=False, variant=None):
        return SR.step_reference(before, after, w, self.model, self.behaviour, self.reward_type, self.case.threshold,
                                 band_of(self.case.worlds[w].span), reset_pass, variant)

    def hold_pose(self, before):
        """State-model actions that hand every agent back the pose it has (the yaw as the host last gave it: bit for bit)."""
        st = before["state"]
        act = np.zeros(st.shape[:2] + (10,), f32)
        act[..., 0:3] = st[..., 0:3]
        act[..., 3] = self.yaw
        act[..., 4:7] = st[..., 7:10]
        return act


def _get_state(s):
    return s.get_state() if hasattr(s, "get_state") else s.debug_get_state()


def _set_state(s, st):
    (s.set_state if hasattr(s, "set_state") else s.debug_set_state)(st)


def _blank(run):
    return np.zeros((len(run.case.worlds), run.case.slots, 10), f32)


# ------------------------------------------------------------------------------------------------------------------
# step_wrap
# ------------------------------------------------------------------------------------------------------------------
PI32 = float(f32(PI))
HEADINGS = (-PI32, PI32, float(np.nextafter(f32(-PI), f32(0))), float(np.nextafter(f32(PI), f32(0))), PI / 2, -PI / 2, 0.0, 3.0, -3.0)
TURNS = (1.0, -1.0, 0.0)
WRAP_SPEED = 10.0


def _wrap_agent(i):
    return HEADINGS[i % 9], TURNS[(i // 9) % 3]


def _wrap_world(name="wrap", count=27, cols=6, pitch=14.0):
    rows = -(-count // cols)
    cars, vel = [], []
    for i in range(count):
        h, _ = _wrap_agent(i)
        x, y = grid(i, cols, pitch, rows)
        cars.append(GC.car(i, x + 0.013 * i, y - 0.007 * i, h))
        vel.append((WRAP_SPEED * math.cos(h), WRAP_SPEED * math.sin(h), 0.0))
    return world(name, cars, vel=vel)


def _wrap_action(model, i, yaw_now):
    """One agent's action: the turn has the sign of its TURNS entry; under DeltaLocal the agents at +-3 whose entry is 0 are
    carried ONTO the seam."""
    h, s = _wrap_agent(i)
    if model == SR.CLASSIC:
        return (0.5, 0.7 * s, 0.0)
    if model == SR.BICYCLE:
        return (0.5, 0.3 * s, 0.0)
    dyaw = 0.3 * s
    if abs(h) == 3.0 and s == 0:
        dyaw = float(f32(math.copysign(PI32, h)) - f32(yaw_now))
    return (0.8, 0.1 * s, dyaw)


def _wrap_actions(run, k, before):
    act = _blank(run)
    yaw = GR.yaw_of(before["state"][..., 3:7])
    for w, wd in enumerate(run.case.worlds):
        for i in range(wd.n):
            act[w, i, 0:3] = _wrap_action(run.model, i, yaw[w, i])
    return act


def _wrap_premise(run):
    before, after, _ = run.history[1]
    ref = run.ref(before[0], after[0], 0)
    d = ref["driven"]
    above, below = int((d & (ref["yaw_sum"] > PI + 1e-4)).sum()), int((d & (ref["yaw_sum"] < -PI - 1e-4)).sum())
    onto = int((d & (np.abs(np.abs(ref["yaw_sum"]) - PI) < 1e-6)).sum())
    assert above >= 3 and below >= 3 and onto >= 2, (above, below, onto)
    rel = SR.angular_distance(ref["yaw0"][:, None], ref["yaw0"][None, :])
    opposite = int((np.abs(rel - PI) < 1e-6).sum()) // 2
    assert opposite >= 3, opposite
    heads = {round(float(v), 3) for v in ref["yaw0"]}
    assert {round(h, 3) for h in HEADINGS} <= heads | {-round(PI, 3), round(PI, 3)}, heads
    return "yaw sums: %d above pi, %d below -pi, %d on the seam; %d pairs of exactly opposite headings" % (above, below, onto, opposite)


# ------------------------------------------------------------------------------------------------------------------
# step_speed
# ------------------------------------------------------------------------------------------------------------------
# (speed, acceleration, vz, steering)
SPEED_AGENTS = ((0.0, 0.0, 0.0, 0.2), (0.0, -2.0, 0.0, 0.2), (0.05, -2.0, 0.0, -0.2), (0.15, -2.0, 0.0, 0.2), (60.0, 1.0, 0.0, 0.05),
                (60.0, -3.0, 0.0, -0.05), (5.0, 0.5, 2.0, 0.2), (0.0, 2.0, 0.0, -0.2), (0.15, -2.0, 0.0, -0.3), (0.05, -2.0, 0.0, 0.3),
                (3.0, -6.0, 1.0, 0.1), (0.12, -2.0, 0.5, 0.0))


def _speed_world():
    cars, vel = [], []
    for i, (speed, _, vz, _) in enumerate(SPEED_AGENTS):
        h = 0.7 * i - 2.0
        x, y = grid(i, 4, 30.0, 3)
        cars.append(GC.car(i, x, y, h))
        vel.append((speed * math.cos(h), speed * math.sin(h), vz))
    return world("speed", cars, vel=vel)


def _speed_actions(run, k, before):
    act = _blank(run)
    for i, (_, a, _, steer) in enumerate(SPEED_AGENTS):
        act[0, i, 0:2] = (a, steer)
    return act


def _speed_premise(run):
    (b1, a1, _), (b2, a2, _) = run.history[1], run.history[2]
    r1, r2 = run.ref(b1[0], a1[0], 0), run.ref(b2[0], a2[0], 0)
    assert r1["driven"].all() and r2["driven"].all()
    still = int((r1["speed0"] == 0).sum())
    mean_neg = int((r1["v_mean"] < 0).sum())
    end_neg = int(((r1["v_end"] < 0) & (r1["v_mean"] > 0)).sum())
    rising = int((b1[0]["state"][0, :len(r1["x"]), 9] != 0).sum())
    backwards = int((r2["along"] < -1e-3).sum())
    assert still >= 3 and mean_neg >= 2 and end_neg >= 2 and rising >= 3 and backwards >= 4 and r1["speed0"].max() >= 60.0, \
        (still, mean_neg, end_neg, rising, backwards)
    assert (np.abs(r1["speed0"][[6, 10, 11]] - np.hypot(np.asarray(SPEED_AGENTS)[[6, 10, 11], 0], np.asarray(SPEED_AGENTS)[[6, 10, 11], 2])) < 1e-5).all()
    return "%d at speed 0, %d with a negative mean speed, %d more whose end speed is negative, %d with vz != 0, 60 m/s; step 2: %d " \
        "start from a velocity against the heading" % (still, mean_neg, end_neg, rising, backwards)


# ------------------------------------------------------------------------------------------------------------------
# step_steer
# ------------------------------------------------------------------------------------------------------------------
STEERS = (0.0, 0.7, -0.7, 1.2, -1.2, 1.5, -1.5)
LENGTHS = ((0.5, 0.5, "pedestrian"), (4.0, 2.0, "vehicle"), (12.0, 2.5, "vehicle"), (22.0, 3.0, "vehicle"))
BIKE_ACCEL = (-7.0, -6.0, -3.0, 0.0, 5.9, 6.0, 6.5)
BIKE_STEER = (-3.5, -3.0, 0.2, 3.0, 3.2, -1.0)
STEER_SPEED = 8.0


def _steer_world():
    cars, vel = [], []
    for i in range(28):
        length, width, kind = LENGTHS[i // 7]
        h = 0.45 * i - 3.0
        x, y = grid(i, 7, 30.0, 4)
        cars.append(GC.car(i, x, y, h, length=length, width=width, kind=kind))
        vel.append((STEER_SPEED * math.cos(h), STEER_SPEED * math.sin(h), 0.0))
    return world("steer", cars, vel=vel)


def _steer_actions(run, k, before):
    act = _blank(run)
    for i in range(28):
        act[0, i, 0:2] = (1.0, STEERS[i % 7]) if run.model == SR.CLASSIC else (BIKE_ACCEL[i % 7], BIKE_STEER[i % 6])
    return act


def _steer_premise(run):
    before, after, _ = run.history[1]
    ref = run.ref(before[0], after[0], 0)
    assert ref["driven"].all()
    a, s = before[0]["action"][0, :28, 0], before[0]["action"][0, :28, 1]
    if run.model == SR.CLASSIC:
        seen = {(round(float(v), 2), round(float(l), 2)) for v, l in zip(s, before[0]["abs_obs"][0, :28, 10])}
        assert len(seen) == 28 and {v for v, _ in seen} == {round(v, 2) for v in STEERS} and {l for _, l in seen} == {0.5, 4.0, 12.0, 22.0}
        return "7 steering angles up to +-1.5 on lengths 0.5, 4, 12 and 22 m"
    outside, on = int(((np.abs(a) > 6) & (np.abs(s) > 3)).sum()), int(((np.abs(a) == 6) | (np.abs(s) == 3)).sum())
    inside = int(((np.abs(a) < 6) & (np.abs(s) < 3)).sum())
    assert outside >= 2 and on >= 8 and inside >= 4, (outside, on, inside)
    want = np.stack([np.clip(a, f32(-6), f32(6)), np.clip(s, f32(-3), f32(3))], -1)
    assert np.array_equal(ref["action"][:, 0:2].astype(f32), want)
    return "%d actions outside both clamps, %d on a clamp, %d inside both" % (outside, on, inside)


# ------------------------------------------------------------------------------------------------------------------
# step_far
# ------------------------------------------------------------------------------------------------------------------
def _far_world(name, radius, span):
    cars, vel = [], []
    for i in range(12):
        ang, h = i * PI / 6 + 0.1, 0.9 * i - 3.0
        r = radius * (1.0 if i % 2 == 0 else 0.55)
        x, y = r * math.cos(ang), r * math.sin(ang)
        cars.append(with_goal(GC.car(i, x, y, h), -0.5 * x, -0.5 * y))
        vel.append((12.0 * math.cos(h), 12.0 * math.sin(h), 0.0))
    return world(name, cars, span=span, vel=vel)


def _far_actions(run, k, before):
    act = _blank(run)
    for w in range(2):
        for i in range(12):
            sgn = 1.0 if i % 2 == 0 else -1.0
            act[w, i, 0:3] = {SR.CLASSIC: (1.0, 0.3 * sgn, 0.0), SR.BICYCLE: (1.0, 0.2 * sgn, 0.0), SR.DELTA: (1.2, 0.2 * sgn, 0.1 * sgn)}[run.model]
    return act


def _far_premise(run):
    before, _, _ = run.history[1]
    out = []
    for w, wd in enumerate(run.case.worlds):
        xy = np.abs(before[0]["state"][w, :wd.n, 0:2]).max()
        goal = np.abs(before[0]["abs_obs"][w, :wd.n, 8:10]).max()
        assert 0.8 * wd.span <= xy <= wd.span - 10.0 and goal <= wd.span, (w, xy, goal)
        out.append("world %d within +-%.0f m (largest coordinate %.0f)" % (w, wd.span, xy))
    same = np.array_equal(before[0]["action"][0, :12], before[0]["action"][1, :12])
    assert same
    return "; ".join(out)


# ------------------------------------------------------------------------------------------------------------------
# step_replay
# ------------------------------------------------------------------------------------------------------------------
def _log_circle(i, cx, cy, radius, t0, dt, **kw):
    t = t0 + dt * np.arange(91)
    speed = radius * dt / 0.1
    return moving_car(i, cx + radius * np.cos(t), cy + radius * np.sin(t), SR.wrap(t + PI / 2), -speed * np.sin(t), speed * np.cos(t), **kw)


def _log_line(i, x0, y0, heading, speed, turn=0.0, **kw):
    k = np.arange(91)
    return moving_car(i, x0 + 0.1 * speed * k * math.cos(heading), y0 + 0.1 * speed * k * math.sin(heading), SR.wrap(heading + turn * k),
                      [speed * math.cos(heading)] * 91, [speed * math.sin(heading)] * 91, **kw)


def _replay_world(mixed):
    holes = np.ones(91, bool)
    holes[[10, 11, 40, 90]] = False
    late = np.ones(91, bool)
    late[0:3] = False
    cars = [_log_circle(0, 0.0, 0.0, 20.0, -2.6, 0.06, expert=True),
            _log_line(1, -40.0, 60.0, 0.3, 9.0, valid=holes, expert=True),
            _log_line(2, -30.0, -60.0, 3.0, 1.5, turn=0.01, expert=True),                   # its heading crosses the seam
            _log_line(3, 80.0, 0.0, 1.0, 4.0, goal=(80.0, 0.0)),                            # parked: its log moves, it does not
            _log_line(4, -80.0, 0.0, -2.0, 3.0, valid=late, expert=True)]
    for k in (10, 11, 40, 90):      # (what the log holds where it is invalid is copied all the same)
        cars[1]["position"][k] = {"x": 5.5 + k, "y": -7.25, "z": 0.0}
    if mixed:
        cars += [GC.car(5, 40.0, -30.0, 0.8), GC.car(6, -50.0, 30.0, -2.4)]
    return world("replay_mixed" if mixed else "replay", cars)


def _replay_actions(run, k, before):
    act = _blank(run)
    act[..., 0], act[..., 1] = 0.3, 0.05
    return act


def _replay_premise(run):
    before, after, _ = run.history[1]
    ref = run.ref(before[0], after[0], 0)
    n = len(ref["x"])
    valid = before[0]["traj"][0, :n, SR.TRAJ_VALID:SR.TRAJ_VALID + 91] != 0
    mixed = n == 7
    assert ref["replayed"][[0, 1, 2, 4]].all() and ref["static"][3] and not ref["controlled"][:5].any()
    assert int(ref["driven"].sum()) == (2 if mixed else 0)
    assert (~valid[1, 1:]).sum() == 4 and not valid[4, 0] and valid[4, 3]
    tr = before[0]["traj"][0, 3]
    assert abs(tr[2 * 90] - tr[0]) > 10.0, "the parked car's log must move"
    indices = [int(run.ref(b[0], a[0], 0)["log_index"][0]) for b, a, reset in run.history if not reset]
    assert indices == list(range(91)), indices
    heads = before[0]["traj"][0, 2, SR.TRAJ_HEAD:SR.TRAJ_HEAD + 91]
    assert heads.max() > 3.1 and heads.min() < -3.1
    last = run.history[-1][1][0]
    assert (last["steps"][0, :n] == 0).all() and np.array_equal(last["state"][0, 3, 0:2], before[0]["state"][0, 3, 0:2])
    return "%d replayed (4 log entries of agent 1 and the first 3 of agent 4 invalid, agent 2's heading crosses the seam), %d driven, " \
        "a parked car whose log moves; log indices 0 ... 90" % (int(ref["replayed"].sum()), int(ref["driven"].sum()))


# ------------------------------------------------------------------------------------------------------------------
# step_goal
# ------------------------------------------------------------------------------------------------------------------
RING = 2.0                      # the ring's radius: the threshold of step_goal; step_goal_zero keeps the ring and has none
NEAR, WIDE = 5.0, 40.0          # bands off the ring, nominally: every aimed agent keeps >= AIMED_FACTOR bands


def _ring_offsets():
    b = band_of(150.0)
    return (RING - NEAR * b, RING + NEAR * b, RING - WIDE * b, RING + WIDE * b, 3.0, 50.0)


def _goal_cars(first, count, place_of):
    """Ring agents: agent k's goal at place_of(k); it stands at one of the six distances from it -- the fifth kind stands
    3 m off and is MOVED onto its goal (distance 0) by the State model, or 0.5 m off where nothing moves it."""
    cars = []
    for k in range(count):
        gx, gy = place_of(k)
        d, ang = _ring_offsets()[k % 6], 0.4 + 0.83 * k
        cars.append(with_goal(GC.car(first + k, gx + d * math.cos(ang), gy + d * math.sin(ang), 0.3 * k - 3.0), gx, gy))
    return cars


def _goal_world(name):
    cars = _goal_cars(0, 24, lambda k: grid(k, 6, 9.0, 4))
    cars.append(with_goal(GC.car(24, 33.0, 20.0, 0.2), 30.0, 20.0))        # moved exactly onto the threshold, along an axis
    cars.append(CC.parked(25, -33.0, 20.0, 1.0))
    return world(name, cars)


def _goal_actions(run, k, before):
    act = run.hold_pose(before)
    if k == 0:
        goal = before["abs_obs"][0, :, 8:10]
        for i in range(4, 24, 6):
            act[0, i, 0:2] = goal[i]
        gx = goal[24, 0]
        act[0, 24, 0] = f32(gx - f32(math.copysign(RING, gx)))     # (towards zero: the difference is exact)
        act[0, 24, 1] = goal[24, 1]
    return act


def _goal_premise(run):
    case = run.case
    band = band_of(150.0)
    (b1, a1, _), (b2, a2, _) = run.history[1], run.history[3]     # (history[2] is the recompute pass behind step 1)
    r1, r2 = run.ref(b1[0], a1[0], 0), run.ref(b2[0], a2[0], 0)
    ring = np.asarray([k for k in range(24) if k % 6 < 4])
    off = np.abs(r1["dist"][ring] - RING)
    assert (off >= AIMED_FACTOR * band).all() and (off[np.arange(16) % 4 < 2] <= (NEAR + 1) * band).all(), (off / band).round(2)
    assert (r1["dist"][4:24:6] == 0).all() and (r1["dist"][5:24:6] > 40).all()
    assert r1["dist"][24] == RING and r1["y"][24] == r1["abs_goal"][24, 1] and not r1["margin"].any()
    assert r1["static"][25] and not r1["controlled"][25] and r1["dist"][25] < 0.2
    reset = run.ref(*[s[0] for s in run.history[0][:2]], 0, reset_pass=True)
    assert reset["early"].all() and not reset["done"].any()
    if case.threshold > 0:
        inside = r1["inside"]
        assert inside[ring[0::2]].all() and not inside[ring[1::2]].any() and inside[4:24:6].all() and not inside[24] and inside[25]
        assert np.array_equal(r1["done"], inside) and np.array_equal(r1["reached"], inside)
        gone = r2["padded"]
        assert np.array_equal(gone, inside & ~r1["static"]) and r2["done"][gone].all() and r2["reached"][gone].all()
        assert (r2["vel"][gone] == 0).all() and (r2["dist"][gone] > 10000).all()
        return "16 ring agents %.1f - %.1f and %.0f bands off the threshold, 4 on their goal, 4 far, one exactly on the threshold, a " \
            "parked car; %d arrive at step 1 and stand at the padding position after step 2" % (off.min() / band, off[np.arange(16) % 4 < 2].max() / band, WIDE, int(gone.sum()))
    assert not r1["inside"].any() and not r2["done"].any() and not r2["padded"].any()
    return "threshold 0: nobody arrives, 4 agents at distance 0 and a parked car among them"


# ------------------------------------------------------------------------------------------------------------------
# step_done
# ------------------------------------------------------------------------------------------------------------------
def _done_world():
    """0: A, driven onto the parked P (3) by step 1.  1: B, stands on the parked Q (4) from the start.  2: C, 30 m from its goal;
    the last step of the 91-step run puts it there.  5: D, within its threshold: arrives at step 1.  6, 7: E and F, on top of
    each other and both within their thresholds."""
    cars = [GC.car(0, 0.0, 0.0, 0.3), GC.car(1, 20.0, 0.6, 1.2), with_goal(GC.car(2, 40.0, 0.0, 0.1), 40.0, 30.0), CC.parked(3, 0.0, 20.0, 0.5),
            CC.parked(4, 20.0, 0.0, 0.2), with_goal(GC.car(5, 60.0, 0.0, -1.0), 61.0, 0.0), with_goal(GC.car(6, 80.0, 0.0, 0.0), 80.5, 0.0),
            with_goal(GC.car(7, 81.0, 0.5, 2.0), 81.5, 0.5)]
    return world("done", cars)


def _done_actions(run, k, before):
    act = run.hold_pose(before)
    if k == 0:
        act[0, 0, 0:3] = before["state"][0, 3, 0:3]
        act[0, 0, 3] = run.yaw[0, 0] = run.yaw[0, 3]
    if k == 90:
        act[0, 2, 0:2] = before["abs_obs"][0, 2, 8:10]
    return act


def _done_premise(run):
    b0, a0, _ = run.history[0]
    assert (a0[0]["state"][0, :8, 10] != 0).tolist() == [False, True, False, False, True, False, True, True], "B on Q, E on F"
    b1, a1, _ = run.history[1]
    r1 = run.ref(b1[0], a1[0], 0)
    assert a1[0]["state"][0, 0, 10] != 0 and a1[0]["state"][0, 3, 10] != 0, "A must hit P"
    b2, a2, _ = run.history[2]
    r2 = run.ref(b2[0], a2[0], 0)
    stop = run.behaviour != CR.IGNORE
    # Q: done by the movement's collision rule (or not), and within its threshold all the same
    removed = run.behaviour == CR.AGENT_REMOVED
    assert r1["static"][4] and r1["done"][4] and r1["reached"][4] == (not removed) and r1["padded"][4] == removed
    assert r1["padded"][[1, 6, 7]].tolist() == [stop] * 3 and r1["reached"][[6, 7]].tolist() == [not stop] * 2
    assert r1["done"][5] and r1["reached"][5] and r2["padded"][5]
    assert r2["padded"][0] == stop and r2["done"][0] == stop and r2["padded"][3] == (run.behaviour == CR.AGENT_REMOVED)
    text = "behaviour %d: after step 2 done %s, at the padding position %s" % (run.behaviour, r2["done"].astype(int).tolist(), r2["padded"].astype(int).tolist())
    if run.case.steps == 91:
        last = run.history[-1]
        rl = run.ref(last[0][0], last[1][0], 0)
        assert (rl["steps"] == 0).all() and rl["done"].all() and rl["reached"][2] and not run.history[-2][1][0]["done"][0, 2]
        text += "; C arrives with the 91st step, every agent is done at steps_remaining 0"
    return text


# ------------------------------------------------------------------------------------------------------------------
# step_slots128
# ------------------------------------------------------------------------------------------------------------------
def _slots_world():
    """100 of step_wrap's agents and 28 of step_goal's ring agents (standing still under the Classic model: speed 0, zero
    action) in 128 live slots."""
    cars, vel = [], []
    for i in range(100):
        h, _ = _wrap_agent(i)
        x, y = grid(i, 12, 12.0, 11)
        cars.append(GC.car(i, x + 0.011 * i, y - 0.005 * i, h))
        vel.append((WRAP_SPEED * math.cos(h), WRAP_SPEED * math.sin(h), 0.0))
    ring = _goal_cars(100, 28, lambda k: grid(100 + k, 12, 12.0, 11))
    for k in range(4, 28, 6):      # (nothing moves these: they stand 0.5 m from their goals -- nearer than 0.2 m they would be parked)
        g = ring[k]["goalPosition"]
        ring[k]["position"] = [{"x": g["x"] + 0.5, "y": g["y"], "z": 0.0}] * 91
    return world("slots128", cars + ring, vel=vel + [(0.0, 0.0, 0.0)] * 28)


def _slots_actions(run, k, before):
    act = _blank(run)
    yaw = GR.yaw_of(before["state"][..., 3:7])
    for w, wd in enumerate(run.case.worlds):
        for i in range(min(wd.n, 100)):
            act[w, i, 0:3] = _wrap_action(run.model, i, yaw[w, i])
    return act


def _slots_premise(run):
    before, after, _ = run.history[1]
    assert before[0]["shape"][:, 0].tolist() == [128, 3]
    ref = run.ref(before[0], after[0], 0)
    d = ref["driven"]
    assert d.all()
    above, below = int((ref["yaw_sum"] > PI + 1e-4).sum()), int((ref["yaw_sum"] < -PI - 1e-4).sum())
    ring = np.asarray([100 + k for k in range(28) if k % 6 < 4])
    off = np.abs(ref["dist"][ring] - RING)
    assert above >= 8 and below >= 8 and (off >= AIMED_FACTOR * band_of(150.0)).all() and not ref["margin"].any()
    arrive = int(ref["reached"].sum())
    assert arrive == int(ref["inside"][100:].sum()) >= 12 and not ref["inside"][:100].any()
    r2 = run.ref(run.history[2][0][0], run.history[2][1][0], 0)
    assert int(r2["padded"].sum()) == arrive
    return "128 live slots beside 3: %d yaw sums above pi, %d below -pi; %d ring agents arrive, %d do not" % (above, below, arrive, 28 - arrive)


# ------------------------------------------------------------------------------------------------------------------
CASE_LIST = [
    Case("step_wrap", [_wrap_world()], (SR.CLASSIC, SR.BICYCLE, SR.DELTA), _wrap_actions, _wrap_premise, steps=2),
    Case("step_speed", [_speed_world()], (SR.CLASSIC, SR.BICYCLE), _speed_actions, _speed_premise, steps=2),
    Case("step_steer", [_steer_world()], (SR.CLASSIC, SR.BICYCLE), _steer_actions, _steer_premise, steps=1),
    Case("step_far", [_far_world("far_near", 135.0, 150.0), _far_world("far_far", 1350.0, 1500.0)], (SR.CLASSIC, SR.BICYCLE, SR.DELTA),
         _far_actions, _far_premise, steps=2, reward_types=(SR.DISTANCE_BASED,)),
    Case("step_replay", [_replay_world(False)], (SR.CLASSIC,), _replay_actions, _replay_premise, steps=91, extra=dict(maxNumControlledAgents=0),
         reward_types=(SR.DISTANCE_BASED,)),
    Case("step_replay_mixed", [_replay_world(True)], (SR.CLASSIC,), _replay_actions, _replay_premise, steps=91, reward_types=(SR.DISTANCE_BASED,)),
    Case("step_goal", [_goal_world("goal")], (SR.STATE,), _goal_actions, _goal_premise, steps=3, reward_types=(SR.DISTANCE_BASED, SR.ON_GOAL)),
    Case("step_goal_zero", [_goal_world("goal_zero")], (SR.STATE,), _goal_actions, _goal_premise, steps=3, threshold=0.0,
         reward_types=(SR.DISTANCE_BASED, SR.ON_GOAL)),
    Case("step_done", [_done_world()], (SR.STATE,), _done_actions, _done_premise, steps=3, behaviours=(CR.AGENT_STOP, CR.AGENT_REMOVED, CR.IGNORE)),
    Case("step_done91", [_done_world()], (SR.STATE,), _done_actions, _done_premise, steps=91, behaviours=(CR.AGENT_STOP,)),
    Case("step_slots128", [_slots_world(), _wrap_world("ragged", 3, 3)], (SR.CLASSIC,), _slots_actions, _slots_premise, steps=2, slots=128),
]
CASES = {c.name: c for c in CASE_LIST}
RECOMPUTE_AFTER_FIRST_STEP = ("step_goal", "step_goal_zero")     # a pass that moves nothing, away from the start of the episode


def script(run, check):
    """The whole scripted run of run.case: place, every step (and the recompute pass of the goal cases); check(before, after,
    tag, reset_pass) is called with the snapshot lists around every pass."""
    before, after = run.place()
    check(before, after, "reset pass", True)
    for k in range(run.case.steps):
        before, after = run.step(k)
        check(before, after, "step %d" % (k + 1), False)
        if k == 0 and run.case.name in RECOMPUTE_AFTER_FIRST_STEP:
            before, after = run.recompute()
            check(before, after, "recompute pass behind step 1", True)


# ------------------------------------------------------------------------------------------------------------------
# comparison with the reference
# ------------------------------------------------------------------------------------------------------------------
def errors(run, before, after, reset_pass=False, variant=None, raw_yaw=False):
    """One simulator's snapshot `after` a pass against the reference of its snapshot `before` it.  Returns dict(err: {(span,
    column): largest float difference}, bad: [texts of the exact outputs that differ on non-marginal agents], agents, marginal).
    raw_yaw: the heading angle of the absolute row is compared as a number, not modulo 2 pi, on agents whose heading lies
    0.01 away from the seam (how the CPU suite sees a reference variant that does not wrap)."""
    case = run.case
    out = dict(err={}, bad=[], agents=0, marginal=0)

    def put(span, col, v):
        v = np.asarray(v, f64)
        if v.size:
            out["err"][(span, col)] = max(out["err"].get((span, col), 0.0), float(v.max()))

    def exact(w, what, differs, only=None):
        differs = np.asarray(differs)
        if differs.ndim > 1:
            differs = differs.reshape(len(differs), -1).any(-1)
        if only is not None:
            differs = differs & only
        if differs.any():
            out["bad"].append("world %d: %s differs for agents %s" % (w, what, np.nonzero(differs)[0][:8].tolist()))

    for w, wd in enumerate(case.worlds):
        ref = run.ref(before, after, w, reset_pass, variant)
        n = len(ref["x"])
        st, so, ab = after["state"][w, :n], after["self_obs"][w, :n].astype(f64), after["abs_obs"][w, :n]
        pad, ok = ref["padded"], ~ref["margin"]
        here = ~pad
        spans = np.where(pad, PAD_SPAN, wd.span)
        put(wd.span, "pos", np.abs(st[here, 0:2].astype(f64) - np.stack([ref["x"], ref["y"]], -1)[here]))
        exact(w, "the padding position", st[:, 0:2] != f32(SR.PAD_XY), pad)
        exact(w, "z", st[:, 2] != ref["z"].astype(f32))
        yaw_err = np.maximum(SR.angular_distance(GR.yaw_of(st[:, 3:7]), ref["yaw"]),
                             np.maximum(SR.angular_distance(GR.yaw_of(ab[:, 3:7]), ref["yaw"]), SR.angular_distance(ab[:, 7], ref["yaw"])))
        if raw_yaw:
            true = run.ref(before, after, w, reset_pass)["yaw"]
            yaw_err = np.where(np.abs(true) < PI - 0.01, np.abs(ab[:, 7].astype(f64) - ref["yaw"]), yaw_err)
        put(wd.span, "yaw", yaw_err)
        put(wd.span, "vel", np.abs(st[:, 7:10].astype(f64) - ref["vel"]))
        put(wd.span, "speed", np.abs(so[:, 0] - ref["self_obs"][:, 0]))
        for span in (wd.span, PAD_SPAN):
            put(span, "goal", np.abs(so[spans == span, 4:6] - ref["self_obs"][spans == span, 4:6]))
        reward = after["reward"][w, :n].astype(f64)
        if run.reward_type == SR.DISTANCE_BASED:
            for span in (wd.span, PAD_SPAN):
                put(span, "reward", np.abs(reward[spans == span] - ref["reward"][spans == span]))
        else:
            exact(w, "reward", reward != ref["reward"], ok)
        exact(w, "steps remaining", after["steps"][w, :n] != ref["steps"])
        exact(w, "done", (after["done"][w, :n] == 1) != ref["done"], ok)
        exact(w, "info[3]", (after["info"][w, :n, 3] == 1) != ref["reached"], ok)
        exact(w, "the action tensor", after["action"][w, :n] != ref["action"].astype(f32))
        exact(w, "the self row's sizes / collided / id", so[:, [1, 2, 3, 6, 7]] != ref["self_obs"][:, [1, 2, 3, 6, 7]])
        exact(w, "the absolute row's position", ab[:, 0:3] != st[:, 0:3])
        exact(w, "the absolute row's goal / sizes / id", ab[:, 8:14].astype(f64) != np.concatenate([ref["abs_goal"], ref["abs_size"], ref["abs_id"][:, None]], -1))
        out["agents"] += n
        out["marginal"] += int(ref["margin"].sum())
    return out


def ratios(err, factor=1.0):
    """{(span, column): error / (factor * ORACLE_STEP_MAX)}."""
    out = {}
    for (span, col), v in err.items():
        bound = factor * ORACLE_STEP_MAX[span][col]
        out[(span, col)] = v / bound if bound > 0 else (0.0 if v == 0 else float("inf"))
    return out


def hold(run, before, after, tag, factor, reset_pass=False):
    """Raises unless `after` meets the reference of `before`: exact outputs exact outside the margin, float outputs within
    factor * ORACLE_STEP_MAX.  Returns errors() with the ratios added."""
    e = errors(run, before, after, reset_pass)
    e["ratio"] = ratios(e["err"], factor)
    over = {k: v for k, v in e["ratio"].items() if v > 1.0}
    if e["bad"] or over:
        raise AssertionError("%s: %s%s [%d of %d agents are marginal]" % (
            tag, "; ".join(e["bad"]), "; ".join("%s at +-%g m: %.3g is %.2f times its bound" % (c, s, e["err"][(s, c)], v) for (s, c), v in over.items()),
            e["marginal"], e["agents"]))
    return e


def marginal_differences(run, before, after_a, after_b):
    """For a failure text: where two simulators' done / info[3] / reward differ, and whether the reference of the second one's
    tensors calls those agents marginal."""
    lines = []
    for w, wd in enumerate(run.case.worlds):
        ref = run.ref(before, after_b, w)
        n = wd.n
        d = (after_a["done"][w, :n] != after_b["done"][w, :n]) | (after_a["info"][w, :n, 3] != after_b["info"][w, :n, 3]) | \
            (np.abs(after_a["reward"][w, :n] - after_b["reward"][w, :n]) > 0.5)
        if d.any():
            lines.append("world %d: %d agents differ, %d of them marginal" % (w, int(d.sum()), int((d & ref["margin"]).sum())))
    return "; ".join(lines) or "no agent differs in done / info[3] / reward"
