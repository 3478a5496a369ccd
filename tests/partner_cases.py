"""Constructed, MOVING worlds for the partner-row reference (tests/partner_reference.py): each case aims a handful of agents at one
rule of collectPartnerObsSystem or at one store path of the kernels that write the partner rows and the packed heads -- every
phase of the aligned path's tail, ragged worlds either side of one 256-row chunk, a partner exactly on the radius, equal
headings, agents that coincide at the padding position, a world rebuilt with fewer agents -- and asserts its own premise FROM THE
REFERENCE'S INTERMEDIATE VALUES so that it cannot quietly stop exercising that rule.

Scenes are built with the helpers of tests/geom_cases.py and tests/step_cases.py; Case, script and the State-model helpers are
those of tests/road_cases.py.  All cases: polylineReductionThreshold = 0, initOnlyValidAgentsAtFirstStep = 0,
isStaticAgentControlled = 0, collisionBehaviour = Ignore unless the case says otherwise, observationRadius = 50 unless the case
says otherwise, one short lane per world, linear road selection.

TOLERANCES.  Every bound on a float column and the radius band are ORACLE_PARTNER_MAX[span][column]: the largest distance of
the ORACLE (float32, host libm) from the reference over every in-radius pair on every pass of every run of
tests/test_partner_reference.py, per coordinate span of the world.  That suite asserts that the oracle stays within each
constant and that no constant is more than twice what is measured.  The GPU suite allows GPU_FACTOR times the constant -- the
factor and the reason of tests/step_cases.py: the device's double-then-round transcendentals differ from glibc's float ones by
about an ulp -- and no bound is ever taken from a kernel's output.  Speed, size, type, id and both zero rows are exact."""
import json
import math
import os

import numpy as np

from tests import collision_cases as CC
from tests import collision_reference as CR
from tests import geom_cases as GC
from tests import parity as P
from tests import partner_reference as PR
from tests import road_cases as RC
from tests import step_cases as SC
from tests import step_reference as SR

f32 = np.float32
f64 = np.float64
PI = GC.PI
GPU_FACTOR = 2.0
MARGIN_AGENTS = CC.MARGIN_AGENTS          # the share of a case's pairs that may be marginal (not by design)
RADIUS = 50.0
COLUMNS = ("x", "y", "heading", "dist")
ALGO = 1                                  # roadObservationAlgorithm of every run: linear

# span: column: the largest |oracle - reference| (metres, radians), rounded up; the measured value in the comment.  Over the
# pairs the oracle puts inside the radius; dist is sqrt(x * x + y * y) of the float32 row, in float32 -- the radius band.
ORACLE_PARTNER_MAX = {
    # measured: x 1.619e-05, heading 4.989e-07 (partner_slots128), y 1.499e-05, dist 1.800e-05 (partner_counts)
    150.0: dict(x=1.7e-5, y=1.5e-5, heading=5.0e-7, dist=1.9e-5),
    # measured: x 8.022e-06, y 9.444e-06, heading 2.640e-07, dist 8.585e-06 (partner_far: the pairs in reach are as near each other
    # as anywhere, and the difference of two float32 coordinates 1,400 m out is exact)
    1500.0: dict(x=8.1e-6, y=9.5e-6, heading=2.7e-7, dist=8.6e-6),
}


def band_of(span, factor):
    return factor * ORACLE_PARTNER_MAX[span]["dist"]


Case = RC.Case
script = RC.script


class Run(RC.Run):
    """RC.Run on the partner tensors.  passes: dict(tag, reset, snaps: one PR.snapshot per simulator, state) per pass."""

    def __init__(self, case, sims):
        RC.Run.__init__(self, case, sims, None)
        self.spans = [wd.span for wd in case.worlds]

    def _record(self, tag, reset):
        self.passes.append(dict(tag=tag, reset=reset, snaps=[PR.snapshot(s) for s in self.sims], state=SC._get_state(self.sims[0])))
        return self.passes[-1]

    def step(self, k):
        before = dict(state=SC._get_state(self.sims[0]), snap=self.passes[-1]["snaps"][0])
        act = self.case.actions(self, k, before)
        for s in self.sims:
            P.write_actions(s, act)
            s.step()
        return self._record("step %d" % (k + 1), False)

    def ref(self, p, w, factor=GPU_FACTOR, variant=None, sim=0):
        """The reference of world w from simulator `sim`'s own tensors after pass p."""
        key = (p, w, factor, variant, sim)
        if key not in self._refs:
            self._refs[key] = PR.partner_reference(self.passes[p]["snaps"][sim], w, self.case.radius, band_of(self.spans[w], factor), variant)
        return self._refs[key]

    def live(self, p, w):
        return int(self.passes[p]["snaps"][0]["shape"][w, 0])


def _world(name, cars, span=150.0, vel=None):
    return SC.world(name, cars, (), span=span, vel=vel)


def _grid_cars(n, cols, pitch, rows, yaw=lambda i: 0.37 * i - 3.0, first=0):
    return [GC.car(first + i, SC.grid(i, cols, pitch, rows)[0] + 0.013 * i, SC.grid(i, cols, pitch, rows)[1] - 0.007 * i, yaw(i)) for i in range(n)]


def _shift_actions(run, k, before):
    """State model: every step shifts and turns EVERY agent by an amount of its own (agent a by 0.11 + 0.013 a and
    -0.07 - 0.009 a metres and by 0.003 (a + 1) radians), so that every float of x, y and heading of every real row changes with
    every step and a row left over from the pass before cannot pass for the new one (`stale_floats`)."""
    act = run.hold_pose(before)
    shape = before["snap"]["shape"]
    for w in range(len(run.case.worlds)):
        for a in range(int(shape[w, 0])):
            run.put(act, w, a, x=before["state"][w, a, 0] + f32(0.11 + 0.013 * a), y=before["state"][w, a, 1] - f32(0.07 + 0.009 * a),
                    yaw=run.yaw[w, a] + f32(0.003 * (a + 1)))
    return act


def stale_floats(run, p, sim=0):
    """How many x, y and heading floats of the pairs inside the radius after step pass p and after the pass before it hold the
    same bits in both passes' rows (worlds whose agent count changed between them are left out)."""
    same = 0
    for w in range(len(run.case.worlds)):
        now, was = run.ref(p, w, sim=sim), run.ref(p - 1, w, sim=sim)
        if now["n"] != was["n"] or now["n"] < 2:
            continue
        both = now["inside"] & was["inside"]
        m = now["n"] - 1
        a = run.passes[p]["snaps"][sim]["rows"][w, :now["n"], :m, PR.X:PR.HEADING + 1]
        b = run.passes[p - 1]["snaps"][sim]["rows"][w, :now["n"], :m, PR.X:PR.HEADING + 1]
        same += int((a.view(np.uint32) == b.view(np.uint32))[both].sum())
    return same


def _all_rows_change(run):
    steps = [p for p in range(1, len(run.passes)) if not run.passes[p]["reset"]]
    stale = [stale_floats(run, p) for p in steps]
    assert sum(stale) == 0, "x / y / heading floats that keep their bits over a step, per step pass: %s" % stale
    return "every x, y and heading float of every real row changes with each of the %d steps" % len(steps)


def pair_counts(run, p, worlds=None):
    """(pairs, inside, outside, exact verdicts within the band, marginal) over the given worlds after pass p, from the reference."""
    tot = np.zeros(5, np.int64)
    for w in (range(len(run.case.worlds)) if worlds is None else worlds):
        ref = run.ref(p, w)
        at = np.abs(ref["dist"] - run.case.radius) < band_of(run.spans[w], GPU_FACTOR)
        tot += [ref["inside"].size, int(ref["inside"].sum()), int((~ref["inside"]).sum()), int((at & ref["exact"]).sum()), int(ref["near"].sum())]
    return tuple(int(v) for v in tot)


# ------------------------------------------------------------------------------------------------------------------
# partner_counts
# ------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 4, 16, 17, 63, 64)


def _counts_worlds():
    return [_world("n%d" % n, _grid_cars(n, 8, 12.0, 8)) for n in COUNTS]


def _counts_premise(run):
    shape = run.passes[0]["snaps"][0]["shape"]
    assert shape[:, 0].tolist() == list(COUNTS), shape[:, 0]
    slots = run.case.slots
    phases = sorted((n * (slots - 1) * 9) % 4 for n in COUNTS[:4])
    assert phases == [0, 1, 2, 3], "the aligned path's tail must take every phase: %s" % phases
    ragged = [n * (n - 1) for n in COUNTS if n < slots]
    assert 240 in ragged and 272 in ragged and COUNTS[-1] * (slots - 1) % 256 == 192
    seen = []
    for p in range(len(run.passes)):
        pairs, inside, outside, _, marginal = pair_counts(run, p)
        assert inside > 1000 and outside > 1000 and marginal == 0, (p, inside, outside, marginal)
        seen.append((inside, outside))
    return "agents per world %s; tail phases %s; ragged rows %s; (inside, outside) pairs per pass %s; %s" % (list(COUNTS), phases, ragged, seen, _all_rows_change(run))


# ------------------------------------------------------------------------------------------------------------------
# partner_radius
# ------------------------------------------------------------------------------------------------------------------
RADIUS_AIMS, RADIUS_WANT = RC.RADIUS_AIMS, RC.RADIUS_WANT
RING_TURN = 0.7


def _ring_world(name, turn):
    """Agent 0 (the ego, at yaw `turn`) and eight partners near R(turn) * their aims; step 1 puts them there to the float."""
    c, s = math.cos(turn), math.sin(turn)
    cars = [GC.car(0, 0.0, 0.0, turn)]
    cars += [GC.car(1 + a, c * dx - s * dy + 1.0, s * dx + c * dy - 1.0, turn) for a, (dx, dy) in enumerate(RADIUS_AIMS)]
    return _world(name, cars)


def _ring_place(turn, dx, dy):
    """R(turn) (dx, dy) in float32 (exactly (dx, dy) at turn 0)."""
    c, s = f32(math.cos(turn)), f32(math.sin(turn))
    return f32(c * f32(dx) - s * f32(dy)), f32(s * f32(dx) + c * f32(dy))


def _radius_actions(run, k, before):
    """Step 1 puts the ego on (0, 0) and partner a on its aim (world 1: turned by the ego's yaw); step 2 hands the poses back;
    step 3 moves every partner on to the next partner's aim."""
    act = run.hold_pose(before)
    if k in (0, 2):
        for w, turn in enumerate((0.0, RING_TURN)):
            run.put(act, w, 0, x=0.0, y=0.0)
            for a in range(8):
                x, y = _ring_place(turn, *RADIUS_AIMS[(a + (k == 2)) % 8])
                run.put(act, w, 1 + a, x=x, y=y)
    return act


def _radius_premise(run):
    texts = []
    assert np.array_equal(run.passes[1]["snaps"][0]["abs_obs"][0, :9, 3:7], np.tile(np.asarray([1, 0, 0, 0], f32), (9, 1))), "world 0: every rotation the identity"
    for p, shift in ((1, 0), (2, 0), (3, 1)):
        ref, rot = run.ref(p, 0), run.ref(p, 1)
        got = []
        for a in range(8):
            aim = RADIUS_AIMS[(a + shift) % 8]
            want_in = RADIUS_WANT[(a + shift) % 8]
            d = math.hypot(*aim)
            # ego -> partner: slot a of agent 0; partner -> ego: slot 0 of agent 1 + a
            for i, k in ((0, a), (1 + a, 0)):
                assert ref["exact"][i, k] and ref["dist"][i, k] == d and not ref["near"][i, k], "pass %d pair (%d, slot %d): offset %r is not exact (distance %r)" % (p, i, k, aim, ref["dist"][i, k])
                assert ref["inside"][i, k] == want_in
                assert rot["near"][i, k] and not rot["exact"][i, k], "pass %d: the rotated ring's pair (%d, slot %d) must be marginal (distance %r)" % (p, i, k, rot["dist"][i, k])
            got.append("%+.1f" % ((d - RADIUS) / float(np.spacing(f32(50)))))
        assert int(ref["near"].sum()) == 0 and int(rot["near"].sum()) == 16, (int(ref["near"].sum()), int(rot["near"].sum()))
        at = np.abs(ref["dist"] - RADIUS) < band_of(150.0, GPU_FACTOR)
        assert int((at & ref["exact"]).sum()) == 16
        texts.append("pass %d: partners at radius %s ulp, 16 exact verdicts, 16 marginal pairs by design on the rotated ring" % (p, " ".join(got)))
    return "; ".join(texts)


def _zero_world():
    """observationRadius = 0: 0 and 1 stand within their goal thresholds (they arrive at step 1 and stand on the padding position
    from step 2 on); 2 and 3 stand 5 m apart, 4 a millimetre from 3."""
    cars = [SC.with_goal(GC.car(0, 10.0, 10.0, 0.5), 11.0, 10.0), SC.with_goal(GC.car(1, -15.0, 30.0, -2.0), -15.5, 30.5),
            GC.car(2, 7.0, -20.0, 1.0), GC.car(3, 12.0, -20.0, 2.0), GC.car(4, 12.001, -20.0, 0.0)]
    return _world("zero", cars)


def _zero_actions(run, k, before):
    return run.hold_pose(before)


def _zero_premise(run):
    assert run.case.radius == 0.0
    pad = lambda p: run.passes[p]["state"][0, :5, 2] == CR.PAD_Z
    assert not pad(0).any() and pad(2)[[0, 1]].all() and not pad(2)[2:].any(), "agents 0 and 1 stand at the padding position after step 2: %s" % pad(2)
    for p in range(len(run.passes)):
        ref = run.ref(p, 0)
        both = pad(p)[0] and pad(p)[1]
        want = np.zeros((5, 4), bool)
        if both:
            want[0, 0] = want[1, 0] = True          # 0 sees 1 in slot 0, 1 sees 0 in slot 0
            assert ref["dist"][0, 0] == 0 and ref["exact"][0, 0] and ref["exact"][1, 0]
        assert np.array_equal(ref["inside"], want) and not ref["near"].any(), (p, ref["inside"], ref["near"])
        assert ref["dist"][~want].min() > 1e-7
    return "radius 0: every separated pair is out (the nearest %.3g m apart); the two agents at the padding position see each other at distance 0 on passes %s" % (
        float(run.ref(0, 0)["dist"].min()), [p for p in range(len(run.passes)) if pad(p)[[0, 1]].all()])


# ------------------------------------------------------------------------------------------------------------------
# partner_headings
# ------------------------------------------------------------------------------------------------------------------
HEADINGS = SC.HEADINGS


def _headings_world():
    return _world("headings", _grid_cars(18, 6, 7.0, 3, yaw=lambda i: HEADINGS[i % 9]))


def _heading_index(a, p):
    """Which heading of the set agent a has after pass p."""
    return (a + (3 + a // 9) * p) % 9


def _headings_actions(run, k, before):
    """Step k turns agent a to another heading of the set (the second nine by another stride) and shifts it by 0.3 m."""
    act = run.hold_pose(before)
    for a in range(18):
        h = HEADINGS[_heading_index(a, k + 1)]
        run.put(act, 0, a, x=before["state"][0, a, 0] + f32(0.3), y=before["state"][0, a, 1] + f32(0.1), yaw=h)
    return act


def _headings_premise(run):
    texts = []
    seen = set()
    for p in range(len(run.passes)):
        snap = run.passes[p]["snaps"][0]
        ref = run.ref(p, 0)
        assert ref["inside"].all() and not ref["near"].any()
        zero, opposite = PR.same_heading_pairs(snap["abs_obs"][0, :18, 3:7])
        off = ~np.eye(18, dtype=bool)
        n_zero, n_opp = int((zero & off).sum()), int((opposite & off).sum())
        assert n_zero >= 18, "every heading is held by two agents: %d pairs with w * z == 0" % n_zero
        yaw = snap["abs_obs"][0, :18, 7].astype(f64)
        raw = yaw[ref["J"]] - yaw[:, None]
        seam = int((np.abs(raw) > PI).sum())
        at_pi = int((np.abs(np.abs(ref["obs"][..., PR.HEADING]) - PI) < 1e-6).sum())
        assert seam >= 40 and at_pi >= 8, (seam, at_pi)
        seen |= {(_heading_index(a, p), _heading_index(b, p)) for a in range(18) for b in range(18) if a != b}
        texts.append("pass %d: %d ordered pairs with w * z == 0 (%d of them with w == 0), %d differences beyond +-pi, %d relative headings at +-pi" % (p, n_zero, n_opp, seam, at_pi))
    missing = {(a, b) for a in range(9) for b in range(9)} - seen
    assert not missing, "ordered heading pairs never seen: %s" % sorted(missing)[:6]
    return "; ".join(texts) + "; every ordered pair of the nine headings occurs (the w * z == 0 branch is reached by construction: counted on the host in plain float32, not observed on the device)"


# ------------------------------------------------------------------------------------------------------------------
# partner_columns
# ------------------------------------------------------------------------------------------------------------------
BIG_ID = 2 ** 31 - 1
COLUMN_IDS = (0, 1, 7, 255, 256, 65536, 16777216, 16777217, 33554433, 1000000007, 2 ** 31 - 129, BIG_ID)
COLUMN_SIZES = ((0.5, 0.5, 0.3), (4.0, 2.0, 1.6), (12.0, 2.5, 3.5), (22.0, 3.0, 4.0))
COLUMN_KINDS = ("vehicle", "pedestrian", "cyclist")
COLUMN_VEL = ((0.0, 0.0, 0.0), (60.0, 0.0, 0.0), (3.0, 4.0, 12.0), (0.0, 0.0, 2.5), (-36.0, 48.0, 0.0), (1.0, -2.0, 2.0))


def _columns_world():
    cars, vel = [], []
    for i in range(12):
        length, width, height = COLUMN_SIZES[i % 4]
        x, y = SC.grid(i, 4, 9.0, 3)
        c = GC.car(COLUMN_IDS[i], x + 0.02 * i, y - 0.01 * i, 0.5 * i - 3.0, length=length, width=width, kind=COLUMN_KINDS[i % 3])
        c["height"] = height
        cars.append(c)
        vel.append(COLUMN_VEL[i % 6])
    return _world("columns", cars, vel=vel)


def _columns_premise(run):
    for p in range(len(run.passes)):
        snap = run.passes[p]["snaps"][0]
        ref = run.ref(p, 0)
        assert ref["n"] == 12 and ref["inside"].all() and not ref["near"].any()
        ab = snap["abs_obs"][0, :12]
        assert set(ab[:, 10].tolist()) == {0.5, 4.0, 12.0, 22.0} and set(ab[:, 12].tolist()) == {float(f32(v)) for v in (0.3, 1.6, 3.5, 4.0)}
        assert set(snap["etype"][0, :12].tolist()) == {7, 8, 9}, "vehicle, pedestrian and cyclist: %s" % snap["etype"][0, :12]
        assert sorted(ab[:, 13].tolist()) == sorted(float(f32(v)) for v in COLUMN_IDS) and ab[:, 13].max() == f32(BIG_ID)
        vel = run.passes[p]["state"][0, :12, 7:10].astype(f64)
        speed = snap["self_obs"][0, :12, 0].astype(f64)
        assert (np.abs(speed - np.sqrt((vel ** 2).sum(-1))) < 1e-5).all(), "the self-row speed is the 3-vector's length"
        rising = vel[:, 2] != 0
        assert rising.sum() >= 6 and (speed[rising] > np.hypot(vel[rising, 0], vel[rising, 1]) + 0.1).all() and speed.min() == 0 and speed.max() >= 60
    return "12 agents: lengths 0.5 - 22 m, vehicle / pedestrian / cyclist, ids up to 2^31 - 1, speeds 0 ... 60 m/s, %d with vz != 0" % int(rising.sum())


# ------------------------------------------------------------------------------------------------------------------
# partner_far
# ------------------------------------------------------------------------------------------------------------------
def _far_world(name, span):
    """Four clusters of four agents in the corners of the span (their mean, which the parser subtracts, stays at the centre)."""
    cars = []
    for c, (sx, sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
        for a, (dx, dy) in enumerate(((0.0, 0.0), (-17.0, 9.0), (8.0, -31.0), (-30.0, -28.0))):
            cars.append(GC.car(4 * c + a, sx * (0.93 * span + dx), sy * (0.9 * span + dy), 0.8 * (4 * c + a) - 3.0))
    return _world(name, cars, span=span)


def _far_premise(run):
    out = []
    for w, wd in enumerate(run.case.worlds):
        for p in range(len(run.passes)):
            xy = np.abs(run.passes[p]["state"][w, :16, 0:2]).max()
            assert 0.8 * wd.span <= xy <= wd.span, (w, xy)
            ref = run.ref(p, w)
            assert int(ref["inside"].sum()) >= 40 and int((~ref["inside"]).sum()) >= 192 and not ref["near"].any(), (int(ref["inside"].sum()), int(ref["near"].sum()))
        out.append("world %d within +-%.0f m (largest coordinate %.0f), %d pairs inside" % (w, wd.span, xy, int(ref["inside"].sum())))
    return "; ".join(out)


# ------------------------------------------------------------------------------------------------------------------
# partner_moves
# ------------------------------------------------------------------------------------------------------------------
def _moves_world(name):
    """0: a logged agent (expert) that drives 0.5 m a step.  1, 2: within their goal thresholds (they arrive at step 1, stand on the
    padding position from step 2 on and come back with the world's reset).  3: driven onto the parked 4 at step 1 (AgentRemoved:
    both go to the padding position).  5: crosses the radius around the parked 6, out at steps 1 and 3, in at steps 2 and 4.  7, 8:
    swap places every step.  9: parked."""
    k = np.arange(91)
    logged = SC.moving_car(0, -40.0 + 0.5 * k, -20.0 + 0.0 * k, [0.2] * 91, [5.0] * 91, [0.0] * 91, expert=True)
    cars = [logged, SC.with_goal(GC.car(1, 10.0, 10.0, 0.5), 11.0, 10.0), SC.with_goal(GC.car(2, -15.0, 30.0, -2.0), -15.5, 30.5),
            GC.car(3, 30.0, -30.0, 1.0), CC.parked(4, 30.0, -22.0, 0.3), GC.car(5, -10.0, 51.0, 2.8), CC.parked(6, -10.0, 2.0, -1.3),
            GC.car(7, 25.0, 20.0, 0.0), GC.car(8, -35.0, 12.0, 3.0), CC.parked(9, 0.0, -45.0, 0.7)]
    return _world(name, cars)


def _moves_actions(run, k, before):
    act = run.hold_pose(before)
    st = before["state"]
    for w in range(2):
        if k == 0:
            act[w, 3, 0:3] = st[w, 4, 0:3]
            act[w, 3, 3] = run.yaw[w, 3] = run.yaw[w, 4]
        if st[w, 5, 2] != CR.PAD_Z:
            run.put(act, w, 5, y=st[w, 5, 1] + (f32(3.0) if k % 2 == 0 else f32(-3.0)), yaw=run.yaw[w, 5] + f32(0.3))
        if st[w, 7, 2] != CR.PAD_Z and st[w, 8, 2] != CR.PAD_Z:
            run.put(act, w, 7, x=st[w, 8, 0], y=st[w, 8, 1])
            run.put(act, w, 8, x=st[w, 7, 0], y=st[w, 7, 1])
    return act


def _moves_reset(run):
    """World 0 is reset; world 1 keeps stepping."""
    for s in run.sims:
        s.reset([0])
    run.yaw[0, :run.case.worlds[0].n] = run.case.worlds[0].yaw
    return "reset of world 0 behind step 3"


def _moves_premise(run):
    """passes: 0 reset pass, 1-3 steps, 4 the reset of world 0, 5-6 steps."""
    pad = lambda p, w: (run.passes[p]["state"][w, :10, 2] == CR.PAD_Z)
    gone = [1, 2, 3, 4]
    assert pad(2, 0)[gone].all() and pad(2, 1)[gone].all() and not pad(2, 0)[[0, 5, 6, 7, 8, 9]].any(), "arrived and removed agents stand at the padding position: %s" % pad(2, 0)
    assert not pad(4, 0).any() and pad(4, 1)[gone].all() and pad(6, 1)[gone].all(), "the reset brings world 0 back, world 1 keeps stepping"
    ref = run.ref(2, 0)
    J = ref["J"]
    among = np.isin(J, gone) & np.isin(np.arange(10), gone)[:, None]
    assert (ref["dist"][among] == 0).all() and ref["inside"][among].all() and ref["exact"][among].all(), "padded agents coincide"
    rest = np.isin(np.arange(10), gone)[:, None] & ~among
    assert not ref["inside"][rest].any(), "a padded ego sees nobody else"
    # 5 around 6: slot 5 of ego 5 is agent 6, slot 5 of ego 6 is agent 5
    cross = [bool(run.ref(p, 1)["inside"][5, 5]) for p in range(len(run.passes))]
    assert cross == [True, False, True, False, False, True, False], "agent 5 crosses the radius around agent 6 in both directions: %s" % cross
    a, b = run.passes[0]["state"][1], run.passes[1]["state"][1]
    assert np.array_equal(a[7, 0:2], b[8, 0:2]) and np.array_equal(a[8, 0:2], b[7, 0:2]), "agents 7 and 8 swap places"
    x0 = [float(p["state"][1, 0, 0]) for p in run.passes]
    assert x0[3] - x0[0] > 0.9, "the logged agent drives on: %s" % x0
    near = [pair_counts(run, p)[4] for p in range(len(run.passes))]
    assert max(near) == 0, near
    snap = run.passes[0]["snaps"][0]
    return "4 agents per world at the padding position after step 2 (they see each other at distance 0, nobody else), back after the reset of world 0 alone; " \
        "agent 5 inside agent 6's radius on passes %s; 7 and 8 swap places; a logged agent (x %s) and 3 parked cars beside the controlled ones" % (
            [p for p, c in enumerate(cross) if c], [round(v, 1) for v in x0[:4]])


def _classic_world():
    """Classic model, zero actions: 0 drives away from the standing 1 at 60 m/s (out at step 2), 2 drives towards it (in at
    step 3), 3 rises at vz = 5 on the spot, 4 and 5 are parked."""
    spec = ((40.0, 0.0, 0.0, 60.0), (0.0, 3.0, 1.0, 0.0), (-66.0, -3.0, 0.0, 60.0), (10.0, -30.0, 2.0, 0.0))
    cars, vel = [], []
    for a, (x, y, h, v) in enumerate(spec):
        gx, gy = (x + 140.0 * math.cos(h), y + 140.0 * math.sin(h)) if v else (x, y + 100.0)
        cars.append(SC.with_goal(GC.car(a, x, y, h), gx, gy))
        vel.append((v * math.cos(h), v * math.sin(h), 5.0 if a == 3 else 0.0))
    cars += [CC.parked(4, -30.0, 25.0, 0.7), CC.parked(5, 25.0, 30.0, -2.1)]
    return _world("classic", cars, vel=vel + [(0.0, 0.0, 0.0)] * 2)


def _classic_actions(run, k, before):
    return RC._blank(run)


def _classic_premise(run):
    away = [bool(run.ref(p, 0)["inside"][1, 0]) for p in range(len(run.passes))]        # ego 1, slot 0: agent 0
    towards = [bool(run.ref(p, 0)["inside"][1, 1]) for p in range(len(run.passes))]     # ego 1, slot 1: agent 2
    assert away == [True, True, False, False, False] and towards == [False, False, False, True, True], (away, towards)
    step = np.hypot(*(run.passes[2]["state"][0, [0, 2], 0:2] - run.passes[1]["state"][0, [0, 2], 0:2]).T)
    assert (np.abs(step - 6.0) < 0.01).all(), step
    assert max(pair_counts(run, p)[4] for p in range(len(run.passes))) == 0
    speed = run.passes[0]["snaps"][0]["self_obs"][0, :6, 0]
    assert abs(speed[3] - 5.0) < 1e-5 and speed[1] == 0
    return "Classic: agent 0 leaves agent 1's radius at step 2 (%s), agent 2 enters it at step 3 (%s), 6 m a step" % (away, towards)


# ------------------------------------------------------------------------------------------------------------------
# partner_rebuild
# ------------------------------------------------------------------------------------------------------------------
REBUILD_BIG, REBUILD_SMALL, REBUILD_OTHER = 40, 5, 7


def _rebuild_worlds():
    big = _world("rebuild_big", _grid_cars(REBUILD_BIG, 8, 11.0, 5))
    other = _world("rebuild_other", _grid_cars(REBUILD_OTHER, 4, 13.0, 2, yaw=lambda i: 0.9 * i))
    return [big, other]


REBUILD_SMALL_WORLD = _world("rebuild_small", _grid_cars(REBUILD_SMALL, 3, 23.0, 2, yaw=lambda i: -0.6 * i + 1.0, first=100))


def _rebuild_to(world, which):
    def event(run):
        for s in run.sims:
            s.set_maps([run.scene_paths[which], run.scene_paths[1]])
        run.yaw[0, :] = 0
        run.yaw[0, :world.n] = world.yaw
        run.yaw[1, :REBUILD_OTHER] = run.case.worlds[1].yaw
        return "set_maps to %d agents" % world.n
    return event


def _rebuild_premise(run):
    """passes: 0 reset pass, 1-2 steps, 3 set_maps (5 agents), 4-5 steps, 6 set_maps (40 agents), 7 a step."""
    n = [run.live(p, 0) for p in range(len(run.passes))]
    assert n == [40, 40, 40, 5, 5, 5, 40, 40] and all(run.live(p, 1) == REBUILD_OTHER for p in range(len(run.passes))), n
    assert [ps["reset"] for ps in run.passes] == [True, False, False, True, False, False, True, False]
    ids = [sorted(run.passes[p]["snaps"][0]["abs_obs"][0, :n[p], 13].astype(int).tolist())[0] for p in (2, 3, 6)]
    assert ids == [0, 100, 0], ids
    for p in (4, 5):
        rows = run.passes[p]["snaps"][0]["rows"][0, :5]
        assert (rows[:, 4:, 8] == -2).all() and (rows[:, :4, 8] >= -1).all()
    inside = [pair_counts(run, p, [0])[1] for p in range(len(run.passes))]
    assert min(inside) >= 4
    return "agents of world 0 per pass %s (beside a world of %d); inside pairs %s; %s" % (n, REBUILD_OTHER, inside, _all_rows_change(run))


# ------------------------------------------------------------------------------------------------------------------
# partner_slots128
# ------------------------------------------------------------------------------------------------------------------
def _slots_worlds():
    return [_world("s127", _grid_cars(127, 16, 9.0, 8)), _world("s128", _grid_cars(128, 16, 9.0, 8, yaw=lambda i: -0.21 * i + 2.0)),
            _world("s3", _grid_cars(3, 3, 20.0, 1))]


def _slots_premise(run):
    shape = run.passes[0]["snaps"][0]["shape"]
    assert shape[:, 0].tolist() == [127, 128, 3] and run.passes[0]["snaps"][0]["rows"].shape[1:] == (128, 127, 9)
    pairs, inside, outside, _, marginal = pair_counts(run, 1)
    assert inside > 5000 and outside > 5000 and marginal <= MARGIN_AGENTS * pairs
    return "127 and 128 live agents in 128 slots beside a ragged world of 3: %d pairs inside, %d outside; %s" % (inside, outside, _all_rows_change(run))


# ------------------------------------------------------------------------------------------------------------------
CASE_LIST = [
    Case("partner_counts", _counts_worlds(), SR.STATE, _shift_actions, _counts_premise, steps=2),
    Case("partner_radius", [_ring_world("ring", 0.0), _ring_world("ring_turned", RING_TURN)], SR.STATE, _radius_actions, _radius_premise, steps=3),
    Case("partner_radius_zero", [_zero_world()], SR.STATE, _zero_actions, _zero_premise, steps=3, radius=0.0),
    Case("partner_headings", [_headings_world()], SR.STATE, _headings_actions, _headings_premise, steps=2),
    Case("partner_columns", [_columns_world()], SR.STATE, _shift_actions, _columns_premise, steps=2),
    Case("partner_far", [_far_world("far_near", 150.0), _far_world("far_far", 1500.0)], SR.STATE, _shift_actions, _far_premise, steps=2),
    Case("partner_moves", [_moves_world("moves_a"), _moves_world("moves_b")], SR.STATE, _moves_actions, _moves_premise, steps=5,
         behaviour=CR.AGENT_REMOVED, events={2: _moves_reset}),
    Case("partner_moves_classic", [_classic_world()], SR.CLASSIC, _classic_actions, _classic_premise, steps=4),
    Case("partner_rebuild", _rebuild_worlds(), SR.STATE, _shift_actions, _rebuild_premise, steps=5,
         events={1: _rebuild_to(REBUILD_SMALL_WORLD, 2), 3: _rebuild_to(_rebuild_worlds()[0], 0)}),
    Case("partner_slots128", _slots_worlds(), SR.STATE, _shift_actions, _slots_premise, steps=2, slots=128),
]
CASES = {c.name: c for c in CASE_LIST}
DESIGNED_MARGINAL = {"partner_radius": (1,)}       # worlds whose marginal pairs are there on purpose: the turned ring
SECOND_STREAM = ("partner_counts", "partner_headings", "partner_moves")      # run once more with GPUDRIVE_SPLIT_PARTNER=1, and with GPUDRIVE_NO_POSE_SKIP=1
PACKED = ("partner_counts", "partner_radius", "partner_moves", "partner_slots128")
LAYOUTS = ("direct", "rows", "conditioned")


def write_scenes(case, directory):
    """The case's scene files; for partner_rebuild also the world its first set_maps loads."""
    paths = case.write(directory)
    if case.name == "partner_rebuild":
        other = os.path.join(str(directory), "rebuild_small.json")
        with open(other, "w") as f:
            json.dump(REBUILD_SMALL_WORLD.scene, f)
        paths = paths + [other]
    return paths


# ------------------------------------------------------------------------------------------------------------------
# comparison with the reference
# ------------------------------------------------------------------------------------------------------------------
def errors(run, p, factor, variant=None, sim=0):
    """Simulator `sim`'s partner rows after pass p against the reference of its own tensors.  Returns dict(err: {(span, column):
    largest float difference over the rows it puts inside}, bad: [texts of what differs beyond the floats], pairs, marginal,
    designed (marginal pairs of the worlds that are marginal by design), inside, outside, exact)."""
    case = run.case
    out = dict(err={}, bad=[], pairs=0, marginal=0, designed=0, inside=0, outside=0, exact=0)
    snap = run.passes[p]["snaps"][sim]
    for w in range(len(case.worlds)):
        span = run.spans[w]
        ref = run.ref(p, w, factor, variant, sim)
        base = ref if variant is None else run.ref(p, w, factor, None, sim)         # (margins are the true rule's)
        n, m = ref["n"], max(ref["n"] - 1, 0)
        rows32 = snap["rows"][w, :n]
        got = rows32.astype(f64)
        where = "world %d" % w
        if not np.isfinite(got).all():
            out["bad"].append("%s: rows that are not finite" % where)
            continue
        tail = PR.is_zero_row(got[:, m:], ref["pad_row"])
        if not tail.all():
            bad = np.argwhere(~tail)[0]
            out["bad"].append("%s: ego %d slot %d (>= n - 1 = %d) is not %s: %s" % (where, bad[0], m + bad[1], m, ref["pad_row"].tolist(), got[bad[0], m + bad[1]].tolist()))
        real = got[:, :m]
        near = base["near"]
        said_out = PR.is_zero_row(real, ref["out_row"])
        wrong = (said_out == ref["inside"]) & ~near
        if wrong.any():
            i, k = np.argwhere(wrong)[0]
            out["bad"].append("%s: ego %d slot %d at %.9g m is %s, the reference puts it %s the radius (%d such pairs)" % (
                where, i, k, ref["dist"][i, k], "the zero row" if said_out[i, k] else "a real row", "inside" if ref["inside"][i, k] else "outside", int(wrong.sum())))
        chk = ~said_out & ~wrong
        want = ref["obs"]
        differs = (real[..., PR.EXACT_COLS] != want[..., PR.EXACT_COLS].astype(f32).astype(f64)).any(-1) & chk
        if differs.any():
            i, k = np.argwhere(differs)[0]
            out["bad"].append("%s: ego %d slot %d: speed / size / type / id %s are not agent %d's %s" % (
                where, i, k, real[i, k, PR.EXACT_COLS].tolist(), ref["J"][i, k], want[i, k, PR.EXACT_COLS].tolist()))

        def put(col, v):
            if v.size:
                out["err"][(span, col)] = max(out["err"].get((span, col), 0.0), float(np.max(v)))
        put("x", np.abs(real[..., PR.X] - want[..., PR.X])[chk])
        put("y", np.abs(real[..., PR.Y] - want[..., PR.Y])[chk])
        put("heading", (np.abs(real[..., PR.HEADING] - want[..., PR.HEADING]) if variant == "no_heading_wrap" else PR.angular_distance(real[..., PR.HEADING], want[..., PR.HEADING]))[chk])
        g32 = rows32[:, :m]
        d32 = np.sqrt(g32[..., PR.X] * g32[..., PR.X] + g32[..., PR.Y] * g32[..., PR.Y])
        put("dist", np.abs(d32.astype(f64) - ref["dist"])[chk])
        out["pairs"] += near.size
        out["designed" if w in DESIGNED_MARGINAL.get(case.name, ()) else "marginal"] += int(near.sum())
        out["inside"] += int(base["inside"].sum())
        out["outside"] += int((~base["inside"]).sum())
        at = np.abs(base["dist"] - case.radius) < band_of(span, factor)
        out["exact"] += int((at & base["exact"]).sum())
    return out


def ratios(err, factor=1.0):
    return {(span, col): v / (factor * ORACLE_PARTNER_MAX[span][col]) for (span, col), v in err.items()}


def hold(run, p, factor, sim=0):
    """Raises unless simulator `sim`'s rows after pass p meet the reference: verdicts outside the margin mask, both zero rows and
    the exact columns exact, float columns within factor * ORACLE_PARTNER_MAX.  Returns errors() with the ratios added."""
    e = errors(run, p, factor, sim=sim)
    e["ratio"] = ratios(e["err"], factor)
    over = {k: v for k, v in e["ratio"].items() if v > 1.0}
    if e["bad"] or over:
        raise AssertionError("%s, %s: %s%s [%d of %d pairs marginal, %d more by design]" % (
            run.case.name, run.passes[p]["tag"], "; ".join(e["bad"][:4]),
            "; ".join("%s at +-%g m: %.3g is %.2f times its bound" % (c, s, e["err"][(s, c)], v) for (s, c), v in over.items()),
            e["marginal"], e["pairs"], e["designed"]))
    return e


def rows_against(run, p, sim_a, sim_b, atol):
    """Simulator sim_a's whole partner tensor against sim_b's within atol, element by element, outside the pairs the reference
    (of sim_b's tensors) calls marginal.  Returns how many pairs that leaves out."""
    a, b = run.passes[p]["snaps"][sim_a]["rows"], run.passes[p]["snaps"][sim_b]["rows"]
    ok = np.isclose(a, b, atol=atol, rtol=0)
    skipped = 0
    for w in range(len(run.case.worlds)):
        ref = run.ref(p, w, GPU_FACTOR, None, sim_b)
        i, k = np.nonzero(ref["near"])
        ok[w, i, k] = True
        skipped += len(i)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError("partner_observations_tensor: %d elements beyond atol %g; first at %s: %r against %r" % (len(bad), atol, bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))
    return skipped


# ------------------------------------------------------------------------------------------------------------------
# the packed heads
# ------------------------------------------------------------------------------------------------------------------
def head_errors(run, p, heads, slots_of_row, factor, sim):
    """Packed heads [R, 6 + (A - 1) * 6] (row r: the head of slot slots_of_row[r] = (world, agent)) against the float64 packing of
    the reference rows of simulator `sim`'s own tensors: every column within PACK_ATOL + PACK_RTOL |want| + the raw bound
    carried through the column's gain (the heading column modulo one turn); the slots of marginal pairs may hold either row.
    Returns (worst error / bound, texts of what is beyond it)."""
    snap = run.passes[p]["snaps"][sim]
    A1 = snap["rows"].shape[2]
    gain = PR.head_gain(A1)
    worst, bad = 0.0, []
    for r, (w, a) in enumerate(slots_of_row):
        ref = run.ref(p, w, factor, None, sim)
        b = ORACLE_PARTNER_MAX[run.spans[w]]
        raw = np.zeros(9)
        raw[[PR.X, PR.Y, PR.HEADING]] = factor * b["x"], factor * b["y"], factor * b["heading"]
        raw_bound = np.concatenate([np.zeros(6), np.tile(raw[:6], A1)])
        want = PR.packed_head(snap["self_obs"][w, a], ref["rows"][a])
        got = np.asarray(heads[r], f64)
        diff = np.abs(got - want)
        turn = np.zeros(len(want), bool)
        turn[6 + PR.HEADING::6] = True
        diff = np.where(turn, np.minimum(diff, np.abs(1.0 - diff)), diff)
        bound = P.PACK_ATOL + P.PACK_RTOL * np.abs(want) + raw_bound * gain
        near = np.zeros(A1, bool)
        near[:ref["near"].shape[1]] = ref["near"][a]
        if near.any():       # either the packed zero row or the packed real row
            other = PR.packed_head(snap["self_obs"][w, a], np.where(ref["inside"][a][:, None], ref["out_row"], ref["obs"][a]))
            alt = np.abs(got[6:6 + 6 * ref["near"].shape[1]] - other[6:])
            sl = np.repeat(near[:ref["near"].shape[1]], 6)
            diff[6:6 + len(alt)][sl] = np.minimum(diff[6:6 + len(alt)][sl], alt[sl])
        ratio = diff / bound
        if not np.isfinite(got).all() or ratio.max() > 1.0:
            c = int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf)))
            bad.append("world %d agent %d column %d: %r against %r (%.2f times its bound)" % (w, a, c, got[c], want[c], ratio[c]))
        else:
            worst = max(worst, float(ratio.max()))
    return worst, bad
