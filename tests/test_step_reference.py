"""CPU suite: the float64 step reference (tests/step_reference.py) against hand-worked answers, the oracle against the
reference on the constructed worlds of tests/step_cases.py after the reset pass and after every step, the cases' premises and
margin condition, the measured constants (ORACLE_STEP_MAX: the oracle stays within each, and none is more than twice what is
measured), and the sensitivity of the cases: every wrong-rule variant of the reference disagrees with the oracle on the case
that aims at its rule."""
import functools
import math
import tempfile

import numpy as np
import pytest

from tests import collision_reference as CR
from tests import parity as P
from tests import step_cases as SC
from tests import step_reference as SR
from tests.test_columns import check_partner_rows_by_brute_force

f32 = np.float32
ALL_RUNS = [r for c in SC.CASE_LIST for r in c.runs()]


# ------------------------------------------------------------------------------------------------------------------
# the reference itself, against answers worked out by hand
# ------------------------------------------------------------------------------------------------------------------
def _one_agent(yaw=0.0, vel=(0.0, 0.0, 0.0), action=(0.0,) * 10, pos=(0.0, 0.0, 1.0), goal=(100.0, 0.0), length=4.0, width=2.0,
               steps=91, done=0, reached=0, collided=0, controlled=1, static=0, traj=None):
    st = np.zeros((1, 1, 11), f32)
    st[0, 0] = pos + (math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)) + tuple(vel) + (collided,)
    ab = np.zeros((1, 1, 14), f32)
    ab[0, 0, 8:14] = goal + (length, width, 1.6, 7.0)
    info = np.zeros((1, 1, 5), np.int32)
    info[0, 0, 3] = reached
    before = dict(shape=np.asarray([[1, 1]], np.int32), state=st, abs_obs=ab, self_obs=np.zeros((1, 1, 8), f32), info=info,
                  controlled=np.full((1, 1), controlled, np.int32), resp=np.full((1, 1), 2 if static else 0, np.int32),
                  done=np.full((1, 1), done, np.int32), steps=np.full((1, 1), steps, np.int64), action=np.asarray(action, f32).reshape(1, 1, 10),
                  reward=np.zeros((1, 1), f32), traj=np.zeros((1, 1, 16 * 91), f32) if traj is None else traj)
    return before, dict(state=st.copy())


def _ref(model=SR.CLASSIC, behaviour=CR.IGNORE, reward=SR.DISTANCE_BASED, threshold=2.0, reset_pass=False, variant=None, **kw):
    before, after = _one_agent(**kw)
    return SR.step_reference(before, after, 0, model, behaviour, reward, threshold, 1e-4, reset_pass, variant)


def test_reference_on_hand_worked_dynamics():
    """Classic, straight: speed 10, a = 2: the mean speed is 10.1, so x moves by 1.01 and the speed ends at 10.2.  Classic from
    rest with a = -2: the mean speed is -0.1 (1 cm backwards), the end speed -0.2 against the heading.  Classic turning: steer with
    tan = 1 on a 4 m car at 10 m/s: beta = atan(1/2), yaw rate 10 cos(beta) / 4.  Bicycle: a = 9 is clamped to 6, steer -4 to -3:
    x moves by 10 * 0.1 + 3 * 0.01, the yaw by -3 * (1 + 0.03).  DeltaLocal at yaw pi / 2: (1, 0) ahead is +y.  len_3: velocity
    (3, 0, 4) has speed 5."""
    r = _ref(vel=(10.0, 0.0, 0.0), action=(2.0,) + (0.0,) * 9)
    assert abs(r["x"][0] - 1.01) < 1e-12 and r["y"][0] == 0 and abs(r["vel"][0, 0] - 10.2) < 1e-12 and r["yaw"][0] == 0
    r = _ref(action=(-2.0,) + (0.0,) * 9)
    assert abs(r["x"][0] + 0.01) < 1e-12 and abs(r["vel"][0, 0] + 0.2) < 1e-12 and abs(r["self_obs"][0, 0] - 0.2) < 1e-12
    r = _ref(vel=(10.0, 0.0, 0.0), action=(0.0, math.atan(1.0)) + (0.0,) * 8)
    beta = math.atan(0.5)
    assert abs(r["yaw"][0] - 10 * math.cos(beta) / 4 * 0.1) < 1e-7 and abs(r["x"][0] - math.cos(beta)) < 1e-7 and abs(r["y"][0] - math.sin(beta)) < 1e-7
    r = _ref(model=SR.BICYCLE, vel=(10.0, 0.0, 0.0), action=(9.0, -4.0) + (0.0,) * 8)
    assert r["action"][0, :2].tolist() == [6.0, -3.0] and abs(r["x"][0] - 1.03) < 1e-7 and abs(r["yaw"][0] + 3.09) < 1e-6 and r["z"][0] == 1.0
    assert abs(np.hypot(*r["vel"][0, :2]) - 10.6) < 1e-7
    r = _ref(model=SR.DELTA, yaw=math.pi / 2, action=(1.0, 0.0, 0.25) + (0.0,) * 7)
    assert abs(r["x"][0]) < 1e-7 and abs(r["y"][0] - 1.0) < 1e-7 and abs(r["vel"][0, 1] - 10.0) < 1e-6 and abs(r["yaw"][0] - math.pi / 2 - 0.25) < 1e-7
    r = _ref(model=SR.BICYCLE, vel=(3.0, 0.0, 4.0))
    assert abs(r["speed0"][0] - 5.0) < 1e-12 and abs(r["x"][0] - 0.3) < 1e-7 and abs(np.hypot(*r["vel"][0, :2]) - 5.0) < 1e-7 and r["vel"][0, 2] == 0
    # a sum across the seam comes back on the other side; the variant that does not wrap leaves it outside
    r = _ref(model=SR.DELTA, yaw=3.0, action=(0.0, 0.0, 0.5) + (0.0,) * 7)
    assert abs(r["yaw"][0] - (3.5 - 2 * math.pi)) < 1e-6 and abs(r["yaw_sum"][0] - 3.5) < 1e-6
    assert abs(_ref(model=SR.DELTA, yaw=3.0, action=(0.0, 0.0, 0.5) + (0.0,) * 7, variant="no_wrap")["yaw"][0] - 3.5) < 1e-6
    assert SR.angular_distance(3.1, -3.1) < 0.09 and SR.angular_distance(0.1, 0.1 + 4 * math.pi) < 1e-12


def test_reference_on_hand_worked_reward_and_done():
    """An agent 1.5 m from its goal, threshold 2: reward 1 (or -1.5), done and info[3] after a step, steps 91 -> 90; the reset pass
    at steps 91 returns early: nothing is set.  At 2.5 m nothing is set until steps reach 0: then done, not info[3].  A done agent
    that has not reached its goal is still looked at (it collided under AgentStop, a parked car within its threshold); one that
    has, is not.  A done agent that is not Static goes to the padding position and its reward is taken from there."""
    near = dict(model=SR.STATE, pos=(98.5, 0.0, 1.0), action=(98.5, 0.0, 1.0) + (0.0,) * 7)
    r = _ref(reward=SR.ON_GOAL, **near)
    assert r["reward"][0] == 1 and r["done"][0] and r["reached"][0] and r["steps"][0] == 90 and abs(r["self_obs"][0, 4] - 1.5) < 1e-12
    assert _ref(**near)["reward"][0] == -1.5
    r = _ref(reward=SR.ON_GOAL, reset_pass=True, **near)
    assert r["reward"][0] == 1 and not r["done"][0] and not r["reached"][0] and r["steps"][0] == 91 and r["early"][0]
    r = _ref(reward=SR.ON_GOAL, reset_pass=True, steps=90, **near)
    assert r["done"][0] and r["reached"][0] and r["steps"][0] == 90
    far = dict(model=SR.STATE, pos=(97.5, 0.0, 1.0), action=(97.5, 0.0, 1.0) + (0.0,) * 7)
    r = _ref(steps=5, **far)
    assert not r["done"][0] and r["steps"][0] == 4
    r = _ref(steps=1, **far)
    assert r["done"][0] and not r["reached"][0] and r["steps"][0] == 0
    r = _ref(behaviour=CR.AGENT_STOP, collided=1, static=1, controlled=0, steps=60, pos=(99.0, 0.0, 1.0))
    assert r["done"][0] and r["reached"][0] and r["x"][0] == 99.0
    r = _ref(behaviour=CR.AGENT_STOP, collided=1, static=1, controlled=0, steps=60, pos=(99.0, 0.0, 1.0), variant="no_reach_when_done")
    assert r["done"][0] and not r["reached"][0]
    r = _ref(behaviour=CR.AGENT_STOP, collided=1, steps=60, vel=(3.0, 0.0, 0.0), **near)
    assert r["done"][0] and not r["reached"][0] and r["padded"][0] and r["x"][0] == -11000 and (r["vel"][0] == 0).all()
    assert abs(r["reward"][0] + math.hypot(11100.0, 11000.0)) < 1e-9
    assert not _ref(behaviour=CR.IGNORE, collided=1, steps=60, **far)["done"][0]
    # exactly on the threshold: outside; the margin does not take an agent whose offset lies along an axis
    on = dict(model=SR.STATE, pos=(98.0, 0.0, 1.0), action=(98.0, 0.0, 1.0) + (0.0,) * 7, reward=SR.ON_GOAL)
    assert not _ref(**on)["done"][0] and not _ref(**on)["margin"][0] and _ref(variant="le_threshold", **on)["done"][0]
    assert not _ref(threshold=0.0, model=SR.STATE, pos=(100.0, 0.0, 1.0), action=(100.0, 0.0, 1.0) + (0.0,) * 7)["done"][0]
    skew = dict(model=SR.STATE, pos=(98.6, 1.43, 1.0), action=(98.6, 1.43, 1.0) + (0.0,) * 7)
    assert _ref(**skew)["margin"][0] == (abs(math.hypot(100 - float(f32(98.6)), float(f32(1.43))) - 2.0) < 1e-4)


def test_reference_replays_the_log_at_the_current_step():
    traj = np.zeros((1, 1, 16 * 91), f32)
    k = np.arange(91)
    traj[0, 0, SR.TRAJ_POS:SR.TRAJ_POS + 182:2], traj[0, 0, SR.TRAJ_POS + 1:SR.TRAJ_POS + 182:2] = k, -k
    traj[0, 0, SR.TRAJ_VEL:SR.TRAJ_VEL + 182:2] = 10 + k
    traj[0, 0, SR.TRAJ_HEAD:SR.TRAJ_HEAD + 91] = 0.01 * k
    for steps, idx in ((91, 0), (90, 1), (1, 90)):
        r = _ref(controlled=0, steps=steps, traj=traj, pos=(5.0, 5.0, 3.0), vel=(1.0, 1.0, 1.0))
        assert (r["x"][0], r["y"][0], r["z"][0]) == (idx, -idx, 1.0) and r["vel"][0].tolist() == [10 + idx, 0, 0]
        assert abs(r["yaw"][0] - float(f32(0.01 * idx))) < 1e-12 and r["log_index"][0] == idx
    r = _ref(controlled=0, static=1, steps=50, traj=traj, pos=(5.0, 5.0, 3.0), vel=(1.0, 1.0, 1.0))
    assert (r["x"][0], r["y"][0], r["z"][0]) == (5.0, 5.0, 3.0) and r["vel"][0].tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(key):
    """The scripted run `key` = (case, model, behaviour, reward type) on the oracle, every pass measured against the reference.
    Returns dict(run, passes: [(tag, errors)], premise)."""
    from oracle import oracle as O
    O.build()
    name, model, behaviour, reward_type = key
    case = SC.CASES[name]
    orc = P.make_oracle_sim(O, case.write(tempfile.mkdtemp(prefix="step_cases_")), max_agents=case.slots, **case.params(model, behaviour, reward_type))
    run = SC.Run(case, [orc], model, behaviour, reward_type)
    passes, partners = [], [0, 0]

    def check(before, after, tag, reset):
        passes.append((tag, SC.errors(run, before[0], after[0], reset), reset))
        if name == "step_wrap" and not reset:    # opposite headings: the full quaternion product of the partner rows
            n_in, n_out = check_partner_rows_by_brute_force(orc, 50.0)
            partners[0], partners[1] = partners[0] + n_in, partners[1] + n_out

    SC.script(run, check)
    orc.close()
    assert name != "step_wrap" or (partners[0] > 0 and partners[1] > 0), partners
    return dict(run=run, passes=passes, premise=case.premise(run))


def _tag(key):
    return "%s (model %d, behaviour %d, reward type %d)" % key


@pytest.mark.parametrize("key", ALL_RUNS, ids=["%s-m%d-b%d-r%d" % k for k in ALL_RUNS])
def test_oracle_meets_the_reference_on_constructed_worlds(oracle_mod, key):
    got = _oracle_run(key)
    agents = marginal = 0
    worst = {}
    for tag, e, _ in got["passes"]:
        assert not e["bad"], "%s, %s: %s [%d of %d agents are marginal]" % (_tag(key), tag, "; ".join(e["bad"]), e["marginal"], e["agents"])
        for k, v in SC.ratios(e["err"]).items():
            assert v <= 1.0, "%s, %s: %s at +-%g m: %.3g is beyond ORACLE_STEP_MAX" % (_tag(key), tag, k[1], k[0], e["err"][k])
            worst[k] = max(worst.get(k, 0.0), e["err"][k])
        agents, marginal = max(agents, e["agents"]), max(marginal, e["marginal"])
    print("STEP %s: %d passes, agents %d, marginal %d; %s; premise: %s" % (
        _tag(key), len(got["passes"]), agents, marginal, ", ".join("%s@%g %.3g" % (c, s, v) for (s, c), v in sorted(worst.items())), got["premise"]))
    assert marginal <= SC.MARGIN_AGENTS * agents, "%s: %d of %d agents are marginal: move the geometry" % (_tag(key), marginal, agents)


def test_the_recorded_constants_are_what_the_oracle_measures(oracle_mod):
    """ORACLE_STEP_MAX[span][column] holds the oracle's largest distance from the reference over every pass of every run, and is
    not more than twice it: a constant that has gone stale in either direction fails here."""
    worst, where = {}, {}
    for key in ALL_RUNS:
        for tag, e, _ in _oracle_run(key)["passes"]:
            for k, v in e["err"].items():
                if v > worst.get(k, -1.0):
                    worst[k], where[k] = v, "%s, %s" % (_tag(key), tag)
    for span, cols in SC.ORACLE_STEP_MAX.items():
        for col, bound in cols.items():
            assert (span, col) in worst, "no run measures %s at +-%g m" % (col, span)
            print("STEP measured %-6s at +-%-6g m: %.3e (recorded %.3e) in %s" % (col, span, worst[(span, col)], bound, where[(span, col)]))
    for span, cols in SC.ORACLE_STEP_MAX.items():
        for col, bound in cols.items():
            v = worst[(span, col)]
            assert v <= bound, "the oracle is %.3g from the reference in %s at +-%g m: ORACLE_STEP_MAX is stale (%s)" % (v, col, span, where[(span, col)])
            assert bound <= 2 * v, "ORACLE_STEP_MAX[%g][%s] = %.3g is more than twice what is measured (%.3g)" % (span, col, bound, v)
    assert set(worst) == {(s, c) for s, cols in SC.ORACLE_STEP_MAX.items() for c in cols}, sorted(worst)


def test_every_case_stays_within_its_span(oracle_mod):
    for key in ALL_RUNS:
        run = _oracle_run(key)["run"]
        for before, after, _ in run.history:
            for w, wd in enumerate(run.case.worlds):
                st, goal = after[0]["state"][w, :wd.n], after[0]["abs_obs"][w, :wd.n, 8:10]
                here = st[:, 2] != CR.PAD_Z
                assert np.abs(st[here, 0:2]).max() <= wd.span and np.abs(goal).max() <= wd.span, (_tag(key), w)


# ------------------------------------------------------------------------------------------------------------------
# sensitivity: every wrong rule is caught by the case that aims at it
# ------------------------------------------------------------------------------------------------------------------
CAUGHT_BY = {
    "mean_is_end_speed": ("step_speed", SR.CLASSIC, CR.IGNORE, SR.ON_GOAL),
    "beta_without_half": ("step_steer", SR.CLASSIC, CR.IGNORE, SR.ON_GOAL),
    "no_wrap": ("step_wrap", SR.CLASSIC, CR.IGNORE, SR.ON_GOAL),
    "width_for_length": ("step_steer", SR.CLASSIC, CR.IGNORE, SR.ON_GOAL),
    "no_clamp": ("step_steer", SR.BICYCLE, CR.IGNORE, SR.ON_GOAL),
    "delta_minus_yaw": ("step_wrap", SR.DELTA, CR.IGNORE, SR.ON_GOAL),
    "log_off_by_one": ("step_replay", SR.CLASSIC, CR.IGNORE, SR.DISTANCE_BASED),
    "le_threshold": ("step_goal", SR.STATE, CR.IGNORE, SR.ON_GOAL),
    "reward_sign": ("step_goal", SR.STATE, CR.IGNORE, SR.DISTANCE_BASED),
    "decrement_after_done": ("step_goal", SR.STATE, CR.IGNORE, SR.ON_GOAL),
    "no_reach_when_done": ("step_done", SR.STATE, CR.AGENT_STOP, SR.ON_GOAL),
    "static_padded": ("step_goal", SR.STATE, CR.IGNORE, SR.ON_GOAL),
}
INTEGER_RULES = ("le_threshold", "decrement_after_done", "no_reach_when_done", "static_padded")


@pytest.mark.parametrize("variant", SR.VARIANTS)
def test_every_wrong_rule_is_caught_by_its_case(oracle_mod, variant):
    """The variant reference against the oracle's own outputs: beyond ORACLE_STEP_MAX in a float column, or -- for the rules
    that decide integers -- an exact output that differs on a non-marginal agent (errors() lists no others).  A heading that
    is not wrapped is the same rotation: it shows only where the heading is exported as a number, the absolute row's angle,
    which is compared as a number here on the agents away from the seam."""
    assert set(CAUGHT_BY) == set(SR.VARIANTS)
    key = CAUGHT_BY[variant]
    got = _oracle_run(key)
    run = got["run"]
    caught = []
    for (before, after, reset), (tag, _, _) in zip(run.history, got["passes"]):
        e = SC.errors(run, before[0], after[0], reset, variant=variant, raw_yaw=variant == "no_wrap")
        over = [k for k, v in SC.ratios(e["err"]).items() if v > 1.0]
        if variant in INTEGER_RULES:
            if e["bad"]:
                caught.append("%s: %s" % (tag, e["bad"][0]))
        elif over or e["bad"]:
            caught.append("%s: %s" % (tag, over or e["bad"][0]))
    print("STEP variant %s on %s: %s" % (variant, _tag(key), caught[:2]))
    assert caught, "the wrong rule '%s' passes on %s: the case does not aim at it" % (variant, _tag(key))


def test_the_comparison_raises_on_a_moved_position_and_a_flipped_done(oracle_mod):
    key = ("step_wrap", SR.CLASSIC, CR.IGNORE, SR.ON_GOAL)
    run = _oracle_run(key)["run"]
    before, after, reset = run.history[1]
    SC.hold(run, before[0], after[0], "untouched", 1.0, reset)
    moved = {k: v.copy() for k, v in after[0].items()}
    moved["state"][0, 5, 0] += f32(4 * SC.ORACLE_STEP_MAX[150.0]["pos"])
    moved["abs_obs"][0, 5, 0] = moved["state"][0, 5, 0]
    with pytest.raises(AssertionError, match="pos at"):
        SC.hold(run, before[0], moved, "moved", 1.0, reset)
    flipped = {k: v.copy() for k, v in after[0].items()}
    flipped["done"][0, 7] ^= 1
    with pytest.raises(AssertionError, match="done differs"):
        SC.hold(run, before[0], flipped, "flipped", 1.0, reset)
