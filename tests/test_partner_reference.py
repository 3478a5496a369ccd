"""CPU suite: the float64 partner-row reference (tests/partner_reference.py) against hand-worked answers, the oracle against the
reference on the constructed, moving worlds of tests/partner_cases.py after the reset pass and after every step, the cases'
premises and margin condition (on the reference alone), the measured constants (ORACLE_PARTNER_MAX: the oracle stays within
each, and none is more than twice what is measured), the packed head's float64 statement, and the sensitivity of the cases: every
wrong-rule variant of the reference disagrees with the oracle on the case that aims at its rule."""
import functools
import math
import tempfile

import numpy as np
import pytest

from tests import parity as P
from tests import partner_cases as PC
from tests import partner_reference as PR

f32 = np.float32
f64 = np.float64
NAMES = [c.name for c in PC.CASE_LIST]


# ------------------------------------------------------------------------------------------------------------------
# the reference itself, against answers worked out by hand
# ------------------------------------------------------------------------------------------------------------------
def _inp(agents, slots=4):
    """agents: (x, y, yaw, speed, length, type, id) per live agent, in a world of slots + 1 agent slots."""
    n = len(agents)
    ab = np.zeros((1, slots + 1, 14), f32)
    so = np.zeros((1, slots + 1, 8), f32)
    et = np.zeros((1, slots + 1), np.int32)
    for a, (x, y, yaw, speed, length, kind, rid) in enumerate(agents):
        ab[0, a, 0:2] = (x, y)
        ab[0, a, 3:7] = (math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2))
        ab[0, a, 10:13] = (length, 2.0, 1.5)
        ab[0, a, 13] = rid
        so[0, a, 0] = speed
        et[0, a] = kind
    return dict(shape=np.asarray([[n, 1]], np.int32), abs_obs=ab, self_obs=so, etype=et, rows=np.zeros((1, slots + 1, slots, 9), f32))


def test_three_agents_by_hand():
    """Ego 1 at (3, 0) turned by 90 degrees: agent 0 at (3, 3) lies 3 m ahead (x = 3, y = 0), agent 2 at (-47, 0) lies 50 m to its
    right, exactly on the radius (inside, and an exact verdict only for an ego that is not turned)."""
    inp = _inp([(3.0, 3.0, math.radians(270), 7.0, 4.0, 7, 11), (3.0, 0.0, math.radians(90), 1.0, 5.0, 8, 12), (-47.0, 0.0, 0.0, 2.0, 6.0, 9, 13)])
    ref = PR.partner_reference(inp, 0, 50.0, 1e-5)
    assert ref["J"].tolist() == [[1, 2], [0, 2], [0, 1]]
    r = ref["rows"][1]
    assert abs(r[0, PR.X] - 3.0) < 1e-6 and abs(r[0, PR.Y]) < 1e-6 and abs(abs(r[0, PR.HEADING]) - math.pi) < 1e-6
    assert r[0, [PR.SPEED, PR.LENGTH, PR.WIDTH, PR.HEIGHT, PR.TYPE, PR.ID]].tolist() == [7.0, 4.0, 2.0, 1.5, 7.0, 11.0]
    assert abs(r[1, PR.X]) < 1e-5 and abs(r[1, PR.Y] - 50.0) < 1e-5 and abs(r[1, PR.HEADING] + math.pi / 2) < 1e-6 and r[1, PR.ID] == 13.0
    assert ref["near"][1, 1] and not ref["exact"][1, 1], "a turned ego's partner at the radius is marginal"
    assert ref["exact"][2, 1] and not ref["near"][2, 1] and ref["inside"][2, 1], "agent 2 (yaw 0) sees agent 1 exactly on the radius: inside"
    assert (ref["rows"][:, 2:] == PR.ZERO_NONEXIST).all()
    # 0 -> 2 is 50.09 m: the zero row
    assert not ref["inside"][0, 1] and ref["rows"][0, 1].tolist() == PR.ZERO.tolist()
    lt = PR.partner_reference(inp, 0, 50.0, 1e-5, "ge_radius")
    assert lt["rows"][2, 1].tolist() == PR.ZERO.tolist()
    assert PR.partner_reference(inp, 0, 50.0, 1e-5, "no_ego_skip")["rows"][1, 0, PR.ID] == 11.0 and PR.partner_reference(inp, 0, 50.0, 1e-5, "no_ego_skip")["rows"][1, 1, PR.ID] == 12.0
    assert abs(PR.partner_reference(inp, 0, 50.0, 1e-5, "rotate_plus_yaw")["rows"][1, 0, PR.X] + 3.0) < 1e-6
    assert abs(PR.partner_reference(inp, 0, 50.0, 1e-5, "heading_reversed")["rows"][1, 1, PR.HEADING] - math.pi / 2) < 1e-6
    assert PR.partner_reference(inp, 0, 50.0, 1e-5, "relative_speed")["rows"][1, 0, PR.SPEED] == 6.0
    assert PR.partner_reference(inp, 0, 50.0, 1e-5, "ego_size")["rows"][1, 0, PR.LENGTH] == 5.0
    assert (PR.partner_reference(inp, 0, 50.0, 1e-5, "ids_swapped")["rows"][:, 2:, PR.ID] == -1).all()


def test_one_agent_alone_and_two_on_one_point():
    alone = PR.partner_reference(_inp([(1.0, 2.0, 0.3, 0.0, 4.0, 7, 5)]), 0, 50.0, 1e-5)
    assert alone["J"].shape == (1, 0) and (alone["rows"] == PR.ZERO_NONEXIST).all()
    two = PR.partner_reference(_inp([(-11000.0, -11000.0, 0.4, 0.0, 4.0, 7, 5), (-11000.0, -11000.0, -2.0, 0.0, 4.0, 7, 6)]), 0, 0.0, 1e-5)
    assert two["inside"].all() and two["exact"].all() and not two["near"].any() and (two["dist"] == 0).all()
    assert abs(two["rows"][0, 0, PR.HEADING] + 2.4) < 1e-6 and two["rows"][1, 0, PR.ID] == 5.0
    assert not PR.partner_reference(_inp([(0.0, 0.0, 0.4, 0.0, 4.0, 7, 5), (1e-3, 0.0, 0.0, 0.0, 4.0, 7, 6)]), 0, 0.0, 1e-5)["inside"].any()


def test_the_heading_wraps_and_the_host_count_of_equal_headings():
    inp = _inp([(0.0, 0.0, 3.0, 0.0, 4.0, 7, 1), (1.0, 0.0, -3.0, 0.0, 4.0, 7, 2), (2.0, 0.0, 3.0, 0.0, 4.0, 7, 3)])
    ref = PR.partner_reference(inp, 0, 50.0, 1e-5)
    assert abs(ref["rows"][0, 0, PR.HEADING] - (2 * math.pi - 6.0)) < 1e-6 and abs(ref["rows"][0, 1, PR.HEADING]) < 1e-12
    assert abs(PR.partner_reference(inp, 0, 50.0, 1e-5, "no_heading_wrap")["rows"][0, 0, PR.HEADING] + 6.0) < 1e-6
    zero, opposite = PR.same_heading_pairs(inp["abs_obs"][0, :3, 3:7])
    assert zero[0, 2] and zero[2, 0] and not zero[0, 1] and not opposite.any()


def test_the_packed_head_is_the_head_of_the_packed_observation():
    rng = np.random.default_rng(3)
    so, rows, road = rng.normal(size=(5, 8)), rng.normal(size=(5, 63, 9)), rng.normal(size=(5, 200, 9))
    full = P.pack_observation_f64(so, rows, road)
    assert np.array_equal(PR.packed_head(so, rows), full[:, :PR.head_width(63)]) and PR.head_width(63) == 384
    assert np.array_equal(PR.head_gain(63), P.pack_column_gain(64)[:384])


# ------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """The scripted run of case `name` on the oracle, every pass measured against the reference.  Returns dict(run, passes:
    [(tag, errors)], premise)."""
    from oracle import oracle as O
    O.build()
    case = PC.CASES[name]
    paths = PC.write_scenes(case, tempfile.mkdtemp(prefix="partner_cases_"))
    orc = P.make_oracle_sim(O, paths[:len(case.worlds)], max_agents=case.slots, **case.params(PC.ALGO))
    run = PC.Run(case, [orc])
    run.scene_paths = paths
    passes = []
    PC.script(run, lambda p: passes.append((run.passes[p]["tag"], PC.errors(run, p, 1.0))))
    orc.close()
    return dict(run=run, passes=passes, premise=case.premise(run))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_meets_the_reference_on_constructed_worlds(oracle_mod, name):
    got = _oracle_run(name)
    run = got["run"]
    worst, pairs, marginal, designed, exact = {}, 0, 0, 0, 0
    for tag, e in got["passes"]:
        assert not e["bad"], "%s, %s: %s [%d of %d pairs marginal]" % (name, tag, "; ".join(e["bad"][:4]), e["marginal"], e["pairs"])
        for k, v in PC.ratios(e["err"]).items():
            assert v <= 1.0, "%s, %s: %s at +-%g m: %.3g is beyond ORACLE_PARTNER_MAX" % (name, tag, k[1], k[0], e["err"][k])
            worst[k] = max(worst.get(k, 0.0), e["err"][k])
    # the margin condition, on the reference alone and at the GPU suite's (wider) margins
    for p in range(len(run.passes)):
        e = PC.errors(run, p, PC.GPU_FACTOR)
        assert e["marginal"] <= PC.MARGIN_AGENTS * e["pairs"], "%s, %s: %d of %d pairs are marginal: move the geometry" % (name, run.passes[p]["tag"], e["marginal"], e["pairs"])
        pairs, marginal, designed, exact = max(pairs, e["pairs"]), max(marginal, e["marginal"]), max(designed, e["designed"]), max(exact, e["exact"])
    print("PARTNER %s: %d passes, pairs %d, marginal %d (cap %d), marginal by design %d, exact verdicts at the radius %d; %s; premise: %s" % (
        name, len(got["passes"]), pairs, marginal, int(PC.MARGIN_AGENTS * pairs), designed, exact,
        ", ".join("%s@%g %.3g" % (c, s, v) for (s, c), v in sorted(worst.items())), got["premise"]))
    assert designed == (16 if name == "partner_radius" else 0)


def test_the_recorded_constants_are_what_the_oracle_measures(oracle_mod):
    """ORACLE_PARTNER_MAX[span][column] holds the oracle's largest distance from the reference over every in-radius pair on
    every pass of every run, and is not more than twice it: a constant that has gone stale in either direction fails here."""
    worst = {}
    for name in NAMES:
        for tag, e in _oracle_run(name)["passes"]:
            for k, v in e["err"].items():
                if v > worst.get(k, (-1.0, ""))[0]:
                    worst[k] = (v, "%s, %s" % (name, tag))
    for span, cols in PC.ORACLE_PARTNER_MAX.items():
        for col, bound in cols.items():
            assert (span, col) in worst, "no run measures %s at +-%g m" % (col, span)
            print("PARTNER measured %-7s at +-%-6g m: %.3e (recorded %.3e) in %s" % (col, span, worst[(span, col)][0], bound, worst[(span, col)][1]))
    for span, cols in PC.ORACLE_PARTNER_MAX.items():
        for col, bound in cols.items():
            v, where = worst[(span, col)]
            assert v <= bound, "the oracle is %.3g from the reference in %s at +-%g m: ORACLE_PARTNER_MAX is stale (%s)" % (v, col, span, where)
            assert bound <= 2 * v, "ORACLE_PARTNER_MAX[%g][%s] = %.3g is more than twice what is measured (%.3g)" % (span, col, bound, v)


def test_every_case_stays_within_its_span(oracle_mod):
    for name in NAMES:
        run = _oracle_run(name)["run"]
        for p, ps in enumerate(run.passes):
            for w in range(len(run.case.worlds)):
                st = ps["state"][w, :run.live(p, w)]
                here = st[:, 0] > -10000
                assert np.abs(st[here, 0:2]).max() <= run.spans[w], (name, p, w)


def test_the_oracles_packed_head_meets_the_reference(oracle_mod):
    """The float64 packing of the oracle's own rows against the float64 packing of the reference rows, within the raw bounds
    carried through each column's gain: what the GPU suite asks of the kernels' packed heads, on the CPU."""
    for name in PC.PACKED:
        run = _oracle_run(name)["run"]
        for p in range(len(run.passes)):
            snap = run.passes[p]["snaps"][0]
            slots = [(w, a) for w in range(len(run.case.worlds)) for a in range(run.live(p, w))]
            heads = [PR.packed_head(snap["self_obs"][w, a], snap["rows"][w, a]) for w, a in slots]
            worst, bad = PC.head_errors(run, p, heads, slots, 1.0, 0)
            assert not bad, "%s, %s: %s" % (name, run.passes[p]["tag"], bad[:3])


# ------------------------------------------------------------------------------------------------------------------
# sensitivity: every wrong rule is caught by the case that aims at it
# ------------------------------------------------------------------------------------------------------------------
CAUGHT_BY = {
    "ge_radius": "partner_radius",
    "no_ego_skip": "partner_counts",
    "rotate_plus_yaw": "partner_far",
    "heading_reversed": "partner_headings",
    "no_heading_wrap": "partner_headings",
    "relative_speed": "partner_columns",
    "ego_size": "partner_columns",
    "ids_swapped": "partner_rebuild",
    "radius_on_unskipped_pair": "partner_moves",
}


@pytest.mark.parametrize("variant", PR.VARIANTS)
def test_every_wrong_rule_is_caught_by_its_case(oracle_mod, variant):
    """The variant reference against the oracle's own rows: a verdict outside the margin mask, a wrong zero row, an exact column
    that differs, or a float column beyond ORACLE_PARTNER_MAX.  A heading that is not wrapped is compared as a number."""
    assert set(CAUGHT_BY) == set(PR.VARIANTS)
    name = CAUGHT_BY[variant]
    run = _oracle_run(name)["run"]
    caught = []
    for p, ps in enumerate(run.passes):
        assert not PC.errors(run, p, 1.0)["bad"], "the true rule must pass where the variant is tried"
        e = PC.errors(run, p, 1.0, variant=variant)
        over = [k for k, v in PC.ratios(e["err"]).items() if v > 1.0]
        if e["bad"] or over:
            caught.append("%s: %s" % (ps["tag"], e["bad"][0] if e["bad"] else over))
    print("PARTNER variant %s on %s: %s" % (variant, name, caught[:2]))
    assert caught, "the wrong rule '%s' passes on %s: the case does not aim at it" % (variant, name)


def test_the_comparison_raises_on_a_moved_row_a_stale_row_and_a_wrong_zero_row(oracle_mod):
    run = _oracle_run("partner_counts")["run"]
    PC.hold(run, 1, 1.0)
    rows = run.passes[1]["snaps"][0]["rows"]
    keep = rows.copy()
    ref = run.ref(1, 4)      # the world of 16
    i, k = np.argwhere(ref["inside"])[0]
    try:
        rows[4, i, k, PR.X] += f32(4 * PC.ORACLE_PARTNER_MAX[150.0]["x"])
        with pytest.raises(AssertionError, match="x at"):
            PC.hold(run, 1, 1.0)
        rows[...] = keep
        rows[4, i, k] = run.passes[0]["snaps"][0]["rows"][4, (i + 1) % 16, k]      # another ego's row of the pass before
        with pytest.raises(AssertionError):
            PC.hold(run, 1, 1.0)
        rows[...] = keep
        rows[4, 3, 15, PR.ID] = -1
        with pytest.raises(AssertionError, match="slot 15"):
            PC.hold(run, 1, 1.0)
        rows[...] = keep
        rows[4, i, k] = PR.ZERO
        with pytest.raises(AssertionError, match="the zero row"):
            PC.hold(run, 1, 1.0)
    finally:
        rows[...] = keep
