"""CPU suite: the float64 road-row reference (tests/road_reference.py) against hand-worked answers, the oracle against the
reference on the constructed, moving worlds of tests/road_cases.py after the reset pass and after every step in every mode, the
cases' premises and margin condition (on the reference alone), the measured constants (ORACLE_ROAD_MAX: the oracle stays within
each, and none is more than twice what is measured), and the sensitivity of the cases: every wrong-rule variant of the
reference disagrees with the oracle on the case that aims at its rule."""
import functools
import math
import tempfile

import numpy as np
import pytest

from tests import heap_pin as HP
from tests import parity as P
from tests import road_cases as RC
from tests import road_reference as RR

f32 = np.float32
CPU_RUNS = sorted({(c.name, RC.CPU_MODES[RC.MODES[m][0]]) for c in RC.CASE_LIST for m in c.modes})     # (case, roadObservationAlgorithm)


def _ref_modes(name, algo):
    return sorted({RC.MODES[m][0] for m in RC.CASES[name].modes if RC.CPU_MODES[RC.MODES[m][0]] == algo})


# ------------------------------------------------------------------------------------------------------------------
# the reference itself, against answers worked out by hand
# ------------------------------------------------------------------------------------------------------------------
def _inp(roads, x=0.0, y=0.0, yaw=0.0):
    roads = np.asarray(roads, f32).reshape(-1, 9)
    ab = np.zeros((1, 1, 14), f32)
    ab[0, 0, 0:2] = (x, y)
    ab[0, 0, 3:7] = (math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2))
    return dict(shape=np.asarray([[1, len(roads)]], np.int32), abs_obs=ab, map_obs=roads[None])


def _row(x, y, heading=0.0, rid=1.0, kind=1.0):
    return [x, y, 2.0, 0.1, 0.1, heading, kind, rid, 15.0]


def test_observation_of_on_the_references_own_example():
    """tests/EgocentricRoadObservationTests.cpp:9-22: the frame at (3, 0) turned by 90 degrees sees the road at (3, 3), turned by
    270 degrees, at (3, 0) with the heading 180 degrees; scale, type, id and mapType are copied."""
    o = RR.observation_of(np.asarray([_row(3.0, 3.0, math.radians(270), rid=7.0, kind=3.0)]), 3.0, 0.0, math.radians(90))[0]
    assert abs(o[0] - 3.0) < 1e-12 and abs(o[1]) < 1e-12 and abs(abs(o[5]) - math.pi) < 1e-12
    assert o[2:5].tolist() == [2.0, 0.1, 0.1] and o[6:9].tolist() == [3.0, 7.0, 15.0]
    plus = RR.observation_of(np.asarray([_row(3.0, 3.0)]), 3.0, 0.0, math.radians(90), variant="rotate_plus_yaw")[0]
    assert abs(plus[0] + 3.0) < 1e-12
    assert abs(RR.observation_of(np.asarray([_row(0.0, 1.0, -3.0)]), 0.0, 0.0, 3.0, variant="no_heading_wrap")[0, 5] + 6.0) < 1e-12
    assert abs(RR.observation_of(np.asarray([_row(0.0, 1.0, -3.0)]), 0.0, 0.0, 3.0)[0, 5] - (2 * math.pi - 6.0)) < 1e-12


def test_radius_filter_swaps_from_the_end():
    """src/knn.hpp:83-97 on [far, a, b, far, c]: the first far row is replaced by c, the second by b's successor ... -> [c, a, b]."""
    dist = np.asarray([60.0, 1.0, 2.0, 70.0, 3.0, 50.0])
    assert RR.radius_filter([0, 1, 2, 3, 4], dist, 50.0) == [4, 1, 2]
    assert RR.radius_filter([0, 1, 2, 3, 4], dist, 50.0, "stable_compaction") == [1, 2, 4]
    assert RR.radius_filter([5, 0], dist, 50.0) == [5] and RR.radius_filter([5, 0], dist, 50.0, "lt_radius") == []


def test_fewer_than_k_roads_and_both_padding_conventions():
    roads = [_row(10.0, 0.0, rid=1.0), _row(80.0, 0.0, rid=2.0), _row(0.0, 50.0, rid=3.0), _row(0.0, -20.0, rid=4.0)]
    knn = RR.road_reference(_inp(roads), 0, 0, 50.0, RR.KNN, 1e-7, 1e-5)
    assert knn["order"][:4].tolist() == [0, 3, 2, -1] and (knn["rows"][3:] == 0).all() and knn["rows"][1, 7] == 4.0
    lin = RR.road_reference(_inp(roads), 0, 0, 50.0, RR.LINEAR, 1e-7, 1e-5)
    assert lin["order"][:4].tolist() == [0, 2, 3, -1] and lin["rows"][3].tolist() == [0, 0, 0, 0, 0, 0, 0, -1, -1]
    # the road exactly on the radius, straight ahead of an agent at yaw 0: an exact verdict, inside; the margin takes the
    # same road once the agent is turned
    assert 2 in knn["required"] and not knn["marginal"] and knn["exact"][2]
    turned = RR.road_reference(_inp(roads, yaw=0.3), 0, 0, 50.0, RR.KNN, 1e-7, 1e-5)
    assert 2 in turned["optional"] and turned["marginal"]


def test_the_heap_run_in_float64_reports_the_smallest_gap_it_compared():
    """K = 3 over keys 9, 1, 4, then 2.25 (an insert) and 16 (not one): the array libstdc++ leaves, and the smallest gap among
    the comparisons made; equal keys do not count.  The float32 protocol gives the same order."""
    keys = [9.0, 1.0, 4.0, 2.25, 16.0]
    order, gap = HP.libstdcxx_order_f64(keys, np.inf, 3)
    assert sorted(order.tolist()) == [1, 2, 3] and order[0] == 2
    assert order.tolist() == HP.libstdcxx_order(keys, 1e9, 3).tolist()
    assert abs(gap - (4.0 - 2.25) / 5.0) < 1e-15, gap           # 2.25 against 4 while it sifts
    order, gap = HP.libstdcxx_order_f64([5.0, 5.0, 5.0, 5.0], np.inf, 3)
    assert order.tolist() == HP.libstdcxx_order([5.0] * 4, 1e9, 3).tolist() and sorted(order.tolist()) == [0, 1, 2] and gap == np.inf
    order, gap = HP.libstdcxx_order_f64([1.0, 100.0], 5.0, 3)
    assert order.tolist() == [0, -1, -1] and gap == np.inf      # fewer than K roads: no comparison at all


def test_set_order_ties_go_to_the_lowest_index_and_linear_stops_at_k():
    roads = [_row(1.0 + (i % 5), 0.0, rid=float(i)) for i in range(12)]
    ref = RR.road_reference(_inp(roads), 0, 0, 50.0, RR.SET, 1e-7, 1e-5, k=4)
    assert sorted(ref["required"]) == [0, 1, 5, 10] and not ref["marginal"]
    high = RR.road_reference(_inp(roads), 0, 0, 50.0, RR.SET, 1e-7, 1e-5, variant="ties_to_highest", k=4)
    assert sorted(high["order"][high["order"] >= 0].tolist()) == [0, 5, 10, 11]
    lin = RR.road_reference(_inp(roads), 0, 0, 50.0, RR.LINEAR, 1e-7, 1e-5, k=4)
    assert lin["order"].tolist() == [0, 1, 2, 3]
    assert RR.road_reference(_inp(roads), 0, 0, 50.0, RR.LINEAR, 1e-7, 1e-5, variant="linear_no_stop", k=4)["order"].tolist() == [8, 9, 10, 11]
    assert RR.road_reference(_inp(roads), 0, 0, 50.0, RR.LINEAR, 1e-7, 1e-5, variant="linear_k_nearest", k=4)["order"].tolist() == [0, 1, 5, 10]


# ------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(key):
    """The scripted run `key` = (case, roadObservationAlgorithm) on the oracle, every pass measured against the reference in
    every reference mode that algorithm answers.  Returns dict(run, passes: [(tag, {mode: errors})], measured, premise)."""
    from oracle import oracle as O
    O.build()
    name, algo = key
    case = RC.CASES[name]
    paths = RC.write_scenes(case, tempfile.mkdtemp(prefix="road_cases_"))
    orc = P.make_oracle_sim(O, paths[:len(case.worlds)], max_agents=case.slots, **case.params(algo))
    modes = _ref_modes(name, algo)
    run = RC.Run(case, [orc], next(m for m in case.modes if RC.MODES[m][0] == modes[0]))
    run.scene_paths = paths
    passes, measured = [], {}

    def check(p):
        passes.append((run.passes[p]["tag"], {mode: RC.errors(run, p, 1.0, mode=mode, heap_rows=True) for mode in modes}))
        for k, v in RC.measure_oracle(run, orc, p).items():
            if v > measured.get(k, (-1.0, ""))[0]:
                measured[k] = (v, "%s, %s" % (name, run.passes[p]["tag"]))

    RC.script(run, check)
    orc.close()
    return dict(run=run, passes=passes, measured=measured, premise=case.premise(run), modes=modes)


@pytest.mark.parametrize("key", CPU_RUNS, ids=["%s-algo%d" % k for k in CPU_RUNS])
def test_oracle_meets_the_reference_on_constructed_worlds(oracle_mod, key):
    got = _oracle_run(key)
    run = got["run"]
    for mode in got["modes"]:
        worst, agents, marginal, undecided = {}, 0, 0, 0
        for tag, by_mode in got["passes"]:
            e = by_mode[mode]
            assert not e["bad"], "%s (%s), %s: %s [%d of %d agents marginal, %d undecided]" % (key[0], mode, tag, "; ".join(e["bad"][:4]), e["marginal"], e["agents"], e["undecided"])
            for k, v in RC.ratios(e["err"]).items():
                assert v <= 1.0, "%s (%s), %s: %s at +-%g m: %.3g is beyond ORACLE_ROAD_MAX" % (key[0], mode, tag, k[1], k[0], e["err"][k])
                worst[k] = max(worst.get(k, 0.0), e["err"][k])
            agents = max(agents, e["agents"])
        # the margin condition, on the reference alone and at the GPU suite's (wider) margins
        for p in range(len(run.passes)):
            refs = [run.ref(p, w, a, mode, RC.GPU_FACTOR) for w, a in run.agents()]
            marginal = max(marginal, sum(r["marginal"] for r in refs))
            undecided = max(undecided, sum(not r["decided"] and not r["marginal"] for r in refs))
        print("ROAD %s (%s): %d passes, agents %d, marginal %d, undecided %d; %s; premise: %s" % (
            key[0], mode, len(got["passes"]), agents, marginal, undecided, ", ".join("%s@%g %.3g" % (c, s, v) for (s, c), v in sorted(worst.items())), got["premise"]))
        assert marginal + undecided <= RC.MARGIN_AGENTS * agents, "%s (%s): %d of %d agents are marginal, %d undecided: move the geometry" % (
            key[0], mode, marginal, agents, undecided)


def test_the_recorded_constants_are_what_the_oracle_measures(oracle_mod):
    """ORACLE_ROAD_MAX[span][column] holds the oracle's largest distance from the reference over every road of every agent on
    every pass of every run, and is not more than twice it: a constant that has gone stale in either direction fails here."""
    worst = {}
    for key in CPU_RUNS:
        for k, (v, where) in _oracle_run(key)["measured"].items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, where)
    for span, cols in RC.ORACLE_ROAD_MAX.items():
        for col, bound in cols.items():
            assert (span, col) in worst, "no run measures %s at +-%g m" % (col, span)
            print("ROAD measured %-7s at +-%-6g m: %.3e (recorded %.3e) in %s" % (col, span, worst[(span, col)][0], bound, worst[(span, col)][1]))
    for span, cols in RC.ORACLE_ROAD_MAX.items():
        for col, bound in cols.items():
            v, where = worst[(span, col)]
            assert v <= bound, "the oracle is %.3g from the reference in %s at +-%g m: ORACLE_ROAD_MAX is stale (%s)" % (v, col, span, where)
            assert bound <= 2 * v, "ORACLE_ROAD_MAX[%g][%s] = %.3g is more than twice what is measured (%.3g)" % (span, col, bound, v)


def test_every_case_stays_within_its_span(oracle_mod):
    for key in CPU_RUNS:
        run = _oracle_run(key)["run"]
        for ps in run.passes:
            for w, wd in enumerate(run.case.worlds):
                st = ps["state"][w, :wd.n]
                here = st[:, 0] > -10000
                R = int(ps["snaps"][0]["shape"][w, 1])
                near = np.abs(ps["snaps"][0]["map_obs"][w, :R, 0:2]).max(-1) < 2500       # (the outliers kilometres away are out of every reach)
                assert np.abs(st[here, 0:2]).max() <= wd.span and np.abs(ps["snaps"][0]["map_obs"][w, :R, 0:2][near]).max() <= wd.span, (key, w)


# ------------------------------------------------------------------------------------------------------------------
# sensitivity: every wrong rule is caught by the case that aims at it
# ------------------------------------------------------------------------------------------------------------------
CAUGHT_BY = {
    "lt_radius": ("road_radius", RR.KNN),
    "filter_before_k": ("road_counts", RR.KNN),
    "stable_compaction": ("road_counts", RR.KNN),
    "zero_padding_knn": ("road_counts", RR.KNN),
    "no_heading_wrap": ("road_rows", RR.KNN),
    "rotate_plus_yaw": ("road_rows", RR.KNN),
    "ties_to_highest": ("road_ties", RR.SET),
    "linear_no_stop": ("road_blocks", RR.LINEAR),
    "linear_k_nearest": ("road_blocks", RR.LINEAR),
}


@pytest.mark.parametrize("variant", RR.VARIANTS)
def test_every_wrong_rule_is_caught_by_its_case(oracle_mod, variant):
    """The variant reference against the oracle's own rows: a row that is no selected road's, a missing road, a wrong padding
    row, an exact column that differs, or a float column beyond ORACLE_ROAD_MAX.  A heading that is not wrapped is compared as
    a number."""
    assert set(CAUGHT_BY) == set(RR.VARIANTS)
    name, mode = CAUGHT_BY[variant]
    got = _oracle_run((name, RC.CPU_MODES[mode]))
    run = got["run"]
    caught = []
    # (set order against the oracle's heap: the agents at the origin, behind whose straddling tie no insert follows -- there the
    # heap keeps the lowest indices too, and the true rule passes)
    only = {(w, 0) for w in range(len(run.case.worlds))} if variant == "ties_to_highest" else None
    for p, ps in enumerate(run.passes):
        assert not RC.errors(run, p, 1.0, mode=mode, only=only)["bad"], "the true rule must pass where the variant is tried"
        e = RC.errors(run, p, 1.0, mode=mode, variant=variant, only=only)
        over = [k for k, v in RC.ratios(e["err"]).items() if v > 1.0]
        if e["bad"] or over:
            caught.append("%s: %s" % (ps["tag"], e["bad"][0] if e["bad"] else over))
    print("ROAD variant %s on %s (%s): %s" % (variant, name, mode, caught[:2]))
    assert caught, "the wrong rule '%s' passes on %s: the case does not aim at it" % (variant, name)


def test_the_comparison_raises_on_a_moved_row_a_swapped_pair_and_a_wrong_padding_row(oracle_mod):
    run = _oracle_run(("road_counts", 0))["run"]
    RC.hold(run, 1, 1.0)
    rows = run.passes[1]["snaps"][0]["rows"]
    keep = rows.copy()
    try:
        rows[1, 0, 3, 0] += f32(4 * RC.ORACLE_ROAD_MAX[150.0]["x"])
        with pytest.raises(AssertionError, match="x at"):
            RC.hold(run, 1, 1.0)
        rows[...] = keep
        rows[1, 0, [3, 4]] = rows[1, 0, [4, 3]]
        with pytest.raises(AssertionError):
            RC.hold(run, 1, 1.0)
        rows[...] = keep
        rows[0, 0, 199, 7] = -1
        with pytest.raises(AssertionError, match="padding rows"):
            RC.hold(run, 1, 1.0)
    finally:
        rows[...] = keep
