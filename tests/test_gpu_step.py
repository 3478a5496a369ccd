"""GPU suite: everything k_world_step does outside collision detection -- the four dynamics models, the log replay, reward, step
counter, done and info[3], the self and absolute rows -- on the constructed worlds of tests/step_cases.py, after the reset
pass and after every step held to the oracle (int tensors exact; agent state bit for bit under the State model, within
P.compare_state otherwise) AND to the float64 reference of tests/step_reference.py computed from the kernel's OWN tensors
before the pass: exact outputs exact outside the reference's margin, float outputs within GPU_FACTOR times the oracle's
measured distance from the same reference (SC.ORACLE_STEP_MAX, measured and asserted in the CPU suite -- never a figure from the
kernel's output).

step_wrap, step_goal and step_done run once more with the direct pack attached (another instantiation of the kernel), and
step_slots128 at 128 slots.  A difference from the oracle on an agent the reference calls marginal is not a kernel bug: the
failure text says how many of the differing agents are marginal; the remedy is to move the case's geometry, not the band."""
import pytest

from tests import geom_reference as GR
from tests import parity as P
from tests import step_cases as SC
from tests import step_reference as SR
from tests.test_columns import check_partner_rows_by_brute_force

pytestmark = pytest.mark.gpu

ALL_RUNS = [r for c in SC.CASE_LIST for r in c.runs()]
PACKED_RUNS = [r for name in ("step_wrap", "step_goal", "step_done") for r in SC.CASES[name].runs()]
IDS = lambda runs: ["%s-m%d-b%d-r%d" % k for k in runs]


def _run(O, tmp_path, key, packed=False):
    name, model, behaviour, reward_type = key
    case = SC.CASES[name]
    scenes = case.write(tmp_path)
    kw = case.params(model, behaviour, reward_type)
    gpu, orc = P.make_gpu_sim(scenes, max_agents=case.slots, **kw), P.make_oracle_sim(O, scenes, max_agents=case.slots, **kw)
    try:
        if packed:
            assert gpu.direct_pack(only=True) is not False
        run = SC.Run(case, [orc, gpu], model, behaviour, reward_type)
        worst, seen = {}, dict(agents=0, marginal=0, passes=0, partners=0)

        def check(before, after, tag, reset):
            tag = "%s%s, %s" % (name, " (direct pack)" if packed else "", tag)
            try:
                P.compare_ints(gpu, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
                if model == SR.STATE:
                    assert P.compare_state_bits(gpu, orc) > 0
                else:
                    P.compare_state(gpu, orc)
            except AssertionError as e:
                raise AssertionError("%s: against the oracle: %s [%s]" % (tag, e, SC.marginal_differences(run, before[1], after[1], after[0])))
            e = SC.hold(run, before[1], after[1], tag, SC.GPU_FACTOR, reset)
            for k, v in e["ratio"].items():
                worst[k] = max(worst.get(k, 0.0), v)
            seen["agents"], seen["marginal"] = max(seen["agents"], e["agents"]), max(seen["marginal"], e["marginal"])
            seen["passes"] += 1
            if name == "step_wrap" and not reset and not packed:   # opposite headings: the full quaternion product of partner_row
                n_in, n_out = check_partner_rows_by_brute_force(gpu, 50.0, as_numpy=GR._np)
                assert n_in > 0 and n_out > 0
                seen["partners"] += n_in
            if model != SR.STATE and case.steps > 3 and not reset:
                # a long free run: the next step starts from the oracle's state on both sides (what P.lockstep does)
                P.inject_and_compare(gpu, orc)

        SC.script(run, check)
        premise = case.premise(run)
        print("STEP_GPU %s%s (model %d, behaviour %d, reward type %d): passes %d, agents %d, marginal %d, partner rows %d; error / bound: %s; premise: %s" % (
            name, " direct pack" if packed else "", model, behaviour, reward_type, seen["passes"], seen["agents"], seen["marginal"], seen["partners"],
            ", ".join("%s@%g %.2f" % (c, s, v) for (s, c), v in sorted(worst.items())), premise))
        assert seen["marginal"] <= SC.MARGIN_AGENTS * seen["agents"]
        assert seen["passes"] >= case.steps + 1
    finally:
        gpu.close()
        orc.close()


@pytest.mark.parametrize("key", ALL_RUNS, ids=IDS(ALL_RUNS))
def test_kernel_meets_oracle_and_reference_at_every_step(oracle_mod, tmp_path, key):
    _run(oracle_mod, tmp_path, key)


@pytest.mark.parametrize("key", PACKED_RUNS, ids=IDS(PACKED_RUNS))
def test_kernel_with_the_direct_pack_attached(oracle_mod, tmp_path, key):
    """direct_pack(only=True): the step kernel's instantiation that writes the packed rows."""
    _run(oracle_mod, tmp_path, key, packed=True)
