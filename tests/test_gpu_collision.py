"""GPU suite: the collision phase of k_world_step on the constructed worlds of tests/collision_cases.py, held to the oracle
(agent state, info columns 0-3, the collided flag in the state and in the self observation, done: bit for bit) AND to the
float64 reference of tests/collision_reference.py, computed from the kernel's own tensors, outside the reference's margin (a
band of twice the largest separation at which the CPU suite sees the oracle's float32 narrowphase flip -- never a figure from
the kernel's output).

Each case runs as a reset pass (poses written with debug_set_state) and as a State-model step pass that moves two agents of
every world, one from clear into contact and one from contact to clear; coll_types and the crowds also run that step and one
more under every collision behaviour, and the crowds once more with the direct pack attached (another instantiation of the
kernel).

A difference from the oracle on an agent the reference calls marginal is not a kernel bug: the failure text says how many of
the differing agents are marginal; the remedy is to move the case's geometry, not the band."""
import numpy as np
import pytest

from tests import collision_cases as CC
from tests import collision_reference as CR
from tests import geom_reference as GR
from tests import parity as P

pytestmark = pytest.mark.gpu


def _sims(O, case, scenes, behaviour, model):
    kw = case.params(behaviour, model)
    return P.make_gpu_sim(scenes, max_agents=case.slots, **kw), P.make_oracle_sim(O, scenes, max_agents=case.slots, **kw)


def _check(case, gpu, orc, tag, before, behaviour, premise=None):
    """The kernel against the oracle, then against the reference of the kernel's own tensors."""
    assert P.compare_state_bits(gpu, orc) > 0
    g, o = CC.flags_of(gpu), CC.flags_of(orc)
    live = P._live_mask(orc)
    info_g, info_o = GR._np(gpu.info_tensor())[..., 0:4], GR._np(orc.info_tensor())[..., 0:4]
    same = (g["collided"] == o["collided"]) & (g["self_obs"] == o["self_obs"]) & (g["done"] == o["done"]) & (info_g == info_o).all(-1)
    if not same[live].all():
        w, a = np.argwhere(~same & live)[0]
        raise AssertionError("%s: %d agents differ from the oracle; first (world %d, agent %d): collided %s / %s, info %s / %s, done %s / %s [%s]" %
                             (tag, int((~same & live).sum()), w, a, g["collided"][w, a], o["collided"][w, a], info_g[w, a].tolist(),
                              info_o[w, a].tolist(), g["done"][w, a], o["done"][w, a], CC.marginal_differences(case, gpu, orc)))
    got = CC.compare_to_reference(case, gpu, tag, before, behaviour)
    print("COLL_GPU %s: agents %d, colliding %d, marginal %d%s" % (tag, got["agents"], got["colliding"], got["marginal"],
                                                                   "" if premise is None else ", premise: " + premise))
    assert got["marginal"] <= CC.MARGIN_AGENTS * got["agents"], tag
    return got


@pytest.mark.parametrize("name", list(CC.CASES))
def test_kernel_meets_oracle_and_reference(oracle_mod, tmp_path, name):
    case = CC.CASES[name]
    gpu, orc = _sims(oracle_mod, case, case.write(tmp_path), CR.IGNORE, 0)
    try:
        _, built = CC.place(case, [orc, gpu])
        got = _check(case, gpu, orc, name + " (reset pass)", built, None, case.premise(case, CR.read_inputs(gpu)))
        assert got["colliding"] > 0
    finally:
        gpu.close()
        orc.close()


@pytest.mark.parametrize("name", list(CC.CASES))
def test_kernel_meets_oracle_and_reference_after_a_step(oracle_mod, tmp_path, name):
    """The State model (dynamicsModel = 3) under Ignore: one step that moves two agents of every world -- one from clear into
    contact, one from contact to clear -- and hands all others back the pose they have."""
    case = CC.CASES[name]
    gpu, orc = _sims(oracle_mod, case, case.write(tmp_path), CR.IGNORE, 3)
    try:
        CC.place(case, [orc, gpu])
        inp = CR.read_inputs(gpu)
        refs = [CR.collision_reference(inp, w, case.band) for w in range(len(case.worlds))]
        _, before = CC.step_pass(case, [orc, gpu])
        _check(case, gpu, orc, name + " (step pass)", before, CR.IGNORE)
        after = CR.read_inputs(gpu)
        CC.moved_flags(case, refs, [CR.collision_reference(after, w, case.band, CR.seen_in_step(before, CR.IGNORE))
                                    for w in range(len(case.worlds))])
        if name == "coll_static_inactive":   # a controlled agent that is done and has not collided, under a neighbour
            _, seen = CC.done_rule_pass(case, [orc, gpu])
            _check(case, gpu, orc, name + " (done rule)", seen, None)
            flags = CC.flags_of(gpu)
            assert not flags["collided"][0, 9] and not flags["collided"][0, 10]
    finally:
        gpu.close()
        orc.close()


@pytest.mark.parametrize("behaviour", [0, 1, 2])
@pytest.mark.parametrize("name", CC.BEHAVIOUR_CASES)
def test_kernel_under_every_collision_behaviour(oracle_mod, tmp_path, name, behaviour):
    """The step pass and one more step under AgentStop (0), AgentRemoved (1) and Ignore (2): flags kept or forgotten, done set,
    removed agents at the padding position and colliding with nothing."""
    case = CC.CASES[name]
    gpu, orc = _sims(oracle_mod, case, case.write(tmp_path), behaviour, 3)
    try:
        CC.place(case, [orc, gpu])
        for k in (1, 2):
            _, before = CC.step_pass(case, [orc, gpu]) if k == 1 else CC.hold_step(case, [orc, gpu])
            _check(case, gpu, orc, "%s (behaviour %d, step %d)" % (name, behaviour, k), before, behaviour)
        if behaviour != CR.IGNORE:
            assert (CC.flags_of(gpu)["z"][0] == CR.PAD_Z).sum() > 0
    finally:
        gpu.close()
        orc.close()


@pytest.mark.parametrize("name", ["coll_crowd64", "coll_crowd128"])
def test_kernel_with_the_direct_pack_attached(oracle_mod, tmp_path, name):
    """direct_pack(only=True): the step kernel's instantiation that writes the packed rows; reset pass and step pass."""
    case = CC.CASES[name]
    gpu, orc = _sims(oracle_mod, case, case.write(tmp_path), CR.IGNORE, 3)
    try:
        assert gpu.direct_pack(only=True) is not False
        _, built = CC.place(case, [orc, gpu])
        _check(case, gpu, orc, name + " (direct pack, reset pass)", built, None)
        _, before = CC.step_pass(case, [orc, gpu])
        _check(case, gpu, orc, name + " (direct pack, step pass)", before, CR.IGNORE)
    finally:
        gpu.close()
        orc.close()
