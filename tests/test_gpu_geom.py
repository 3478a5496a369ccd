"""GPU suite: k_bev and k_lidar on the constructed worlds of tests/geom_cases.py, held to the oracle (P.compare_bev /
P.compare_lidar unchanged: 0 cells / 0 rays off, depth 1e-4) AND to the float64 references of tests/geom_reference.py outside
their own margin masks (cell value, hit / miss and type exact; depth and hit position within twice the largest difference the
CPU suite measures between the oracle and the reference, GC.ORACLE_DEPTH_MAX -- never a figure from the kernel's own output).

Each case runs as a reset pass (poses written with debug_set_state, every variant) and once as a step pass: the State model
hands every agent back its own pose except two, so the BEV / LiDAR dirty flags decide what is repainted / retraced.

A difference from the oracle on an element the reference calls marginal is not a kernel bug: the failure text says how many of
the differing elements are marginal; the remedy is to nudge the case's geometry, not the bounds."""
import numpy as np
import pytest

from tests import geom_cases as GC
from tests import geom_reference as GR
from tests import parity as P

pytestmark = pytest.mark.gpu

DEPTH_BOUND = GC.GPU_DEPTH_FACTOR * GC.ORACLE_DEPTH_MAX


def _sims(O, case, scenes, variant, model):
    kw, okw, gkw = case.params(variant, model)
    gpu = P.make_gpu_sim(scenes, max_agents=case.slots, **gkw, **kw)
    orc = P.make_oracle_sim(O, scenes, max_agents=case.slots, **kw, **okw)
    return gpu, orc


def _check(case, gpu, orc, variant, tag):
    """The kernel against the oracle, then against the reference of the kernel's own input tensors."""
    assert P.compare_state_bits(gpu, orc) > 0
    try:
        if case.kind == "lidar":
            P.compare_lidar(gpu, orc)
        else:
            P.compare_bev(gpu, orc)
    except AssertionError as e:
        raise AssertionError("%s: %s [%s]" % (tag, e, GC.marginal_differences(gpu, orc, case, variant)))
    if case.kind == "lidar":
        got = GC.compare_lidar_to_reference(gpu, variant, tag)
        print("GEOM_GPU %s: rays per plane %d, masked share %s, depth |kernel - reference| %.3g (bound %.3g)" %
              (tag, got["rays"], np.round(got["share"], 5).tolist(), got["depth"], DEPTH_BOUND))
        assert got["depth"] <= DEPTH_BOUND, "%s: depth / hit position %.3g from the reference (bound %.3g)" % (tag, got["depth"], DEPTH_BOUND)
    else:
        rasters = [(w, a) for w, agents in enumerate(case.rasters) for a in agents]
        got = GC.compare_bev_to_reference(gpu, variant, tag, rasters)
        print("GEOM_GPU %s: cells %d, painted %d, masked %d" % (tag, got["cells"], got["painted"], got["masked"]))
        assert got["painted"] > 0


@pytest.mark.parametrize("name", list(GC.CASES))
def test_kernel_meets_oracle_and_reference(oracle_mod, tmp_path, name):
    case = GC.CASES[name]
    scenes = case.write(tmp_path)
    for k, variant in enumerate(case.variants):
        gpu, orc = _sims(oracle_mod, case, scenes, variant, 0)
        try:
            GC.place(case, [orc, gpu], k)
            print("GEOM_GPU %s premise (%g): %s" % (name, variant, case.premise(case, GR.read_inputs(gpu), variant)))
            _check(case, gpu, orc, variant, "%s (%g, reset pass)" % (name, variant))
        finally:
            gpu.close()
            orc.close()


@pytest.mark.parametrize("name", list(GC.CASES))
def test_kernel_meets_oracle_and_reference_after_a_step(oracle_mod, tmp_path, name):
    """The State model (dynamicsModel = 3): one step that moves two agents of every world and hands all others back the pose
    they have, bit for bit; what the step leaves in the tensors is compared (under this model the head angle, action column 2,
    is the z the action carries)."""
    case = GC.CASES[name]
    scenes = case.write(tmp_path)
    k = len(case.variants) - 1
    variant = case.variants[k]
    gpu, orc = _sims(oracle_mod, case, scenes, variant, 3)
    try:
        GC.place(case, [orc, gpu], k)
        before = GR.read_inputs(gpu)["state"]
        act = GC.state_step_actions(case, orc)
        P.write_actions(gpu, act)
        np.copyto(orc.action_tensor(), act)
        gpu.step()
        orc.step()
        after = GR.read_inputs(gpu)["state"]
        moved = int((before[..., :7].view(np.uint32) != after[..., :7].view(np.uint32)).any(-1).sum())
        live = sum(wd.n for wd in case.worlds)
        # the two scripted agents of every world, and the experts whose log puts them back at z = 1: everyone else stands still
        assert 2 * len(case.worlds) <= moved < live, "%d of %d live agents changed pose" % (moved, live)
        if case.kind == "bev":
            print("GEOM_GPU %s step: %d of %d agents moved, %d rasters repainted" % (name, moved, live, gpu.stat(31)))
        else:
            print("GEOM_GPU %s step: %d of %d agents moved" % (name, moved, live))
        _check(case, gpu, orc, variant, "%s (%g, step pass)" % (name, variant))
    finally:
        gpu.close()
        orc.close()
