"""GPU suite: the agent road rows (agent_roadmap_tensor) on the constructed, moving worlds of tests/road_cases.py, in every road
selection the engine has -- reference order on the rank path, reference order with GPUDRIVE_NO_RANK_REPLAY=1, set order fused
and with the row kernel, linear -- after the reset pass and after EVERY step held to the oracle (the tolerances of
tests/parity.py: ints exact, state bit for bit under the State model, rows within OBS_ATOL) AND to the float64 reference of
tests/road_reference.py computed from the kernel's OWN exported tensors of that pass: the rows in the reference's order for an
order-decided agent, as a set otherwise and in set order; scale, type, id, mapType and every padding row exact; x, y and heading
within GPU_FACTOR times the oracle's measured distance from the same reference (RC.ORACLE_ROAD_MAX, measured and asserted in
the CPU suite -- never a figure from a kernel's output).

road_counts, road_jump and road_ties run once more with the direct pack attached (another instantiation of the row kernels).
The premise of a case that is about which path ran is checked on debug_road_path(), and gd_stat 21 (the rank path's bounds
audit) must be 0 at the end of every run.  A difference from the oracle on an agent the reference calls marginal is not a kernel
bug; the remedy is to move the case's geometry, not the band."""
import numpy as np
import pytest

from tests import geom_reference as GR
from tests import parity as P
from tests import road_cases as RC
from tests import road_reference as RR
from tests import step_reference as SR

pytestmark = pytest.mark.gpu

PACKED_RUNS = [(name, "ref_order_rank") for name in RC.PACKED]
IDS = lambda runs: ["%s-%s" % k for k in runs]


def _rows_against_the_oracle(run, p, gpu, orc, ref_mode, bit_identical):
    """The kernel's rows against the oracle's: in place in the reference's order and in linear mode, as sets in set order --
    there without the agents for whom a tie straddles the K-th key (set order keeps the lowest indices, the heap what its
    history left: the one documented difference).  Returns how many agents that leaves out."""
    atol = P.OBS_ATOL if bit_identical else P.FREE_OBS_ATOL
    if ref_mode != RR.SET:
        P.compare_obs(gpu, orc, atol=atol, names=["agent_roadmap_tensor"])
        return 0
    g, o = run.passes[p]["snaps"][1]["rows"].copy(), run.passes[p]["snaps"][0]["rows"].copy()
    skipped = 0
    for w, a in run.agents():
        if run.ref(p, w, a, RR.SET, sim=1)["cut_ties"]:
            g[w, a], o[w, a] = 0, 0
            skipped += 1
    gs, os_ = P._sorted_rows(g), P._sorted_rows(o)
    ok = np.isclose(gs, os_, atol=atol, rtol=0)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError("agent_roadmap (as a set): %d elements differ; first at %s gpu %r oracle %r" % (len(bad), bad[0], gs[tuple(bad[0])], os_[tuple(bad[0])]))
    return skipped


def _run(O, monkeypatch, tmp_path, name, mode, packed=False):
    case = RC.CASES[name]
    ref_mode, knn_order, algo, env = RC.MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    paths = RC.write_scenes(case, tmp_path)
    kw = case.params(algo)
    nw = len(case.worlds)
    gpu = P.make_gpu_sim(paths[:nw], max_agents=case.slots, knn_order=knn_order, **kw)
    orc = P.make_oracle_sim(O, paths[:nw], max_agents=case.slots, **kw)
    try:
        if packed:
            assert gpu.direct_pack(only=False) is not False
        run = RC.Run(case, [orc, gpu], mode)
        run.scene_paths = paths
        worst, seen, road_paths = {}, dict(agents=0, marginal=0, undecided=0, passes=0, ties=0), []

        def check(p):
            tag = "%s (%s%s), %s" % (name, mode, ", direct pack" if packed else "", run.passes[p]["tag"])
            try:
                P.compare_ints(gpu, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
                bit_identical = case.model == SR.STATE
                if bit_identical:
                    assert P.compare_state_bits(gpu, orc) > 0
                else:
                    P.compare_state(gpu, orc)
                seen["ties"] += _rows_against_the_oracle(run, p, gpu, orc, ref_mode, bit_identical)
            except AssertionError as e:
                late = RC.errors(run, p, RC.GPU_FACTOR, sim=1)
                raise AssertionError("%s: against the oracle: %s [the reference calls %d of %d agents marginal, %d undecided]" % (
                    tag, e, late["marginal"], late["agents"], late["undecided"]))
            e = RC.hold(run, p, RC.GPU_FACTOR, sim=1)
            for k, v in e["ratio"].items():
                worst[k] = max(worst.get(k, 0.0), v)
            seen["agents"] = max(seen["agents"], e["agents"])
            seen["marginal"], seen["undecided"] = max(seen["marginal"], e["marginal"]), max(seen["undecided"], e["undecided"])
            seen["passes"] += 1
            road_paths.append(gpu.debug_road_path().copy())
            if packed:
                P.compare_packed(gpu.packed_observations().cpu().numpy(), GR._np(gpu.self_observation_tensor()), GR._np(gpu.partner_observations_tensor()),
                                 run.passes[p]["snaps"][1]["rows"], what=tag + ": packed observation")

        RC.script(run, check)
        premise = case.premise(run)
        how = case.gpu_premise(run, road_paths) if case.gpu_premise else ""
        taken = sorted({int(v) if v < 0 else 1 for pth in road_paths for w, wd in enumerate(case.worlds) for v in pth[w, :wd.n]})
        audit = gpu.stat(21)
        print("ROAD_GPU %s (%s%s): passes %d, agents %d, marginal %d, undecided %d, agents with a tie across the cut %d; paths taken (1 = ranked) %s; "
              "error / bound: %s; premise: %s; %s" % (name, mode, ", direct pack" if packed else "", seen["passes"], seen["agents"], seen["marginal"],
                                                   seen["undecided"], seen["ties"], taken,
                                                   ", ".join("%s@%g %.2f" % (c, s, v) for (s, c), v in sorted(worst.items())), premise, how))
        assert audit == 0, "rank-path bounds audit: %d violations (gd_stat 21)" % audit
        assert seen["marginal"] + seen["undecided"] <= RC.MARGIN_AGENTS * seen["agents"]
        assert seen["passes"] == case.steps + 1 + len(case.events)
    finally:
        gpu.close()
        orc.close()


@pytest.mark.parametrize("key", RC.ALL_RUNS, ids=IDS(RC.ALL_RUNS))
def test_road_rows_meet_oracle_and_reference_at_every_pass(oracle_mod, monkeypatch, tmp_path, key):
    _run(oracle_mod, monkeypatch, tmp_path, *key)


@pytest.mark.parametrize("key", PACKED_RUNS, ids=IDS(PACKED_RUNS))
def test_road_rows_with_the_direct_pack_attached(oracle_mod, monkeypatch, tmp_path, key):
    """direct_pack(only=False): the row kernels' instantiation that writes the packed road columns, the raw rows kept."""
    _run(oracle_mod, monkeypatch, tmp_path, *key, packed=True)
