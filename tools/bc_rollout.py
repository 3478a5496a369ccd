#!/usr/bin/env python3
"""One 91-step closed-loop episode with the BC policy in the loop (128 slots, num_stack 5, num_layer (3, 2), 6 components), two
ways (three with --compact) on the same GPU, same scenes and weights, one JSON line:

  (a) ClosedLoopBC.run(): one C call (gd_bc_rollout);
  (b) the Python composition of the tests' reference loop (tests/bc_rollout_reference.closed_loop): the call-sequence harness
      plus one DeviceBCPolicy call per step on obs[~dead], with its boolean-mask gathers, the `cat` of the stacked observation
      and the scatter into the action tensor;
  (c) with --compact, ClosedLoopBC.run(compact=True): one C call (gd_bc_rollout_compact), the forward on the rows still alive.

The worlds are the three committed test scenes tiled --tiles times (default 64: 192 worlds, 832 controlled agents).  (a) and (b)
alternate in one process, --runs each after a warm-up run of either: device events around (a), a host clock around (b), which
synchronises by itself every step.  Also timed, with events, on the same simulator and rows: 91 gd_bc_forward calls on all N rows
(the forward's share of the episode) and 91 bare steps of the simulator; what is left of (a) is the reset, the row, action and
bookkeeping kernels and the summary together.  Reported too: whether (a) and (b) agree bit for bit in every per-row output.
With --compact (c) alternates with (a) and (b) under the same events; reported are the mean of live_count / N over the
iterations that ran, whether (c) agrees with (a) bit for bit, and (c) - (a) over the first --head-steps steps, where nearly every
row is alive and the list saves nothing: what the two list launches and the list instantiations cost by themselves.
--collision removed: agents that collide leave the episode (today's default, ignore, keeps them).
tools/bc_rollout.py [--tiles 64] [--agents 128] [--stack 5] [--runs 3] [--compact] [--collision ignore|removed]
                    [--head-steps 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd import ClosedLoopBC  # noqa: E402
from gpudrive_lab_amd.bc_policy import DeviceBCPolicy  # noqa: E402
from gpudrive_lab_amd.harness import TorchCallSequence  # noqa: E402
from tests import bc_cases as BC  # noqa: E402
from tests import bc_rollout_reference as REF  # noqa: E402
from tests import parity as P  # noqa: E402
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON  # noqa: E402

T = 91


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return dict(ms=ms, median=statistics.median(ms), lo=min(ms), hi=max(ms))


def main(args):
    A, R = args.agents, args.stack
    scenes = [TEST_JSON, SCENE_407, SCENE_4] * args.tiles
    mk = lambda: P.make_gpu_sim(scenes, max_agents=A, knn_order=0, dynamicsModel=2,  # noqa: E731
                                collisionBehaviour={"removed": 1, "ignore": 2}[args.collision],
                                roadObservationAlgorithm=1, polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1,
                                distanceToGoalThreshold=2.0, initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1,
                                isStaticAgentControlled=0)
    rsim, tsim = mk(), mk()
    pol = DeviceBCPolicy.from_state_dict(BC.state_dict(R), max_agents=A, num_stack=R, **BC.CFG)
    loop = ClosedLoopBC(rsim, pol)
    N = loop.num_agents
    h = TorchCallSequence(tsim, dynamics_model="delta_local", num_stack=R)
    run_a = lambda: loop.run()  # noqa: E731
    run_b = lambda: REF.closed_loop(h, pol, source=tsim.packed_observations)  # noqa: E731
    run_c = lambda: loop.run(compact=True)  # noqa: E731
    K = args.head_steps
    ep, r = run_a(), run_b()  # the warm-up of either
    if args.compact:
        epc = run_c()
        loop.run(n_steps=K), loop.run(n_steps=K, compact=True)
    a_ms, b_ms, c_ms, ha_ms, hc_ms = [], [], [], [], []
    for _ in range(args.runs):
        ms, ep = event_ms(run_a)
        a_ms.append(ms)
        ms, r = host_ms(run_b)
        b_ms.append(ms)
        if args.compact:
            ms, epc = event_ms(run_c)
            c_ms.append(ms)
            ha_ms.append(event_ms(lambda: loop.run(n_steps=K))[0])
            ms, head = event_ms(lambda: loop.run(n_steps=K, compact=True))
            hc_ms.append(ms)
    same = all(torch.equal(getattr(ep, k).view(torch.int32) if getattr(ep, k).dtype == torch.float32 else getattr(ep, k),
                           r[k].view(torch.int32) if r[k].dtype == torch.float32 else r[k])
               for k in ("goal_achieved", "off_road", "veh_collision", "goal_step", "off_road_step", "init_goal_dist", "goal_dist",
                         "dead", "window"))

    # the parts of (a), each alone: 91 forwards on all N rows, 91 bare steps
    pm = torch.zeros((N, R, A - 1), dtype=torch.bool, device="cuda")
    rm = torch.zeros((N, R, 200), dtype=torch.bool, device="cuda")
    pm[:, R - 1], rm[:, R - 1] = ep.partner_mask, ep.road_mask
    out = torch.empty((N, 1, 3), dtype=torch.float32, device="cuda")

    def forwards():
        for _ in range(T):
            pol(ep.window, pm, rm, deterministic=True, out=out)

    def steps():
        rsim.reset(list(range(rsim._W)))
        for _ in range(T):
            rsim.step()

    forwards(), steps()
    f_ms = [event_ms(forwards)[0] for _ in range(args.runs)]
    s_ms = [event_ms(steps)[0] for _ in range(args.runs)]
    res = dict(tool="tools/bc_rollout.py", worlds=len(scenes), slots=A, num_stack=R, rows=N, steps=T, runs=args.runs,
               config=dict(BC.CFG), source_stamp=bench.source_stamp(), iterations=int(ep.steps), episode=ep.summary(),
               a=summary(a_ms), b=summary(b_ms), forwards=summary(f_ms), sim_steps=summary(s_ms),
               a_nbytes=ClosedLoopBC.nbytes(rsim, pol), same_bits=bool(same), collision=args.collision)
    a = res["a"]["median"]
    if args.compact:
        bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
        keys = ("goal_achieved", "off_road", "veh_collision", "goal_step", "off_road_step", "init_goal_dist", "goal_dist", "dead",
                "window", "partner_value", "partner_mask", "road_mask", "any_alive", "summary_tensor")
        it = int(epc.steps)
        res.update(c=summary(c_ms), c_over_a=statistics.median(c_ms) / a, c_nbytes=ClosedLoopBC.nbytes(rsim, pol, compact=True),
                   compact_same_bits=all(torch.equal(bits(getattr(epc, k)), bits(getattr(ep, k))) for k in keys),
                   live_count=epc.live_count.tolist(), live_fraction=float(epc.live_count[:it].sum()) / (it * N),
                   head_steps=K, head_a=summary(ha_ms), head_c=summary(hc_ms),
                   head_live_fraction=float(head.live_count[:K].sum()) / (K * N),
                   head_c_minus_a_ms=statistics.median(hc_ms) - statistics.median(ha_ms))
    res["b_over_a"] = res["b"]["median"] / a
    res["forward_share_of_a"] = res["forwards"]["median"] / a
    res["sim_step_share_of_a"] = res["sim_steps"]["median"] / a
    res["rest_share_of_a"] = 1.0 - res["forward_share_of_a"] - res["sim_step_share_of_a"]
    rsim.close()
    tsim.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--stack", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--collision", choices=("ignore", "removed"), default="ignore")
    ap.add_argument("--head-steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
