#!/usr/bin/env python3
"""One 91-step closed-loop episode with the BC policy in the loop and the read-outs of the reference's interpretability scripts
(importance_weight.py's attention scores, intervention.py's probe classes) taken per step, on the workload tools/bc_rollout.py
times (the three committed scenes tiled 64 times: 192 worlds x 128 slots, 832 controlled agents, num_stack 5), under collision
behaviour IGNORE and AgentRemoved, on the same GPU, scenes and weights, one JSON line:

  (a) ClosedLoopBC.run();
  (b) run(attention=True);
  (c) run(readout=ro) with one (ego, other) pair of probes at ('ro_attn', 0) and a label;
  (d) the same with four pairs;
  (e) the Python composition a user had to write before: the call-sequence harness stepped in Python
      (tests/bc_rollout_reference.closed_loop) and per step, on obs[~dead], the forward, `context(ego_attn_score=)` and one
      `probe.predict` per probe -- each of which runs the attention encoder again.  It reads the probes at their own taps (the
      inner layer could not be named) and has no ego_pred_prime; with one pair (e1) and with four (e4).

(a) - (d) also with compact=True (ac, bc, cc, dc).  All alternate in one process, --runs each after a warm-up run of each; device
events around the C-call variants, a host clock around (e), which synchronises by itself every step.  Also timed with events, on
the same rows: 91 `hidden('ro_attn')` calls on all N rows -- what ONE re-encoding per step costs -- as the bound (c) - (a) is held
against.  Reported: the times, (b) - (a), (c) - (a), (d) - (c), that bound, and whether every field of (a) is bit-identical in (d).
tools/bc_readout_time.py [--tiles 64] [--runs 3] [--out FILE]"""
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
from gpudrive_lab_amd import ClosedLoopBC, DeviceLinearProbe, ProbeReadout  # noqa: E402
from gpudrive_lab_amd.bc_policy import DeviceBCPolicy  # noqa: E402
from gpudrive_lab_amd.harness import TorchCallSequence  # noqa: E402
from tests import bc_cases as BC  # noqa: E402
from tests import bc_rollout_reference as REF  # noqa: E402
from tests import parity as P  # noqa: E402
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON  # noqa: E402

T, A, R = 91, 128, 5


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


def head(seed):
    g = torch.Generator().manual_seed(seed)
    return {"head.weight": torch.randn(64, 64, generator=g), "head.bias": torch.randn(64, generator=g)}


class Composed:
    """(e): the policy the stepped loop calls -- the forward, the attention scores and one predict per probe."""

    def __init__(self, pol, probes):
        self.pol, self.probes = pol, probes

    def __call__(self, obs, pm, rm, deterministic=False, u=None, z=None):
        actions = self.pol(obs, pm, rm, deterministic=deterministic, u=u, z=z)
        score = torch.empty((obs.shape[0], 4, A - 1), dtype=torch.float32, device=obs.device)
        self.pol.context(obs, pm, rm, ego_attn_score=score)
        self.kept = [score] + [pr.predict(obs, pm, rm) for pr in self.probes]
        return actions


def main(args):
    scenes = [TEST_JSON, SCENE_407, SCENE_4] * args.tiles
    pol = DeviceBCPolicy.from_state_dict(BC.state_dict(R), max_agents=A, num_stack=R, **BC.CFG)
    others = [DeviceLinearProbe(pol, head(10 + i), model="late_lp", exp="other") for i in range(4)]
    egos = [DeviceLinearProbe(pol, head(20 + i), model="late_lp", exp="ego") for i in range(4)]
    ro1 = ProbeReadout(pol, "ro_attn", 0, other=others[:1], ego=egos[:1], labels=10)
    ro4 = ProbeReadout(pol, "ro_attn", 0, other=others, ego=egos, labels=10)
    res = dict(tool="tools/bc_readout_time.py", worlds=len(scenes), slots=A, num_stack=R, steps=T, runs=args.runs,
               config=dict(BC.CFG), source_stamp=bench.source_stamp(), workloads={})
    for name, behaviour in (("ignore", 2), ("removed", 1)):
        mk = lambda: P.make_gpu_sim(scenes, max_agents=A, knn_order=0, dynamicsModel=2, collisionBehaviour=behaviour,  # noqa: E731
                                    roadObservationAlgorithm=1, polylineReductionThreshold=0.1, observationRadius=50.0,
                                    rewardType=1, distanceToGoalThreshold=2.0, initOnlyValidAgentsAtFirstStep=1,
                                    IgnoreNonVehicles=1, isStaticAgentControlled=0)
        rsim, tsim = mk(), mk()
        loop = ClosedLoopBC(rsim, pol)
        N = loop.num_agents
        h = TorchCallSequence(tsim, dynamics_model="delta_local", num_stack=R)
        variants = {}
        for tag, compact in (("", False), ("c", True)):
            variants["a" + tag] = lambda compact=compact: loop.run(compact=compact)
            variants["b" + tag] = lambda compact=compact: loop.run(attention=True, compact=compact)
            variants["c" + tag] = lambda compact=compact: loop.run(readout=ro1, compact=compact)
            variants["d" + tag] = lambda compact=compact: loop.run(readout=ro4, compact=compact)
        composed = {"e1": Composed(pol, others[:1] + egos[:1]), "e4": Composed(pol, others + egos)}
        for k, c in composed.items():
            variants[k] = lambda c=c: REF.closed_loop(h, c, source=tsim.packed_observations)
        last = {k: fn() for k, fn in variants.items()}  # the warm-up of each
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.runs):
            for k, fn in variants.items():
                t, last[k] = (host_ms if k in composed else event_ms)(fn)
                ms[k].append(t)
        # one re-encoding per step: 91 hidden('ro_attn') calls on all N rows
        ep = last["a"]
        pm = torch.zeros((N, R, A - 1), dtype=torch.bool, device="cuda")
        rm = torch.zeros((N, R, 200), dtype=torch.bool, device="cuda")
        pm[:, R - 1], rm[:, R - 1] = ep.partner_mask, ep.road_mask
        hid = torch.empty((N, A, 64), dtype=torch.float32, device="cuda")

        def hiddens():
            for _ in range(T):
                pol.hidden(ep.window, pm, rm, tap="ro_attn", out=hid)

        hiddens()
        h_ms = [event_ms(hiddens)[0] for _ in range(args.runs)]
        bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
        same = all(torch.equal(bits(getattr(last["d"], k)), bits(v)) for k, v in ep.__dict__.items() if isinstance(v, torch.Tensor))
        out = dict(rows=N, iterations=int(ep.steps), **{k: summary(v) for k, v in ms.items()}, hidden_x91=summary(h_ms),
                   d_holds_every_field_of_a=bool(same), live_fraction=float(last["ac"].live_count[:int(ep.steps)].sum()) / (int(ep.steps) * N),
                   nbytes=dict(a=ClosedLoopBC.nbytes(rsim, pol), b=ClosedLoopBC.nbytes(rsim, pol, attention=True),
                               c=ClosedLoopBC.nbytes(rsim, pol, readout=ro1), d=ClosedLoopBC.nbytes(rsim, pol, readout=ro4)))
        med = lambda k: out[k]["median"]  # noqa: E731
        for tag in ("", "c"):
            out["b_minus_a" + tag] = med("b" + tag) - med("a" + tag)
            out["c_minus_a" + tag] = med("c" + tag) - med("a" + tag)
            out["d_minus_c" + tag] = med("d" + tag) - med("c" + tag)
        out["one_reencoding_per_step"] = med("hidden_x91")
        out["c_minus_a_below_one_reencoding"] = out["c_minus_a"] < out["one_reencoding_per_step"]
        out["e1_over_c"], out["e4_over_d"] = med("e1") / med("c"), med("e4") / med("d")
        res["workloads"][name] = out
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
