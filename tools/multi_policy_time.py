#!/usr/bin/env python3
"""One 91-step closed-loop episode with several late-fusion PPO policies in the same worlds at ppo_default (Waymo tiles, 1024
worlds x 128 slots, linear road selection), under collision behaviour IGNORE and under AgentRemoved, three ways on the same GPU,
the same scenes, weights and draws, one JSON line:

  (a) ClosedLoopMultiPPO.run() with P = 2 (owners dealt by slot parity) and P = 4 (slot mod 4): one C call
      (gd_multi_policy_rollout) after the reset;
  (b) the same episode composed in Python from what existed before that call, as well as it can be put together without a
      host synchronisation: per step and per policy `live_rows(mask_p & live)` and `pol_p(obs, u[t], rows=..., out=...)` on the
      evaluator's own [N, D] learner rows, then `torch.where(live, a, 0)`, `sim.set_discrete_actions`, `sim.step()` and the
      bookkeeping in torch (index_select of done and info by the rows' slots, masked adds, live &= ~done, an index_add_ per world
      for the world test), and after the loop the per-policy counts by index_add_.  It never breaks: all 91 iterations run;
  (c) ClosedLoopPPO.run(compact=True) with ONE policy: the floor.

All five alternate in one process, --runs each after a warm-up run of each, device events around every one (none synchronises).
Each evaluator owns the learner rows of its simulator, so (a) P = 2, (a) P = 4 and (c) have a simulator each, on the same scenes;
(b) runs on the simulator and the rows of (a) with the same P.  Reported: the times, the ratios (a) / (b) and (a) / (c), the
launches of each beside the simulator's own, and whether (a) and (b) agree in every per-policy count.
tools/multi_policy_time.py [--worlds 1024] [--runs 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd import ClosedLoopMultiPPO, ClosedLoopPPO  # noqa: E402
from gpudrive_lab_amd.policy import DevicePolicy, LiveRows, live_rows  # noqa: E402
from tests import policy_cases as PC  # noqa: E402

WORKLOAD = "ppo_default"
T = 91
SEEDS = (11, 12, 13, 14)
COUNTS = ("goal_achieved_count", "collided_count", "off_road_count")


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def summary(ms):
    return dict(ms=ms, median=statistics.median(ms), lo=min(ms), hi=max(ms))


class Composition:
    """(b): one episode by the pieces that existed before gd_multi_policy_rollout, on the rows of a ClosedLoopMultiPPO."""

    def __init__(self, sim, ev, pols, u):
        self.sim, self.ev, self.pols, self.u = sim, ev, pols, u
        N, dev = ev.num_agents, sim._device
        self.slots = ev.mask.view(-1).nonzero().squeeze(1)  # setup: a synchronisation of the composition's own
        self.world = self.slots // sim._A
        self.mine = [ev.owner == p for p in range(len(pols))]
        self.lists = [LiveRows(N, dev) for _ in pols]
        self.outs = (torch.zeros(N, dtype=torch.int64, device=dev),) + tuple(torch.zeros(N, device=dev) for _ in range(3))

    def __call__(self):
        sim, ev, u = self.sim, self.ev, self.u
        W, N, dev, world, slots = sim._W, ev.num_agents, sim._device, self.world, self.slots
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)  # noqa: E731
        goal, coll, off, lengths = f(N), f(N), f(N), f(W)
        live = torch.ones(N, dtype=torch.bool, device=dev)
        active = torch.ones(W, dtype=torch.bool, device=dev)
        zero = torch.zeros(N, dtype=torch.int64, device=dev)
        controlled = f(W).index_add_(0, world, torch.ones(N, device=dev))
        done_flat = sim.done_tensor().to_torch().view(-1)
        info_flat = sim.info_tensor().to_torch().view(-1, 5)
        sim.reset(list(range(W)))
        for t in range(T):
            for pol, mine, lr in zip(self.pols, self.mine, self.lists):
                pol(ev.obs, u[t], rows=live_rows(mine & live, out=lr), out=self.outs)
            sim.set_discrete_actions(torch.where(live, self.outs[0], zero), ev.table)
            sim.step()
            done = done_flat.index_select(0, slots) != 0
            info = info_flat.index_select(0, slots).float()
            lf = live.float()
            off += info[:, 0] * lf
            coll += (info[:, 1] + info[:, 2]) * lf
            goal += info[:, 3] * lf
            live &= ~done
            finished = f(W).index_add_(0, world, done.float()) == controlled
            lengths = torch.where(active & finished, float(t), lengths)
            active &= ~finished
        per_world = lambda flag: f(W).index_add_(0, world, flag.float())  # noqa: E731
        return dict(goal_achieved_count=torch.stack([per_world((goal > 0) & m) for m in self.mine]),
                    collided_count=torch.stack([per_world((coll > 0) & m) for m in self.mine]),
                    off_road_count=torch.stack([per_world((off > 0) & m) for m in self.mine]), episode_lengths=lengths)


def main(args):
    _, order, A = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, args.worlds, 0, agents=A)
    res = dict(tool="tools/multi_policy_time.py", workload=WORKLOAD, worlds=args.worlds, slots=A, steps=T, runs=args.runs,
               source_stamp=bench.source_stamp(), workloads={})
    pols = [DevicePolicy.from_state_dict(PC.state_dict(s, 6, 91), max_agents=A, ego_width=6) for s in SEEDS]
    slot = torch.arange(A, device="cuda").expand(args.worlds, A)
    for name, behaviour in (("ignore", 2), ("agent_removed", 1)):
        kw = dict(bench.params_for(WORKLOAD), collisionBehaviour=behaviour)
        sims = [bench.make_sim(scenes, kw, A, 0, knn_order=order) for _ in range(3)]
        evs = {P: ClosedLoopMultiPPO(sim, {"p%d" % p: (pols[p], slot % P == p) for p in range(P)})
               for P, sim in zip((2, 4), sims)}
        floor = ClosedLoopPPO(sims[2], pols[0])
        N = floor.num_agents
        u = torch.rand((T, N), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        seed = lambda: torch.Generator(device="cuda").manual_seed(0)  # noqa: E731  (run() draws the same u from the same seed)
        variants = {"a2": lambda: evs[2].run(generator=seed()), "a4": lambda: evs[4].run(generator=seed()),
                    "b2": Composition(sims[0], evs[2], pols[:2], u), "b4": Composition(sims[1], evs[4], pols[:4], u),
                    "c": lambda: floor.run(generator=seed(), compact=True)}
        last = {k: fn() for k, fn in variants.items()}  # the warm-up of each
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.runs):
            for k, fn in variants.items():
                t, last[k] = event_ms(fn)
                ms[k].append(t)
        out = dict(rows=N, iterations=int(last["a2"].steps), **{k: summary(v) for k, v in ms.items()})
        for P in (2, 4):
            a, b = last["a%d" % P], last["b%d" % P]
            out["same_results_P%d" % P] = bool(torch.equal(a.u, u)) and all(
                torch.equal(getattr(a, "policy_" + k), b[k]) for k in COUNTS) and bool(torch.equal(a.episode_lengths, b["episode_lengths"]))
            out["a_over_b_P%d" % P] = out["a%d" % P]["median"] / out["b%d" % P]["median"]
            out["a_over_c_P%d" % P] = out["a%d" % P]["median"] / out["c"]["median"]
            out["mean_list_count_over_rows_P%d" % P] = float(a.list_count.sum(1).float().mean()) / N
            out["episode_P%d" % P] = a.summary()
        out["a4_over_a2"] = out["a4"]["median"] / out["a2"]["median"]
        out["b4_over_b2"] = out["b4"]["median"] / out["b2"]["median"]
        out["launches_beside_the_steps"] = dict(
            a="%d for every P: 91 x (2 list + 3 forward + 2) + 4" % (T * 7 + 4),
            b="91 x 5 P for the lists and the forwards (P = 2: %d, P = 4: %d), beside torch's own kernels for the scatter and the "
              "bookkeeping" % (T * 10, T * 20),
            c="%d: 91 x (2 list + 3 forward + 2) + 2" % (T * 7 + 2))
        res["workloads"][name] = out
        for sim in sims:
            sim.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main(a)
