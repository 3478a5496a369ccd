#!/usr/bin/env python3
"""One 91-step closed-loop episode with the late-fusion PPO policy in the loop at ppo_default (Waymo tiles, 1024 worlds x 128
slots, linear road selection), two ways on the same GPU, the same simulator, rows, weights and draws, one JSON line:

  (a) ClosedLoopPPO.run(): one C call (gd_policy_rollout) after the reset;
  (b) the Python composition of the pieces that existed before it, as well as they can be put together without a host
      synchronisation: per step `pol(obs, u[t], out=...)` on the evaluator's own [N, D] learner rows, `torch.where(live, a, 0)`,
      `sim.set_discrete_actions`, `sim.step()`, then the bookkeeping in torch (index_select of done and info by the rows' slots,
      masked adds, live &= ~done, an index_add_ per world for the world test, torch.where for the episode lengths), and after
      the loop the counts by index_add_.  It never breaks: all 91 iterations run.

(a) and (b) alternate in one process, --runs each after a warm-up run of either, device events around both (neither
synchronises).  Also timed, with events, on the same simulator and rows: 91 forwards on all N rows alone and 91 bare steps of
the simulator alone; what is left of (a) is the reset, the two kernels per step and the two at the end.  Reported too: whether
(a) and (b) agree in every per-world result, the launches of (a) beside the simulator's own, what `nbytes` says run() allocates
and what torch's allocator saw.
tools/ppo_rollout_time.py [--worlds 1024] [--runs 5] [--out FILE]

--compact times something else, one JSON line again: run() and run(compact=True) -- the forward on the list of live rows
(gd_policy_rollout_compact) -- in alternation, --runs each after a warm-up of either, with device events, at the same
ppo_default workload (collision behaviour IGNORE) and at that workload under AgentRemoved, one simulator each.  Per workload:
the two sets of times, whether every per-world result and per-row sum agrees, and the mean of live_count / N over the 91 steps
(from a record=True run's live_mask, so that it can be measured without the compact call too).  --skip-compact leaves
run(compact=True) out: the same file then runs on a commit that has no such call, for the yardstick.
tools/ppo_rollout_time.py --compact [--skip-compact] [--worlds 1024] [--runs 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd import ClosedLoopPPO  # noqa: E402
from gpudrive_lab_amd.policy import DevicePolicy  # noqa: E402
from gpudrive_lab_amd.ppo_rollout import WORLD_RESULTS  # noqa: E402
from tests import policy_cases as PC  # noqa: E402

WORKLOAD = "ppo_default"
T = 91


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def summary(ms):
    return dict(ms=ms, median=statistics.median(ms), lo=min(ms), hi=max(ms))


def composition(sim, ev, pol, u):
    """(b): one episode by the parent's pieces; returns the per-world results as run() names them."""
    W, A, N, dev = sim._W, sim._A, ev.num_agents, sim._device
    slots = ev.slots
    world = ev.world_of_row
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
        a = pol(ev.obs, u[t], out=ev.outs)[0]
        sim.set_discrete_actions(torch.where(live, a, zero), ev.table)
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
    r = dict(goal_achieved_count=per_world(goal > 0), collided_count=per_world(coll > 0), off_road_count=per_world(off > 0),
             other_count=per_world((goal == 0) & (coll == 0) & (off == 0)), controlled_per_scene=controlled,
             episode_lengths=lengths)
    for k in ("goal_achieved", "collided", "off_road", "other"):
        r["frac_" + k] = r[k + "_count"] / controlled
    return r


def compact_main(args):
    """run() against run(compact=True) at ppo_default under IGNORE and under AgentRemoved."""
    _, order, A = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, args.worlds, 0, agents=A)
    res = dict(tool="tools/ppo_rollout_time.py --compact", workload=WORKLOAD, worlds=args.worlds, slots=A, steps=T, runs=args.runs,
               source_stamp=bench.source_stamp(), compact_timed=not args.skip_compact, workloads={})
    for name, behaviour in (("ignore", 2), ("agent_removed", 1)):
        kw = dict(bench.params_for(WORKLOAD), collisionBehaviour=behaviour)
        sim = bench.make_sim(scenes, kw, A, 0, knn_order=order)
        pol = DevicePolicy.from_state_dict(PC.state_dict(11, 6, 91), max_agents=A, ego_width=6)
        ev = ClosedLoopPPO(sim, pol)
        N = ev.num_agents
        seeded = lambda **k: ev.run(generator=torch.Generator(device="cuda").manual_seed(0), **k)  # noqa: E731
        rec = seeded(record=True)
        live = rec.live_mask.sum(0).float()  # [91]: the rows live before step t (0 for iterations that do not exist)
        out = dict(rows=N, iterations=int(rec.steps), mean_live_fraction=float(live.mean()) / N,
                   live_fraction_at=dict((str(t), float(live[t]) / N) for t in (0, 10, 30, 60, 90)), episode=rec.summary())
        del rec
        ep = seeded()
        if not args.skip_compact:
            epc = seeded(compact=True)
        torch.cuda.synchronize()
        a_ms, c_ms = [], []
        for _ in range(args.runs):
            ms, ep = event_ms(seeded)
            a_ms.append(ms)
            if not args.skip_compact:
                ms, epc = event_ms(lambda: seeded(compact=True))
                c_ms.append(ms)
        out["run"] = summary(a_ms)
        if not args.skip_compact:
            out["compact"] = summary(c_ms)
            out["compact_over_run"] = out["compact"]["median"] / out["run"]["median"]
            out["mean_live_count_over_rows"] = float(epc.live_count.float().mean()) / N
            out["same_results"] = all(
                torch.equal(torch.nan_to_num(getattr(ep, k), nan=-1.0), torch.nan_to_num(getattr(epc, k), nan=-1.0))
                for k in WORLD_RESULTS + ("episode_lengths", "goal_achieved", "collided", "off_road", "summary_tensor"))
            out["launches_beside_the_steps"] = dict(run=T * (3 + 2) + 2, compact=T * (2 + 3 + 2) + 2)
        res["workloads"][name] = out
        sim.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def main(args):
    kw = bench.params_for(WORKLOAD)
    _, order, A = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, args.worlds, 0, agents=A)
    sim = bench.make_sim(scenes, kw, A, 0, knn_order=order)
    pol = DevicePolicy.from_state_dict(PC.state_dict(11, 6, 91), max_agents=A, ego_width=6)
    ev = ClosedLoopPPO(sim, pol)
    N, W = ev.num_agents, sim._W
    ev.slots = ev.mask.view(-1).nonzero().squeeze(1)  # setup: a synchronisation of the composition's own
    ev.world_of_row = ev.slots // A
    ev.outs = (torch.empty(N, dtype=torch.int64, device="cuda"),) + tuple(torch.empty(N, device="cuda") for _ in range(3))
    gen = torch.Generator(device="cuda").manual_seed(0)
    u = torch.rand((T, N), device="cuda", generator=gen)

    def run_a():  # (run() draws u [n_steps, N] from its generator: the same seed, the same draws as u)
        g = torch.Generator(device="cuda").manual_seed(0)
        return ev.run(generator=g)

    run_b = lambda: composition(sim, ev, pol, u)  # noqa: E731
    ep, r = run_a(), run_b()  # the warm-up of either
    torch.cuda.synchronize()
    a_ms, b_ms = [], []
    for _ in range(args.runs):
        ms, ep = event_ms(run_a)
        a_ms.append(ms)
        ms, r = event_ms(run_b)
        b_ms.append(ms)
    same = bool(torch.equal(ep.u, u)) and all(
        torch.equal(torch.nan_to_num(getattr(ep, k), nan=-1.0), torch.nan_to_num(r[k], nan=-1.0))
        for k in WORLD_RESULTS + ("episode_lengths",))

    def forwards():
        for t in range(T):
            pol(ev.obs, u[t], out=ev.outs)

    def steps():
        sim.reset(list(range(W)))
        for _ in range(T):
            sim.step()

    forwards(), steps()
    f_ms = [event_ms(forwards)[0] for _ in range(args.runs)]
    s_ms = [event_ms(steps)[0] for _ in range(args.runs)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    held = run_a()
    torch.cuda.synchronize()
    seen = torch.cuda.memory_allocated() - before
    res = dict(tool="tools/ppo_rollout_time.py", workload=WORKLOAD, worlds=W, slots=A, rows=N, steps=T, runs=args.runs,
               source_stamp=bench.source_stamp(), iterations=int(held.steps), episode=held.summary(), a=summary(a_ms),
               b=summary(b_ms), forwards=summary(f_ms), sim_steps=summary(s_ms),
               a_launches_beside_the_steps=T * (3 + 2) + 2, a_nbytes=ClosedLoopPPO.nbytes(sim, pol, stochastic=True),
               a_allocator_bytes=seen, row_buffer_bytes=ev.obs.numel() * 4, same_results=same)
    a = res["a"]["median"]
    res["b_over_a"] = res["b"]["median"] / a
    res["forward_share_of_a"] = res["forwards"]["median"] / a
    res["sim_step_share_of_a"] = res["sim_steps"]["median"] / a
    res["rest_share_of_a"] = 1.0 - res["forward_share_of_a"] - res["sim_step_share_of_a"]
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
    ap.add_argument("--compact", action="store_true", help="time run() against run(compact=True) instead")
    ap.add_argument("--skip-compact", action="store_true", help="with --compact: time run() alone (a commit without the call)")
    a = ap.parse_args()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        (compact_main if a.compact else main)(a)
