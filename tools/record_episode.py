#!/usr/bin/env python3
"""One recorded expert episode (the imitation-learning dataset of gpudrive/integrations/il/storage.py) at ppo_default (Waymo
tiles, 1024 worlds x 128 slots, linear road selection), three ways, one JSON line:

  (a) ExpertRecorder.record(): one C call, one kernel launch per time index between the steps;
  (b) the best composition without it: per step, expert_actions()[:, :, t] copied into the action tensor and sim.step(), with
      packed_observations()[slots] and the harness's masks scattered into [N, 91, ...] by vectorised torch (torch.where on the
      live rows: no host synchronisation; it always runs all 91 steps);
  (c) at --small-worlds only, the per-index reference loop of tests/il_reference.py, for the record ((a) is timed at that
      size as well, beside it).

(a) and (b) alternate in one process, --runs each; medians of the milliseconds per episode (a host clock around work that ends
in a device synchronise; the reset is inside, the allocations too).  Also: k_record's average duration from HIP events around
every launch (a run of its own: it synchronises), and its achieved bytes/s over its algorithmic bytes -- live (row, step)s x
(raw self + partner + road rows read, D * 4 + masks + action + pose written), one byte per dead one.  bench.py's workload
builders are imported, not changed.
tools/record_episode.py [--worlds 1024] [--small-worlds 8] [--runs 3] [--out FILE]"""
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
from gpudrive_lab_amd.harness import TorchCallSequence  # noqa: E402
from gpudrive_lab_amd.recorder import ExpertRecorder, packed_width  # noqa: E402
from tests import il_reference  # noqa: E402

WORKLOAD = "ppo_default"
T = 91
_NAMES = {0: "classic", 1: "bicycle", 2: "delta_local"}


def make(worlds):
    kw = bench.params_for(WORKLOAD)
    _, order, agents = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, worlds, 0, agents=agents)
    return bench.make_sim(scenes, kw, agents, 0, knn_order=order), agents


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class TorchComposition:
    """(b): what a caller could build from the exported tensors, expert_actions() and packed_observations()."""

    def __init__(self, sim, mask):
        self.sim, self.A, self.W = sim, sim._A, sim._W
        self.slots = mask.view(-1).nonzero().squeeze(1)
        self.N = int(self.slots.numel())
        # partner j of ego a is slot j for j < a, j + 1 otherwise (an index tensor: boolean indexing would synchronise)
        self.partner_slot = torch.tensor([[j if j < a else j + 1 for j in range(self.A - 1)] for a in range(self.A)],
                                         device=sim._device)

    def record(self):
        sim, A, W, N, slots = self.sim, self.A, self.W, self.N, self.slots
        D, dev = packed_width(A), sim._device
        sim.reset(list(range(W)))
        obs = torch.zeros((N, T, D), device=dev)
        actions = torch.zeros((N, T, 3), device=dev)
        dead_mask = torch.ones((N, T), dtype=torch.bool, device=dev)
        partner_mask = torch.full((N, T, A - 1), 2, dtype=torch.uint8, device=dev)
        road_mask = torch.ones((N, T, 200), dtype=torch.bool, device=dev)
        pos = torch.zeros((N, T, 2), device=dev)
        rot = torch.zeros((N, T, 1), device=dev)
        expert = sim.expert_actions()[0]
        exp_rows = expert.view(W * A, T, 3).index_select(0, slots)
        act = sim.action_tensor().to_torch()
        done = sim.done_tensor().to_torch().view(-1)
        info = sim.info_tensor().to_torch().view(-1, 5)
        resp = sim.response_type_tensor().to_torch().view(W, A)
        partner = sim.partner_observations_tensor().to_torch().view(W * A, A - 1, 9)
        roadmap = sim.agent_roadmap_tensor().to_torch().view(W * A, 200, 9)
        absobs = sim.absolute_self_observation_tensor().to_torch().view(W * A, 14)
        dead = torch.zeros((N,), dtype=torch.bool, device=dev)
        goal, off, col = (torch.zeros((N,), device=dev) for _ in range(3))
        two = torch.full((), 2, dtype=torch.uint8, device=dev)
        for t in range(T):
            live = ~dead
            rows = sim.packed_observations().view(-1, D).index_select(0, slots)
            obs[:, t] = torch.where(live[:, None], rows, 0.0)
            actions[:, t] = torch.where(live[:, None], exp_rows[:, t], 0.0)
            psum = rows[:, 6:6 + (A - 1) * 6].view(N, A - 1, 6).sum(-1)
            static = (resp == 2)[:, self.partner_slot].reshape(W * A, A - 1).index_select(0, slots)
            ids = partner.index_select(0, slots)[..., 8]
            pm = torch.where(static & (psum != 0), 1, torch.where(ids <= -1, 2, 0)).to(torch.uint8)
            partner_mask[:, t] = torch.where(live[:, None], pm, two)
            road_mask[:, t] = (roadmap.index_select(0, slots)[..., 7] == -1) | dead[:, None]
            a = absobs.index_select(0, slots)
            pos[:, t] = torch.where(live[:, None], a[:, 0:2], 0.0)
            rot[:, t] = torch.where(live[:, None], a[:, 7:8], 0.0)
            dead_mask[:, t] = dead
            act[:, :, :3] = expert[:, :, t]
            sim.step()
            dead = dead | (done.index_select(0, slots) != 0)
            i = info.index_select(0, slots).to(torch.float32)
            goal = torch.clamp(goal + i[:, 3], max=1.0)
            off = torch.clamp(off + i[:, 0], max=1.0)
            col = torch.clamp(col + i[:, 1] + i[:, 2], max=1.0)
        return dict(obs=obs, actions=actions, dead_mask=dead_mask, partner_mask=partner_mask, road_mask=road_mask,
                    ego_global_pos=pos, ego_global_rot=rot, goal_achieved=goal, off_road=off, veh_collision=col)


def algorithmic_bytes(ep, A):
    """What k_record has to move for this episode: see the module docstring."""
    D = packed_width(A)
    read = 8 * 4 + (A - 1) * 9 * 4 + 200 * 9 * 4
    write = D * 4 + (A - 1) + 200 + 1 + 3 * 4 + 3 * 4
    live = int((~ep.dead_mask).sum())
    return live, live * (read + write) + (ep.dead_mask.numel() - live)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--small-worlds", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(tool="tools/record_episode.py", workload=WORKLOAD, worlds=args.worlds, runs=args.runs,
               source_stamp=bench.source_stamp())

    sim, A = make(args.worlds)
    model = _NAMES[int(sim._params.dynamicsModel)]
    rec = ExpertRecorder(sim)
    comp = TorchComposition(sim, rec.mask)
    res.update(slots=A, rows=rec.num_agents, dynamics=model, nbytes=ExpertRecorder.nbytes(sim))
    rec.record()  # warm every shape of both variants
    comp.record()
    a_ms, b_ms = [], []
    same = {}
    for _ in range(args.runs):
        ms, ep = clocked(rec.record)
        a_ms.append(ms)
        ms, ref = clocked(comp.record)
        b_ms.append(ms)
        steps = int(ep.steps)
        for k, v in ref.items():  # (b) never breaks: equal where the reference's loop runs
            x = getattr(ep, k)
            same[k] = bool(torch.equal(x[:, :steps], v[:, :steps])) if x.dim() > 1 else (bool(torch.equal(x, v)) if steps == T else None)
        del ep, ref
    res.update(a_ms=a_ms, b_ms=b_ms, a_ms_median=statistics.median(a_ms), b_ms_median=statistics.median(b_ms),
               a_equals_b=same, episode_steps=steps)
    res["b_over_a"] = res["b_ms_median"] / res["a_ms_median"]
    # the playback alone (the steps both variants contain), for the bound 91 x (step + one row-sized pass)
    play = []
    for _ in range(args.runs):
        sim.reset(list(range(sim._W)))
        play.append(clocked(lambda: sim.advance_log_playback(90))[0] * 91 / 90)
    res["playback_91_steps_ms_median"] = statistics.median(play)
    # k_record alone, from events around every launch (a run of its own)
    kms = []
    for _ in range(args.runs):
        ep = rec.record(time_kernel=True)
        kms.append(rec.last_kernel_ms)
    live, nbytes = algorithmic_bytes(ep, A)
    k = statistics.median(kms)
    res.update(k_record_total_ms=kms, k_record_launches=T + 1, k_record_avg_ms=k / (T + 1), live_row_steps=live,
               row_steps=ep.dead_mask.numel(), algorithmic_bytes=nbytes, achieved_GBps=nbytes / (k * 1e-3) / 1e9)
    del ep
    sim.close()
    del sim, rec, comp
    torch.cuda.empty_cache()

    # (c) the per-index reference loop, at a small size
    if args.small_worlds > 0:
        sim, A = make(args.small_worlds)
        rec = ExpertRecorder(sim)
        rec.record()
        h = TorchCallSequence(sim, dynamics_model=model)
        c_ms, a_small = [], []
        for _ in range(args.runs):
            a_small.append(clocked(rec.record)[0])
            ms, r = clocked(lambda: il_reference.save_trajectory(h))
            c_ms.append(ms)
        res.update(small_worlds=args.small_worlds, small_rows=rec.num_agents, c_ms=c_ms, c_ms_median=statistics.median(c_ms),
                   a_small_ms=a_small, a_small_ms_median=statistics.median(a_small), c_iterations=r["iterations"])
        res["c_over_a_small"] = res["c_ms_median"] / res["a_small_ms_median"]
        sim.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main()
