#!/usr/bin/env python3
"""One learner step at ppo_default (Waymo tiles, 1024 worlds x 128 slots, linear road selection), two ways, one JSON line:

  (a) the best path without learner rows: the full direct pack ([W, A, D], only = 1), the action indices decoded in torch and
      scattered into action[:, :, :3] of the controlled slots, the simulator step + EpisodeTracker, then index_select of the
      controlled rows out of the packed tensor and the four flat gathers (slot indices computed once at setup: no host sync);
  (b) DeviceLearnerEnv.step: the same, with the indices decoded on the device and every output written per learner row.

Milliseconds per learner step (CUDA events over --steps steps after --warmup, the step repeated as a PPO rollout calls it),
the kernel times of the row writers (the state step, which writes the ego + partner columns, and the road kernel; HIP events
around every launch, steps kernel by kernel), and the bytes of both observation buffers.  bench.py's workload builders are
imported, not changed.  --init-steps k: both paths warm every world k steps at setup and every world they reset on the
device (EpisodeTracker / DeviceLearnerEnv init_steps; --warmup-scope picks the scope).  --reset-at n: before the timing the
worlds are advanced by log playback so that their episodes end at step n of the timed window (default: no advance, as
before).

--reward-type reward_conditioned times the reward-conditioned learner's [N, D + 3] rows two ways instead:
  (a) DeviceLearnerEnv's [N, D] rows with the conditioned tracker, then the torch assembly: index_select of the weights by the
      slot index (computed once at setup) and torch.cat into [N, D + 3];
  (b) ConditionedLearnerEnv.step: the rows written as [N, D + 3] by the step's kernels.
tools/learner_step.py [--worlds 1024] [--steps 50] [--warmup 10] [--init-steps 0] [--reset-at -1] [--reward-type T]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.episode import EpisodeTracker  # noqa: E402
from gpudrive_lab_amd.learner import ConditionedLearnerEnv, DeviceLearnerEnv, action_table  # noqa: E402

WORKLOAD = "ppo_default"


def make(worlds):
    kw = bench.params_for(WORKLOAD)
    _, order, agents = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, worlds, 0, agents=agents)
    return bench.make_sim(scenes, kw, agents, 0, knn_order=order), agents


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def kernel_ms(sim, step, steps):
    """Per-launch ms of the state step (0) and the road kernel (1) over `steps` steps run kernel by kernel."""
    sim.kernel_timing(True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    out = {}
    for k, name in ((0, "state_step"), (1, "road_obs")):
        ms, n = sim.kernel_timing_read(k)
        out[name] = ms / max(n, 1)
        out[name + "_launches"] = n
    sim.kernel_timing(False)
    return out


def conditioned(args, res, table, idx_for, pre):
    """(a) [N, D] rows + torch assembly, (b) ConditionedLearnerEnv; both with the conditioned tracker."""
    k = args.init_steps
    sim, A = make(args.worlds)
    D = 6 + (A - 1) * 6 + 200 * 13
    # DeviceLearnerEnv refuses reward_conditioned at its front door (the rows it writes are [N, D]); its setup takes it
    env = DeviceLearnerEnv.__new__(DeviceLearnerEnv)
    env._init(sim, None, True, k, args.warmup_scope, dict(reward_type="reward_conditioned"))
    if pre > 0:
        sim.advance_log_playback(pre)
    N = env.num_agents
    idx = idx_for(N)
    slots = env.controlled_agent_mask.view(-1).nonzero().squeeze(1)  # setup: the one sync
    wflat = env.tracker.reward_weights_tensor.view(-1, 3)
    obs = torch.empty((N, D + 3), dtype=torch.float32, device="cuda")

    def step_a():
        rows, r, t, u, m = env.step(idx)
        torch.cat((rows[:, :6], wflat.index_select(0, slots), rows[:, 6:]), 1, out=obs)
        return obs, r, t, u, m

    res["rows"] = N
    res["a_ms_per_step"] = timed(step_a, args.steps, args.warmup)
    res["a_kernels_ms"] = kernel_ms(sim, step_a, args.steps)
    res["a_obs_bytes"] = N * (2 * D + 3) * 4
    sim.close()
    del sim, env, obs, wflat
    torch.cuda.empty_cache()

    sim, A = make(args.worlds)
    env = ConditionedLearnerEnv(sim, init_steps=k, warmup=args.warmup_scope)
    assert env.num_agents == N
    if pre > 0:
        sim.advance_log_playback(pre)

    def step_b():
        return env.step(idx)

    w0 = sim.stat(46)
    res["b_ms_per_step"] = timed(step_b, args.steps, args.warmup)
    res["b_worlds_warmed"] = sim.stat(46) - w0
    res["b_episodes"] = env.pop_stats().get("num_completed_episodes", 0)
    res["b_kernels_ms"] = kernel_ms(sim, step_b, args.steps)
    res["b_obs_bytes"] = N * (D + 3) * 4
    sim.close()
    res["b_over_a"] = res["b_ms_per_step"] / res["a_ms_per_step"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--init-steps", type=int, default=0)
    ap.add_argument("--warmup-scope", default="reset_worlds", choices=("reset_worlds", "all_worlds"))
    ap.add_argument("--reset-at", type=int, default=-1)
    ap.add_argument("--reward-type", default="weighted_combination", choices=("weighted_combination", "reward_conditioned"))
    args = ap.parse_args()
    k = args.init_steps
    # log-playback steps before the timing: the episode (91 - k learner steps after the setup's warm-up) ends at step
    # reset_at of the timed window, which follows the --warmup untimed steps
    pre = 0 if args.reset_at < 0 else max(0, 91 - k - args.warmup - args.reset_at - 1)
    gen = torch.Generator(device="cuda").manual_seed(0)
    table = action_table("classic").cuda()
    res = dict(tool="tools/learner_step.py", workload=WORKLOAD, worlds=args.worlds, steps=args.steps, warmup=args.warmup,
               init_steps=k, warmup_scope=args.warmup_scope, reset_at=args.reset_at, source_stamp=bench.source_stamp())
    if args.reward_type == "reward_conditioned":
        res["reward_type"] = args.reward_type
        conditioned(args, res, table, lambda n: torch.randint(0, table.shape[0], (n,), device="cuda", generator=gen), pre)
        return

    # (a) full direct pack + torch decode + gathers
    sim, A = make(args.worlds)
    assert sim.direct_pack(only=True)
    if k > 0:
        sim.advance_log_playback(k)  # (a fresh simulator: what DeviceLearnerEnv's setup does)
    if pre > 0:
        sim.advance_log_playback(pre)
    tr = EpisodeTracker(sim, init_steps=k, warmup=args.warmup_scope)
    slots = tr.controlled_agent_mask.view(-1).nonzero().squeeze(1)  # setup: the one sync
    N = int(slots.numel())
    D = 6 + (A - 1) * 6 + 200 * 13
    act = sim.action_tensor().to_torch().view(-1, 10)
    packed = sim.packed_observations().view(-1, D)
    idx = torch.randint(0, table.shape[0], (N,), device="cuda", generator=gen)

    def step_a():
        act[slots, :3] = table[idx]
        r, t, u, m = tr.step()
        return (packed.index_select(0, slots), r.view(-1)[slots], t.view(-1)[slots], u.view(-1)[slots], m.view(-1)[slots])

    res["rows"] = N
    res["a_ms_per_step"] = timed(step_a, args.steps, args.warmup)
    res["a_kernels_ms"] = kernel_ms(sim, step_a, args.steps)
    res["a_obs_bytes"] = args.worlds * A * D * 4
    sim.close()
    del sim, tr, act, packed
    torch.cuda.empty_cache()

    # (b) DeviceLearnerEnv
    sim, A = make(args.worlds)
    env = DeviceLearnerEnv(sim, init_steps=k, warmup=args.warmup_scope)
    assert env.num_agents == N
    if pre > 0:
        sim.advance_log_playback(pre)

    def step_b():
        return env.step(idx)

    w0 = sim.stat(46)
    res["b_ms_per_step"] = timed(step_b, args.steps, args.warmup)
    res["b_worlds_warmed"] = sim.stat(46) - w0
    res["b_episodes"] = env.pop_stats().get("num_completed_episodes", 0)
    res["b_kernels_ms"] = kernel_ms(sim, step_b, args.steps)
    res["b_obs_bytes"] = N * D * 4
    sim.close()
    res["b_over_a"] = res["b_ms_per_step"] / res["a_ms_per_step"]
    print(json.dumps(res))


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main()
