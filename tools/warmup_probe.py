#!/usr/bin/env python3
"""developer tool: the warm-up of the device auto-reset at ppo_default (1024 Waymo worlds x 128 slots, linear road selection),
DeviceLearnerEnv(init_steps=k).  One JSON line.

Three phases of learner steps, in this order (run it under `rocprofv3 --kernel-trace --stats` and split the warm-up kernel's
dispatches by the counts printed: one dispatch per learner step, none from setup or host resets):
  none     --none steps in which no world ends (the warm-up launch returns at once)
  all      the step in which every world reaches the step limit together (the first episode after setup)
  typical  --typical steps with the worlds' ends spread over the episode (host resets of 1/80 of the worlds per step first)
Then, timed with CUDA events (meaningful without the profiler): the learner step in which every world ends against an ordinary
one, and the host composition of the reference -- sim.reset(every world) + advance_log_playback(k).
tools/warmup_probe.py [--init-steps 11] [--worlds 1024] [--none 40] [--typical 80]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table  # noqa: E402

WORKLOAD = "ppo_default"


def make(worlds):
    kw = bench.params_for(WORKLOAD)
    _, order, agents = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, worlds, 0, agents=agents)
    return bench.make_sim(scenes, kw, agents, 0, knn_order=order)


def event_ms(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--init-steps", type=int, default=11)
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--none", type=int, default=40)
    ap.add_argument("--typical", type=int, default=80)
    args = ap.parse_args()
    k, W = args.init_steps, args.worlds
    sim = make(W)
    env = DeviceLearnerEnv(sim, init_steps=k)
    table = action_table("classic").cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = torch.randint(0, table.shape[0], (env.num_agents,), device="cuda", generator=gen)
    step = lambda: env.step(idx)
    res = dict(tool="tools/warmup_probe.py", workload=WORKLOAD, worlds=W, init_steps=k, source_stamp=bench.source_stamp())
    # every world ends after 91 - k learner steps; the phase "none" ends one step before that
    episode = 91 - k
    assert args.none < episode
    sim.advance_log_playback(episode - 1 - args.none)
    w0 = sim.stat(46)
    for _ in range(args.none):
        step()
    torch.cuda.synchronize()
    res["none_steps"], res["none_warmed"] = args.none, sim.stat(46) - w0
    w0 = sim.stat(46)
    step()  # every world ends here
    torch.cuda.synchronize()
    res["all_steps"], res["all_warmed"] = 1, sim.stat(46) - w0
    # spread the ends: 1/80 of the worlds is reset by the host before each of 80 steps (host resets launch no warm-up)
    for g in range(80):
        sim.reset(list(range(g, W, 80)))
        step()
    w0 = sim.stat(46)
    for _ in range(args.typical):
        step()
    torch.cuda.synchronize()
    res["spread_steps"], res["typical_steps"], res["typical_warmed"] = 80, args.typical, sim.stat(46) - w0
    # timed: an ordinary learner step, the step in which every world ends, the host composition
    sim.reset(list(range(W)))
    sim.advance_log_playback(k)
    sim.advance_log_playback(episode - 2)
    res["ordinary_step_ms"] = event_ms(step)
    w0 = sim.stat(46)
    res["all_end_step_ms"] = event_ms(step)
    assert sim.stat(46) - w0 == W, "every world was to end in the timed step"
    res["host_reset_all_ms"] = event_ms(lambda: sim.reset(list(range(W))))
    res["host_advance_ms"] = event_ms(lambda: sim.advance_log_playback(k))
    res["host_composition_ms"] = res["host_reset_all_ms"] + res["host_advance_ms"]
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main()
