#!/usr/bin/env python3
"""The BC policy forward of one trainer batch (B = 512 samples, 128 slots, num_stack 5, num_layer (3, 2), 6 components), two
ways, one JSON line:

  (a) DeviceBCPolicy.forward with out= (gd_bc_forward: context, mixture parameters, deterministic action and NLL);
  (b) the stand-in module of tests/bc_cases.py (StandIn: the reference's operators in eager torch float32) on the same
      device, the same weights and the same inputs, producing the same outputs.

Observations are synthetic: uniform in [-1, 1], masks 40 % padding.  (a) and (b) alternate in one process, --runs each: device
events around --calls calls after a warm-up.  Reported: the median and the range of the microseconds per call, the peak
device memory either side allocates during a call (torch's allocator statistics; (a)'s includes its chunk scratch), (a)'s
launch count and scratch bytes, the largest difference between (a)'s and (b)'s context.
The per-kernel split takes two more steps, the second without a device:
  1. rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bc_forward.py --runs 1 --calls 5 --only a
  2. tools/bc_forward.py --merge FILE --kernel-stats DIR/.../*_kernel_stats.csv
     adds `kernel_average_us` and `kernel_calls` (the k_bc_* rows) to the JSON line in FILE and rewrites it.
tools/bc_forward.py [--rows 512] [--agents 128] [--stack 5] [--runs 3] [--calls 20] [--only a] [--out FILE]"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.bc_policy import DeviceBCPolicy, obs_width  # noqa: E402
from tests import bc_cases as BC  # noqa: E402

OUTPUTS = ("context", "means", "covariances", "weights", "actions", "nll")


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls  # microseconds per call


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(us):
    return dict(us=us, median=statistics.median(us), lo=min(us), hi=max(us))


def merge(path, stats):
    """Step 2 of the per-kernel split: no device is touched."""
    with open(path) as f:
        res = json.loads(f.readline())
    with open(stats) as f:
        rows = [r for r in csv.DictReader(f) if "k_bc_" in r["Name"]]
    name = lambda r: re.search(r"k_bc_\w+", r["Name"]).group(0)  # noqa: E731
    res["kernel_average_us"] = {name(r): float(r["AverageNs"]) / 1e3 for r in rows}
    res["kernel_calls"] = {name(r): int(r["Calls"]) for r in rows}
    res["kernel_total_share"] = {name(r): float(r["Percentage"]) for r in rows}
    line = json.dumps(res)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--stack", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=("a",), default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main(args):
    B, A, R, cfg = args.rows, args.agents, args.stack, BC.CFG
    sd = BC.state_dict(R, cfg)
    bc = DeviceBCPolicy.from_state_dict(sd, max_agents=A, num_stack=R, **cfg)
    chunks = -(-B // bc.chunk_rows)
    res = dict(tool="tools/bc_forward.py", rows=B, slots=A, num_stack=R, obs_width=obs_width(A), config=cfg, runs=args.runs,
               calls=args.calls, observations="synthetic", source_stamp=bench.source_stamp(), chunk_rows=bc.chunk_rows,
               a_launches_per_call=chunks * (2 * cfg["num_layer"][0] + 2 * cfg["num_layer"][1] + 3),
               a_scratch_bytes=4 * int(bc._scratch.numel()), a_nbytes=bc.nbytes(B))
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((B, R, obs_width(A)), device="cuda", generator=g) * 2 - 1
    pm = torch.rand((B, R, A - 1), device="cuda", generator=g) < 0.4
    rm = torch.rand((B, R, 200), device="cuda", generator=g) < 0.4
    expert = torch.randn((B, 1, 3), device="cuda", generator=g)
    out = bc.forward(obs, pm, rm, OUTPUTS, deterministic=True, expert_actions=expert)
    run_a = lambda: bc.forward(obs, pm, rm, OUTPUTS, deterministic=True, expert_actions=expert, out=out)  # noqa: E731
    a_us, b_us = [], []
    if args.only == "a":
        a_us = [timed(run_a, args.calls) for _ in range(args.runs)]
    else:
        net = BC.StandIn(sd, A, cfg, torch.float32, "cuda")

        def run_b():
            o = net.forward(obs, pm, rm, expert)
            c = o["weights"].argmax(-1)
            return o, torch.gather(o["means"], 1, c[:, None, None].expand(-1, 1, 3))

        res["max_context_difference"] = float((run_a()["context"] - run_b()[0]["context"]).abs().max())
        for _ in range(args.runs):
            a_us.append(timed(run_a, args.calls))
            b_us.append(timed(run_b, args.calls))
        res["a_peak_bytes_in_call"], res["b_peak_bytes_in_call"] = peak_bytes(run_a), peak_bytes(run_b)
        res["b"] = summary(b_us)
    res["a"] = summary(a_us)
    if b_us:
        res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
        res["a_faster_than_b"] = res["a"]["hi"] < res["b"]["lo"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ARGS = arguments()
    if ARGS.merge:
        merge(ARGS.merge, ARGS.kernel_stats)
    else:
        with torch.cuda.stream(torch.cuda.Stream()):
            main(ARGS)
