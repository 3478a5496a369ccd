#!/usr/bin/env python3
"""One BC gradient step on one trainer batch (B = 512 samples, 128 slots, num_stack 5, num_layer (3, 2), 6 components), two ways
on the same GPU, one JSON line:

  (a) DeviceBC.update: one C call (gd_bc_update: forward, row statistics, backward, clipping and AdamW, the evaluation
      policy's packed weights stored in place);
  (b) the path before it: loss = tbp(obs, pm, rm, expert).mean() on a TrainableBCPolicy, opt.zero_grad(), loss.backward(),
      torch.nn.utils.clip_grad_norm_(.., 20), torch.optim.AdamW.step(), then DeviceBCPolicy.load_state_dict(tbp.state_dict()).

Inputs are tools/bc_forward.py's: synthetic observations uniform in [-1, 1], masks 40 % padding.  (a) and (b) start from the
same weights and alternate in one process, --runs each: device events around --calls steps after a warm-up.  Reported: the
median and the range of the microseconds per step of either, the peak device memory either side allocates during a step and
what (a) holds in all (nbytes), whether (a) is not slower than (b) beyond (b)'s own run-to-run spread, and the largest
difference of the weights relative to each tensor's largest weight, after one step from the same weights and after the timed
steps (every step on the same batch: the two trajectories part as any two float32 runs of Adam do).
The launches per step take two more steps, the second without a device:
  1. rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bc_update.py --runs 1 --calls 5 --only a
  2. tools/bc_update.py --merge FILE --kernel-stats DIR/.../*_kernel_stats.csv
(--only a makes 3 warm-up steps, 5 timed ones and one more before them: the calls of every kernel over those 9 steps.)

--dim 128 is the same comparison at the model of the reference's sweep (network_dim 128, num_layer (4, 3)): (a) is
DeviceBCDim.update (gd_bc_update_dim), (b) a TrainableBCPolicyDim step, torch's clip, AdamW.step and the re-pack of a 128-wide
DeviceBCPolicy.  There the result also carries what is asserted of (a): the bytes a step allocates and the host
synchronisations it makes (torch's sync debug mode), both 0.
tools/bc_update.py [--dim 64] [--rows 512] [--agents 128] [--stack 5] [--runs 3] [--calls 10] [--only a] [--out FILE]"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from bc_forward import peak_bytes, summary, timed  # noqa: E402
from gpudrive_lab_amd import DeviceBC, TrainableBCPolicy, TrainableBCPolicyDim  # noqa: E402
from gpudrive_lab_amd.bc_opt import DeviceBCDim  # noqa: E402
from gpudrive_lab_amd.bc_policy import DeviceBCPolicy, obs_width  # noqa: E402
from tests import bc_cases as BC  # noqa: E402

WARM = 3  # bc_forward.timed's warm-up steps


def merge(path, stats):
    """Step 2 of the launch count: no device is touched."""
    with open(path) as f:
        res = json.loads(f.readline())
    with open(stats) as f:
        rows = [r for r in csv.DictReader(f) if re.search(r"k_bcg?_", r["Name"])]
    name = lambda r: re.search(r"k_bcg?_\w+(<[^>]*>)?", r["Name"]).group(0)  # noqa: E731
    steps = res["runs"] * (res["calls"] + WARM) + 1 + ("network_dim" in res)  # (--dim 128 makes one more, under the sync check)
    res["kernel_average_us"] = {name(r): float(r["AverageNs"]) / 1e3 for r in rows}
    res["kernel_calls"] = {name(r): int(r["Calls"]) for r in rows}
    res["kernel_total_share"] = {name(r): float(r["Percentage"]) for r in rows}
    res["profiled_steps"] = steps
    res["launches_per_step"] = sum(res["kernel_calls"].values()) / steps
    res["update_kernels_us_per_step"] = sum(res["kernel_average_us"][k] * res["kernel_calls"][k] for k in res["kernel_calls"]
                                            if re.fullmatch(r"k_bc_(rows|sq|step|adamw)", k)) / steps
    line = json.dumps(res)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, choices=(64, 128), default=64)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--stack", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--partials", type=int, default=None)
    ap.add_argument("--chunk-rows", type=int, default=None)
    ap.add_argument("--only", choices=("a",), default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main(args):
    B, A, R, cfg = args.rows, args.agents, args.stack, BC.CFG
    kw = {} if args.chunk_rows is None else dict(chunk_rows=args.chunk_rows)
    Trainer, Module = DeviceBC, TrainableBCPolicy
    if args.dim != 64:   # the sweep's model
        cfg = dict(BC.CFG, num_layer=(4, 3))
        kw["network_dim"] = args.dim
        Trainer, Module = DeviceBCDim, TrainableBCPolicyDim
    sd = BC.state_dict(R, cfg, **({} if args.dim == 64 else dict(network_dim=args.dim)))
    bc = Trainer(sd, max_agents=A, num_stack=R, batch_size=B, partials=args.partials, **cfg, **kw)
    res = dict(tool="tools/bc_update.py", rows=B, slots=A, num_stack=R, obs_width=obs_width(A), config=cfg, runs=args.runs,
               calls=args.calls, observations="synthetic", source_stamp=bench.source_stamp(), chunk_rows=bc.chunk_rows,
               partials=bc.partials, a_nbytes=bc.nbytes, parameters=bc.G, tensors=len(bc._names))
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((B, R, obs_width(A)), device="cuda", generator=g) * 2 - 1
    pm = torch.rand((B, R, A - 1), device="cuda", generator=g) < 0.4
    rm = torch.rand((B, R, 200), device="cuda", generator=g) < 0.4
    expert = torch.randn((B, 1, 3), device="cuda", generator=g)

    def step_a():
        bc.update(obs, expert, pm, rm)

    step_a()
    a_us, b_us = [], []
    if args.only == "a":
        a_us = [timed(step_a, args.calls) for _ in range(args.runs)]
    else:
        tbp = Module.from_state_dict(sd, max_agents=A, num_stack=R, device="cuda", partials=args.partials, **cfg, **kw)
        pol = DeviceBCPolicy.from_state_dict(sd, max_agents=A, num_stack=R, **cfg, **kw)
        opt = torch.optim.AdamW(tbp.parameters(), lr=bc.learning_rate, betas=bc.betas, eps=bc.eps, weight_decay=bc.weight_decay)

        def step_b():
            loss = tbp(obs, pm, rm, expert).mean()
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(tbp.parameters(), bc.max_grad_norm)
            opt.step()
            pol.load_state_dict(tbp.state_dict())

        step_b()

        def difference():
            mine = bc.state_dict()
            return max(float((mine[k] - p.detach()).abs().max() / p.detach().abs().max().clamp_min(1e-30))
                       for k, p in tbp.named_parameters())

        res["one_step_max_relative_weight_difference"] = difference()   # one step each from the same weights
        for _ in range(args.runs):
            a_us.append(timed(step_a, args.calls))
            b_us.append(timed(step_b, args.calls))
        # both sides have made the same number of steps from the same weights
        res["max_relative_weight_difference"] = difference()
        res["steps_compared"] = int(bc._step.item())
        res["a_peak_bytes_in_step"], res["b_peak_bytes_in_step"] = peak_bytes(step_a), peak_bytes(step_b)
        res["b"] = summary(b_us)
        res["b_spread"] = res["b"]["hi"] - res["b"]["lo"]
    res["a"] = summary(a_us)
    if args.dim != 64:   # one more step, after everything that is compared or timed
        res["network_dim"] = args.dim
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")   # a host synchronisation inside the step raises
        try:
            step_a()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        res["a_bytes_allocated_per_step"], res["a_host_synchronisations_per_step"] = torch.cuda.memory_allocated() - held, 0
        assert res["a_bytes_allocated_per_step"] == 0, "the update allocated"
    if b_us:
        res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
        res["a_not_slower_beyond_b_spread"] = res["a"]["median"] <= res["b"]["median"] + res["b_spread"]
        res["a_faster_than_b"] = res["a"]["hi"] < res["b"]["lo"]
    res["last_losses"] = bc.losses()
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
