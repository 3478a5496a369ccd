#!/usr/bin/env python3
"""One BC training step's forward plus backward of one trainer batch (B = 512 samples, 128 slots, num_stack 5, num_layer (3, 2),
6 components), two ways, one JSON line:

  (a) TrainableBCPolicy: loss = tbp(obs, pm, rm, expert).mean(); loss.backward()  (gd_bc_forward, then gd_bc_backward, which
      runs the forward again per chunk);
  (b) the differentiable stand-in of tests/bc_grad_reference.py (Net: the reference's operators under eager torch float32
      autograd) on the same device, the same weights and the same inputs.

With --dim 128 the model is the reference sweep's (network_dim 128, num_layer (4, 3)): (a) is TrainableBCPolicyDim
(gd_bc_forward_dim, gd_bc_backward_dim), (b) the stand-in of tests/bc_wide_grad_reference.py; the result also carries the
launches per chunk.  profiles/bc_wide_backward.json is `--dim 128 --out` of it.

Inputs are tools/bc_forward.py's: synthetic observations uniform in [-1, 1], masks 40 % padding.  (a) and (b) alternate in one
process, --runs each: device events around --calls steps after a warm-up.  Reported: the median and the range of the
microseconds per step, the peak device memory either side allocates during a step, (a)'s forward alone (the share of the
step that is the recomputed forward is that time over the step's, the recomputation running the same kernels), the largest
relative difference between (a)'s and (b)'s gradients per tensor.
The per-kernel split takes two more steps, the second without a device:
  1. rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bc_backward.py --runs 1 --calls 5 --only a
  2. tools/bc_backward.py --merge FILE --kernel-stats DIR/.../*_kernel_stats.csv
tools/bc_backward.py [--dim 64] [--rows 512] [--agents 128] [--stack 5] [--runs 3] [--calls 10] [--only a] [--out FILE]"""
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
from gpudrive_lab_amd import TrainableBCPolicyDim  # noqa: E402  (at 64 it is TrainableBCPolicy: the same C calls)
from gpudrive_lab_amd.bc_policy import obs_width  # noqa: E402
from tests import bc_cases as BC  # noqa: E402
from tests import bc_grad_reference as GR  # noqa: E402
from tests import bc_wide_grad_reference as WGR  # noqa: E402


def merge(path, stats):
    """Step 2 of the per-kernel split: no device is touched."""
    with open(path) as f:
        res = json.loads(f.readline())
    with open(stats) as f:
        rows = [r for r in csv.DictReader(f) if re.search(r"k_bcg?_", r["Name"])]
    name = lambda r: re.search(r"k_bcg?_\w+(<[^>]*>)?", r["Name"]).group(0)  # noqa: E731
    res["kernel_average_us"] = {name(r): float(r["AverageNs"]) / 1e3 for r in rows}
    res["kernel_calls"] = {name(r): int(r["Calls"]) for r in rows}
    res["kernel_total_share"] = {name(r): float(r["Percentage"]) for r in rows}
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
    B, A, R = args.rows, args.agents, args.stack
    cfg = BC.CFG if args.dim == 64 else BC._cfg((4, 3), 2, 6, -20.0)
    sd = BC.state_dict(R, cfg, network_dim=args.dim)
    kw = {} if args.chunk_rows is None else dict(chunk_rows=args.chunk_rows)
    tbp = TrainableBCPolicyDim.from_state_dict(sd, max_agents=A, num_stack=R, device="cuda", partials=args.partials,
                                               network_dim=args.dim, **cfg, **kw)
    layers = sum(cfg["num_layer"])
    # per chunk: the forward (embed, kv + attn per layer, cross kv, no head without nll), XS copies, head, kvx, then per layer a
    # copy, kv, attn<SAVE>, post, dq, dkv, and the embedders
    res = dict(tool="tools/bc_backward.py", network_dim=args.dim, backward_launches_per_chunk=1 + 3 * layers + 1 + 2 + 6 * layers + 1,
               parameters=tbp._G, rows=B, slots=A, num_stack=R, obs_width=obs_width(A), config=cfg, runs=args.runs,
               calls=args.calls, observations="synthetic", source_stamp=bench.source_stamp(), chunk_rows=tbp.chunk_rows,
               partials=tbp.partials, a_nbytes=tbp.nbytes(B))
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((B, R, obs_width(A)), device="cuda", generator=g) * 2 - 1
    pm = torch.rand((B, R, A - 1), device="cuda", generator=g) < 0.4
    rm = torch.rand((B, R, 200), device="cuda", generator=g) < 0.4
    expert = torch.randn((B, 1, 3), device="cuda", generator=g)

    def step_a():
        for p in tbp.parameters():
            p.grad = None
        tbp(obs, pm, rm, expert).mean().backward()

    def forward_a():
        with torch.no_grad():
            tbp(obs, pm, rm, expert)

    step_a()
    a_us, b_us, f_us = [], [], []
    if args.only == "a":
        a_us = [timed(step_a, args.calls) for _ in range(args.runs)]
    else:
        net = (GR.Net if args.dim == 64 else WGR.Net)(sd, A, cfg, torch.float32, device="cuda")

        def step_b():
            for p in net.params.values():
                p.grad = None
            net.nll(obs, pm, rm, expert).mean().backward()

        step_b()
        res["max_relative_gradient_difference"] = max(
            float((p.grad - net.params[k].grad).abs().max() / net.params[k].grad.abs().max().clamp_min(1e-30))
            for k, p in tbp.named_parameters() if not k.endswith("k_proj.bias"))
        for _ in range(args.runs):
            a_us.append(timed(step_a, args.calls))
            b_us.append(timed(step_b, args.calls))
            f_us.append(timed(forward_a, args.calls))
        res["a_peak_bytes_in_step"], res["b_peak_bytes_in_step"] = peak_bytes(step_a), peak_bytes(step_b)
        res["b"] = summary(b_us)
        res["a_forward"] = summary(f_us)
    res["a"] = summary(a_us)
    if b_us:
        res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
        res["a_faster_than_b"] = res["a"]["hi"] < res["b"]["lo"]
        res["recomputed_forward_share"] = res["a_forward"]["median"] / res["a"]["median"]
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
