#!/usr/bin/env python3
"""The policy forward of one rollout step at ppo_default's rows (N = 4435 controlled rows, 128 slots, D = 3368, 91 actions),
two ways, one JSON line:

  (a) DevicePolicy.__call__ with out= (gd_policy_forward: three launches);
  (b) the late-fusion module out of plain torch.nn layers under the reference's key names, its eager float32 forward plus
      the operators of the reference's sample_logits (logsumexp, softmax, multinomial, gather, the entropy sum), on the
      device under no_grad and eval.

Observations are synthetic: uniform in [-1, 1] with a padding tail of zero rows in each set, the ranges of packed rows.  The
weights are N(0, 1 / fan_in).  (a) and (b) alternate in one process, --runs each: device events around --calls calls after a
warm-up of 20.  Reported: the median and the range of the microseconds per call, (a)'s algorithmic FLOP/s against the
155 TFLOP/s float32 MFMA ceiling, (a)'s algorithmic bytes (the observations read once, the features and logits written and
read once, the outputs written) against the 6.29 TB/s copy ceiling, and the largest difference between (a)'s and (b)'s logits.
The per-kernel split takes two more steps, the second without a device:
  1. rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/policy_forward.py --runs 1 --calls 50
  2. tools/policy_forward.py --merge FILE --kernel-stats DIR/.../*_kernel_stats.csv
     adds `kernel_average_us` (the AverageNs column of the k_policy_* rows) to the JSON line in FILE and rewrites it.
--dropout P: (a) runs with dropout_rule=DropoutRule(P, 0) (gd_policy_forward_dropout), (b) in train mode with nn.Dropout(P),
and a third side (a0), the same DevicePolicy in eval mode (the same build without the masks), joins the alternation;
`a_over_a0` is the forward's slowdown over its own dropout-off path.  The logits of (a) and (b) are then not compared.
tools/policy_forward.py [--rows 4435] [--agents 128] [--actions 91] [--runs 3] [--calls 200] [--dropout P] [--out FILE]"""
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
from torch import nn  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.dropout import DropoutRule  # noqa: E402
from gpudrive_lab_amd.policy import DevicePolicy, obs_width  # noqa: E402

MFMA_CEILING, COPY_CEILING = 155e12, 6.29e12
EGO = 6


class LateFusion(nn.Module):
    def __init__(self, agents, actions, dropout=0.01):
        super().__init__()
        self.agents = agents

        def embed(k):
            return nn.Sequential(nn.Linear(k, 64), nn.LayerNorm(64), nn.Tanh(), nn.Dropout(dropout), nn.Linear(64, 64))

        self.ego_embed, self.partner_embed, self.road_map_embed = embed(EGO), embed(6), embed(13)
        self.shared_embed = nn.Sequential(nn.Linear(192, 128), nn.Dropout(dropout))
        self.actor, self.critic = nn.Linear(128, actions), nn.Linear(128, 1)

    def logits_value(self, obs):
        n, r0 = obs.shape[0], EGO + 6 * (self.agents - 1)
        ego = self.ego_embed(obs[:, :EGO])
        partner, _ = self.partner_embed(obs[:, EGO:r0].view(n, self.agents - 1, 6)).max(dim=1)
        road, _ = self.road_map_embed(obs[:, r0:].view(n, 200, 13)).max(dim=1)
        hidden = self.shared_embed(torch.cat([ego, partner, road], dim=1))
        return self.actor(hidden), self.critic(hidden)

    def forward(self, obs):
        logits, value = self.logits_value(obs)
        norm = logits - logits.logsumexp(dim=-1, keepdim=True)          # sample_logits, late_fusion.py:30-66
        probs = torch.softmax(norm, dim=-1)
        action = torch.multinomial(probs, 1).squeeze(-1)
        logprob = norm.gather(-1, action.unsqueeze(-1)).squeeze(-1)
        entropy = -(norm * probs).sum(-1)
        return action, logprob, entropy, value


def timed(fn, calls, warm=20):
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls  # microseconds per call


def summary(us):
    return dict(us=us, median=statistics.median(us), lo=min(us), hi=max(us))


def merge(path, stats):
    """Step 2 of the per-kernel split: no device is touched."""
    with open(path) as f:
        res = json.loads(f.readline())
    with open(stats) as f:
        rows = [r for r in csv.DictReader(f) if "k_policy_" in r["Name"]]
    res["kernel_average_us"] = {re.search(r"k_policy_\w+", r["Name"]).group(0): float(r["AverageNs"]) / 1e3 for r in rows}
    res["kernel_sum_us"] = sum(res["kernel_average_us"].values())
    line = json.dumps(res)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4435)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--actions", type=int, default=91)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--dropout", type=float, default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main(args):
    N, A, NA = args.rows, args.agents, args.actions
    D = obs_width(A, EGO)
    res = dict(tool="tools/policy_forward.py", rows=N, slots=A, obs_width=D, actions=NA, runs=args.runs, calls=args.calls,
               observations="synthetic", source_stamp=bench.source_stamp())
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((N, D), device="cuda", generator=g) * 2 - 1
    obs[:, EGO:EGO + 6 * (A - 1)].view(N, A - 1, 6)[:, A - 9:] = 0
    obs[:, EGO + 6 * (A - 1):].view(N, 200, 13)[:, 170:] = 0
    P = args.dropout
    res["dropout"] = P
    net = LateFusion(A, NA, dropout=P or 0.0).cuda()
    net.train(P is not None)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Linear):
                m.weight.normal_(0.0, m.in_features ** -0.5, generator=g)
                m.bias.normal_(0.0, 0.1, generator=g)
    pol = DevicePolicy.from_state_dict(net.state_dict(), max_agents=A, ego_width=EGO,
                                       dropout_rule=None if P is None else DropoutRule(P, 0))
    u = torch.rand(N, device="cuda", generator=g)
    out = pol(obs, u)
    with torch.no_grad():
        logits_a = torch.empty((N, NA), device="cuda")
        pol(obs, u, out=out, logits_out=logits_a)
        if P is None:
            logits_b, _ = net.logits_value(obs)
            res["max_logit_difference"] = float((logits_a - logits_b).abs().max())
        a_us, b_us, a0_us = [], [], []
        for _ in range(args.runs):
            a_us.append(timed(lambda: pol(obs, u, out=out), args.calls))
            if P is not None:
                pol.eval()
                a0_us.append(timed(lambda: pol(obs, u, out=out), args.calls))
                pol.train()
            b_us.append(timed(lambda: net(obs), args.calls))
    res.update(a=summary(a_us), b=summary(b_us))
    if P is not None:
        res["a0"] = summary(a0_us)
        res["a_over_a0"] = res["a"]["median"] / res["a0"]["median"]
    res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
    res["a_outside_b_range_on_the_fast_side"] = res["a"]["hi"] < res["b"]["lo"]
    flop = 2.0 * N * ((A - 1) * (6 * 64 + 64 * 64) + 200 * (13 * 64 + 64 * 64) + EGO * 64 + 64 * 64 + 192 * 128 + 128 * (NA + 1))
    nbytes = 4.0 * N * (D + 2 * 192 + 2 * NA + 1 + 3 + 2) + 4.0 * pol.blob.numel()
    sec = res["a"]["median"] * 1e-6
    res.update(a_flop_per_call=flop, a_TFLOPs=flop / sec / 1e12, a_frac_of_mfma_ceiling=flop / sec / MFMA_CEILING,
               a_bytes_per_call=nbytes, a_GBps=nbytes / sec / 1e9, a_frac_of_copy_ceiling=nbytes / sec / COPY_CEILING)
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
