#!/usr/bin/env python3
"""The policy's training step on one minibatch at the reference's size (N = 8192 rows, 128 slots, D = 3368, 91 actions) --
the forward for given actions plus the backward to parameter gradients -- two ways, one JSON line:

  (a) TrainablePolicy: gd_policy_evaluate and gd_policy_backward (three launches each, plus torch's re-pack of the blob);
  (b) the late-fusion module out of plain torch.nn layers under the reference's key names, dropout 0, its eager float32
      forward (log_softmax, gather, the entropy sum) and autograd backward, on the same device.

Both backpropagate the same three upstream gradients (seeded, size 1 / N) into `.grad` tensors that exist already; the loss
arithmetic, clipping and the optimiser are the caller's torch code either way and are not timed.  Observations are synthetic:
uniform in [-1, 1] with a padding tail of zero rows in each set.  The weights are N(0, 1 / fan_in).  (a) and (b) alternate in
one process, --runs each: device events around --calls calls after a warm-up of 10.  Reported: the median and the range of
the microseconds per call, the rise of torch's peak allocated memory over one call of each, and the largest relative
difference between (a)'s and (b)'s gradients per tensor (the two pool at their own float32 winners).
The per-kernel split takes two more steps, the second without a device:
  1. rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/policy_backward.py --runs 1 --calls 20 --only a
  2. tools/policy_backward.py --merge FILE --kernel-stats DIR/.../*_kernel_stats.csv
     adds `kernel_average_us` (the AverageNs column of the k_policy_* and k_pg_* rows) to the JSON line in FILE.
--dropout P: (a) runs in train mode with dropout_rule=DropoutRule(P, 0) (gd_policy_evaluate_dropout and
gd_policy_backward_dropout), (b) in train mode with nn.Dropout(P), and a third side (a0), the same TrainablePolicy in eval
mode (the same build without the masks), joins the alternation; the gradients of (a) and (b) are then not compared.
tools/policy_backward.py [--rows 8192] [--agents 128] [--actions 91] [--partials 256] [--runs 3] [--calls 50] [--dropout P]
                         [--out FILE]"""
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
from gpudrive_lab_amd.policy import TrainablePolicy, obs_width  # noqa: E402

EGO = 6


class LateFusion(nn.Module):
    def __init__(self, agents, actions, dropout=0.0):
        super().__init__()
        self.agents = agents

        def embed(k):
            return nn.Sequential(nn.Linear(k, 64), nn.LayerNorm(64), nn.Tanh(), nn.Dropout(dropout), nn.Linear(64, 64))

        self.ego_embed, self.partner_embed, self.road_map_embed = embed(EGO), embed(6), embed(13)
        self.shared_embed = nn.Sequential(nn.Linear(192, 128), nn.Dropout(dropout))
        self.actor, self.critic = nn.Linear(128, actions), nn.Linear(128, 1)

    def forward(self, obs, action):
        n, r0 = obs.shape[0], EGO + 6 * (self.agents - 1)
        ego = self.ego_embed(obs[:, :EGO])
        partner, _ = self.partner_embed(obs[:, EGO:r0].view(n, self.agents - 1, 6)).max(dim=1)
        road, _ = self.road_map_embed(obs[:, r0:].view(n, 200, 13)).max(dim=1)
        hidden = self.shared_embed(torch.cat([ego, partner, road], dim=1))
        logits, value = self.actor(hidden), self.critic(hidden)
        norm = torch.log_softmax(logits, dim=-1)
        logprob = norm.gather(-1, action.unsqueeze(-1)).squeeze(-1)
        entropy = -(norm * norm.exp()).sum(-1)
        return action, logprob, entropy, value.squeeze(-1)


def timed(fn, calls, warm=10):
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls  # microseconds per call


def peak_rise(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def summary(us):
    return dict(us=us, median=statistics.median(us), lo=min(us), hi=max(us))


def merge(path, stats):
    """Step 2 of the per-kernel split: no device is touched."""
    with open(path) as f:
        res = json.loads(f.readline())
    with open(stats) as f:
        rows = [r for r in csv.DictReader(f) if re.search(r"k_policy_|k_pg_", r["Name"])]
    res["kernel_average_us"] = {re.search(r"k_(policy|pg)_\w+(<[\w, ]+>)?", r["Name"]).group(0): float(r["AverageNs"]) / 1e3 for r in rows}
    res["kernel_sum_us"] = sum(res["kernel_average_us"].values())
    line = json.dumps(res)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--actions", type=int, default=91)
    ap.add_argument("--partials", type=int, default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--dropout", type=float, default=None)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main(args):
    N, A, NA = args.rows, args.agents, args.actions
    D = obs_width(A, EGO)
    res = dict(tool="tools/policy_backward.py", rows=N, slots=A, obs_width=D, actions=NA, runs=args.runs, calls=args.calls,
               observations="synthetic", source_stamp=bench.source_stamp())
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((N, D), device="cuda", generator=g) * 2 - 1
    obs[:, EGO:EGO + 6 * (A - 1)].view(N, A - 1, 6)[:, A - 9:] = 0
    obs[:, EGO + 6 * (A - 1):].view(N, 200, 13)[:, 170:] = 0
    action = torch.randint(0, NA, (N,), device="cuda", generator=g)
    ups = [torch.randn(N, device="cuda", generator=g) / N for _ in range(3)]
    P = args.dropout
    res["dropout"] = P
    net = LateFusion(A, NA, dropout=P or 0.0).cuda()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Linear):
                m.weight.normal_(0.0, m.in_features ** -0.5, generator=g)
                m.bias.normal_(0.0, 0.1, generator=g)
    tp = TrainablePolicy.from_state_dict(net.state_dict(), max_agents=A, ego_width=EGO, device="cuda", partials=args.partials,
                                         dropout_rule=None if P is None else DropoutRule(P, 0))
    res["partials"] = tp.partials

    def step(mod):
        def fn():
            for p in mod.parameters():
                p.grad.zero_()
            _, logprob, entropy, value = mod(obs, action)
            torch.autograd.backward([logprob, entropy, value], ups)
        return fn

    for mod in (tp, net):
        for p in mod.parameters():
            p.grad = torch.zeros_like(p)
    a, b = step(tp), step(net)
    if args.only != "b":
        a()
    if args.only != "a":
        b()
    if args.only is None and P is None:
        res["max_relative_gradient_difference"] = {
            k: float((p.grad - q.grad).abs().max() / q.grad.abs().max())
            for (k, p), (_, q) in zip(tp.named_parameters(), net.named_parameters())}
    a_us, b_us, a0_us = [], [], []
    for _ in range(args.runs):
        if args.only != "b":
            a_us.append(timed(a, args.calls))
            if P is not None:
                tp.eval()
                a0_us.append(timed(a, args.calls))
                tp.train()
        if args.only != "a":
            b_us.append(timed(b, args.calls))
    if a_us:
        res.update(a=summary(a_us), a_peak_bytes=peak_rise(a), a_nbytes=tp.nbytes(N))
    if a0_us:
        res["a0"] = summary(a0_us)
        res["a_over_a0"] = res["a"]["median"] / res["a0"]["median"]
    if b_us:
        res.update(b=summary(b_us), b_peak_bytes=peak_rise(b))
    if a_us and b_us:
        res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
        res["a_outside_b_range_on_the_fast_side"] = res["a"]["hi"] < res["b"]["lo"]
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
