#!/usr/bin/env python3
"""One whole PPO minibatch update (forward for the stored actions, loss, backward, gradient clipping, Adam, and the rollout's
policy following the new weights) at the reference's shapes (128 slots, D = 3368, 91 actions), two ways, one JSON line:

  (a) DevicePPO.update: gd_ppo_update, nine launches, nothing in torch;
  (b) TrainablePolicy (gd_policy_evaluate / gd_policy_backward under autograd) + the reference's loss lines in torch on the
      device (tests/ppo_update_reference.ppo_loss) + clip_grad_norm_ + torch.optim.Adam(eps=1e-5) +
      DevicePolicy.load_state_dict, without any .item(): what a caller wrote before `DevicePPO` existed.

Both use the puffer yaml's hyper-parameters.  Observations are synthetic (tools/policy_backward.py's), the old logprobs and
values are the initial policy's own, perturbed by +-0.01, the advantages are N(0, 1).  (a) and (b) alternate in one process,
--runs each: device events around --calls updates after a warm-up of 10.  Reported: the median and the range of the
microseconds per update, and whether (a)'s range lies wholly below (b)'s.  Run it at --rows 8192 (the reference's minibatch)
and at --rows 512, where the launch count dominates.
--dropout P: (a) is DevicePPO(dropout_rule=DropoutRule(P, 0)) (gd_ppo_update_dropout); (b) becomes eager torch -- the plain
torch.nn module in train mode with nn.Dropout(P), the same loss lines, clip_grad_norm_ and Adam; and a third side (a0), a
DevicePPO without the rule (the same build without the masks), joins the alternation.  The parameters are then not compared.
tools/ppo_update.py [--rows 8192] [--agents 128] [--actions 91] [--partials 256] [--runs 3] [--calls 50] [--dropout P]
                    [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from torch import nn  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.dropout import DropoutRule  # noqa: E402
from gpudrive_lab_amd.policy import DevicePolicy, TrainablePolicy, obs_width  # noqa: E402
from gpudrive_lab_amd.ppo import DevicePPO  # noqa: E402
from policy_backward import EGO, LateFusion, summary, timed  # noqa: E402
from tests.ppo_update_reference import ppo_loss  # noqa: E402

YAML = dict(clip_coef=0.2, vf_clip_coef=0.2, ent_coef=1e-4, vf_coef=0.3, norm_adv=True, clip_vloss=False)
LR, BETAS, EPS, MAX_NORM = 3e-4, (0.9, 0.999), 1e-5, 0.5


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--actions", type=int, default=91)
    ap.add_argument("--partials", type=int, default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--dropout", type=float, default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main(args):
    N, A, NA = args.rows, args.agents, args.actions
    D = obs_width(A, EGO)
    res = dict(tool="tools/ppo_update.py", rows=N, slots=A, obs_width=D, actions=NA, runs=args.runs, calls=args.calls,
               observations="synthetic", source_stamp=bench.source_stamp())
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((N, D), device="cuda", generator=g) * 2 - 1
    obs[:, EGO:EGO + 6 * (A - 1)].view(N, A - 1, 6)[:, A - 9:] = 0
    obs[:, EGO + 6 * (A - 1):].view(N, 200, 13)[:, 170:] = 0
    P = args.dropout
    res["dropout"] = P
    net = LateFusion(A, NA, dropout=P or 0.0).cuda()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Linear):
                m.weight.normal_(0.0, m.in_features ** -0.5, generator=g)
                m.bias.normal_(0.0, 0.1, generator=g)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    ppo = DevicePPO(sd, max_agents=A, ego_width=EGO, minibatch_size=N, learning_rate=LR, betas=BETAS, eps=EPS,
                    max_grad_norm=MAX_NORM, partials=args.partials, dropout_rule=None if P is None else DropoutRule(P, 0), **YAML)
    ppo0 = None if P is None else DevicePPO(sd, max_agents=A, ego_width=EGO, minibatch_size=N, learning_rate=LR, betas=BETAS,
                                            eps=EPS, max_grad_norm=MAX_NORM, partials=args.partials, **YAML)
    res["partials"], res["a_nbytes"] = ppo.partials, ppo.nbytes
    action, logprob, _, value = ppo.policy(obs, torch.rand(N, device="cuda", generator=g))
    sign = (torch.arange(N, device="cuda") % 2).float() * 2 - 1
    old_lp, old_v = logprob + 0.01 * sign, value - 0.01 * sign
    adv = torch.randn(N, device="cuda", generator=g)
    ret = old_v + adv

    tp = TrainablePolicy.from_state_dict(sd, max_agents=A, ego_width=EGO, device="cuda", partials=args.partials)
    pol = DevicePolicy.from_state_dict(sd, max_agents=A, ego_width=EGO)
    opt = torch.optim.Adam((tp if P is None else net).parameters(), lr=LR, betas=BETAS, eps=EPS)
    hyper = {k: v for k, v in YAML.items()}

    def a():
        ppo.update(obs, action, old_lp, old_v, adv, ret)

    def a0():
        ppo0.update(obs, action, old_lp, old_v, adv, ret)

    def b_eager():
        _, newlogprob, entropy, newvalue = net(obs, action)
        loss, _ = ppo_loss(newlogprob, entropy, newvalue, old_lp, adv, ret, old_v, **hyper)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)
        opt.step()

    def b():
        if P is not None:
            return b_eager()
        _, newlogprob, entropy, newvalue = tp(obs, action)
        loss, _ = ppo_loss(newlogprob, entropy, newvalue, old_lp, adv, ret, old_v, **hyper)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(tp.parameters(), MAX_NORM)
        opt.step()
        pol.load_state_dict(tp.state_dict())

    a(), b()
    torch.cuda.synchronize()
    if P is None:
        flat = torch.cat([p.detach().reshape(-1) for p in tp.parameters()])
        res["max_parameter_difference_after_one_update"] = float((ppo.flat[:-1] - flat).abs().max())
    a_us, b_us, a0_us = [], [], []
    for _ in range(args.runs):
        a_us.append(timed(a, args.calls))
        if P is not None:
            a0_us.append(timed(a0, args.calls))
        b_us.append(timed(b, args.calls))
    res.update(a=summary(a_us), b=summary(b_us))
    if P is not None:
        res["a0"] = summary(a0_us)
        res["a_over_a0"] = res["a"]["median"] / res["a0"]["median"]
    res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
    res["a_range_wholly_below_b"] = res["a"]["hi"] < res["b"]["lo"]
    res["a_losses"] = ppo.losses()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):
        main(arguments())
