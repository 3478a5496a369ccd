#!/usr/bin/env python3
"""One linear-probing step and one evaluation batch at lp.yaml's sizes (B = 256 samples, 128 slots, num_stack 5, num_layer
(3, 2)), for exp 'other' and 'ego', two ways on the same GPU, one JSON line:

  (a) DeviceLinearProbe.update: one C call (gd_lp_update: the tap's launches, the row kernel per chunk, the reduction, AdamW);
      and one batch of DeviceLinearProbe.evaluate (gd_lp_eval_accumulate);
  (b) the eager composition the reference runs: bc_cases.StandIn's layers on the GPU up to the tap (float32, no_grad),
      nn.Linear(64, 64), CrossEntropyLoss on the selected rows, AdamW(lr, eps=1e-4).step(), then the predictions and labels
      copied to the host and the macro F1 there, per step, as baselines/il/linear_probing.py:218-232 does.

Also timed: DeviceBCPolicy.hidden(tap='fusion_attn') and (tap='ro_attn') against the full DeviceBCPolicy.forward (actions): what
stopping at the tap saves.  `update - hidden` is an upper estimate of what the probe's own kernels cost in a step (hidden
includes its copy launch).  Inputs are tools/bc_forward.py's: synthetic observations uniform in [-1, 1], masks 40 % padding;
labels uniform over the 64 classes, half the rows selected.  (a) and (b) alternate in one process, --runs each: device events
around --calls steps after a warm-up.  Reported: the median and the range of the microseconds per call, the launches per step
(from the launch sequence: per chunk 1 + 2 per self layer + 1 row launch, then 3), the bytes either side allocates during a
step and what the probe holds in all (nbytes).
tools/lp_probe.py [--rows 256] [--agents 128] [--stack 5] [--runs 3] [--calls 10] [--model early_lp] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from bc_forward import peak_bytes, summary, timed  # noqa: E402
from gpudrive_lab_amd import DeviceLinearProbe  # noqa: E402
from gpudrive_lab_amd.bc_policy import DeviceBCPolicy, obs_width  # noqa: E402
from gpudrive_lab_amd.lp_probe import macro_f1  # noqa: E402
from tests import bc_cases as BC  # noqa: E402
from tests import probe_cases as PC  # noqa: E402


def eager_tap(s, obs, pm, rm, A, tap):
    """bc_cases.StandIn's layers up to the tap, on its device: [B, A, 64]."""
    cfg = s.cfg
    B, R, _ = obs.shape
    pmt, rmt = pm[:, -1], rm[:, -1]
    ego = obs[..., :6].reshape(B, R * 6)
    ro = obs[..., 6:6 + 6 * (A - 1)].view(B, R, A - 1, 6).permute(0, 2, 1, 3).reshape(B, A - 1, R * 6)
    rg = obs[..., 6 + 6 * (A - 1):].view(B, R, 200, 13).permute(0, 2, 1, 3).reshape(B, 200, R * 13)
    x = torch.cat([s._embed(ego, "ego_state_net").unsqueeze(1), s._embed(ro, "road_object_net"), s._embed(rg, "road_graph_net")], 1)
    ego_mask = torch.zeros(B, 1, dtype=torch.bool, device=obs.device)
    all_mask, obj_mask = torch.cat([ego_mask, pmt, rmt], -1), torch.cat([ego_mask, pmt], -1)
    for i in range(cfg["num_layer"][0]):
        x = s._self(x, all_mask, "fusion_attn.%d" % i)
    objs = x[:, :A]
    if tap == "ro_attn":
        for i in range(cfg["num_layer"][1]):
            objs = s._self(objs, obj_mask, "ro_attn.%d" % i)
    return objs


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--stack", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--model", choices=("early_lp", "late_lp"), default="early_lp")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main(args):
    B, A, R, cfg = args.rows, args.agents, args.stack, BC.CFG
    sd = BC.state_dict(R, cfg)
    bc = DeviceBCPolicy.from_state_dict(sd, max_agents=A, num_stack=R, **cfg)
    tap = PC.TAP_OF[args.model]
    layers = cfg["num_layer"][0] + (cfg["num_layer"][1] if tap == "ro_attn" else 0)
    chunks = -(-B // bc.chunk_rows)
    res = dict(tool="tools/lp_probe.py", rows=B, slots=A, num_stack=R, obs_width=obs_width(A), config=cfg, model=args.model, runs=args.runs,
               calls=args.calls, observations="synthetic", source_stamp=bench.source_stamp(), chunk_rows=bc.chunk_rows,
               launches_per_update=1 + chunks * (1 + 2 * layers + 1) + 2, launches_per_eval_batch=1 + chunks * (1 + 2 * layers + 1) + 1,
               launches_full_forward=chunks * (2 * sum(cfg["num_layer"]) + 3))
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.rand((B, R, obs_width(A)), device="cuda", generator=g) * 2 - 1
    pm = torch.rand((B, R, A - 1), device="cuda", generator=g) < 0.4
    rm = torch.rand((B, R, 200), device="cuda", generator=g) < 0.4
    hidden_out = torch.empty((B, A, 64), device="cuda")
    actions = {"actions": torch.empty((B, 1, 3), device="cuda")}
    fwd = dict(full_forward=lambda: bc.forward(obs, pm, rm, ("actions",), out=actions),
               hidden_fusion=lambda: bc.hidden(obs, pm, rm, tap="fusion_attn", out=hidden_out),
               hidden_ro=lambda: bc.hidden(obs, pm, rm, tap="ro_attn", out=hidden_out))
    for f in fwd.values():
        f()
    us = {k: [] for k in fwd}
    for _ in range(args.runs):
        for k, f in fwd.items():
            us[k].append(timed(f, args.calls))
    res.update({k: summary(v) for k, v in us.items()})
    stand = BC.StandIn(sd, A, cfg, torch.float32, "cuda")
    for exp in PC.EXPS:
        shape = (B, A - 1) if exp == "other" else (B,)
        use = torch.rand(shape, device="cuda", generator=g) < 0.5
        mask = ~use if exp == "other" else use
        labels = torch.randint(0, 64, shape, device="cuda", generator=g)
        hd = PC.head(64)
        probe = DeviceLinearProbe(bc, hd, model=args.model, exp=exp)
        batch = (obs, None, None, None, pm, rm, mask, labels)
        lin = torch.nn.Linear(64, 64).cuda()
        lin.load_state_dict({"weight": hd["head.weight"], "bias": hd["head.bias"]})
        opt = torch.optim.AdamW(lin.parameters(), lr=probe.lr, eps=probe.eps)
        crit = torch.nn.CrossEntropyLoss()

        def step_a():
            probe.update(*batch)

        def eval_a():
            probe.evaluate([batch])

        def step_b():
            with torch.no_grad():
                h = eager_tap(stand, obs, pm, rm, A, tap)
            x = h[:, 0] if exp == "ego" else h[:, 1:A]
            z = lin(x)[use]
            y = labels[use]
            loss = crit(z, y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            p, t = z.argmax(-1).cpu().numpy(), y.cpu().numpy()
            return macro_f1(np.bincount(t[p == t], minlength=64), np.bincount(p, minlength=64), np.bincount(t, minlength=64)), loss.item()

        step_a(), eval_a(), step_b()
        a_us, e_us, b_us = [], [], []
        for _ in range(args.runs):
            a_us.append(timed(step_a, args.calls))
            e_us.append(timed(eval_a, args.calls))
            b_us.append(timed(step_b, args.calls))
        r = dict(update=summary(a_us), eval_batch=summary(e_us), eager=summary(b_us), probe_nbytes=probe.nbytes,
                 update_peak_bytes=peak_bytes(step_a), eager_peak_bytes=peak_bytes(step_b))
        r["eager_over_update"] = r["eager"]["median"] / r["update"]["median"]
        r["update_minus_hidden_us"] = r["update"]["median"] - res["hidden_fusion" if tap == "fusion_attn" else "hidden_ro"]["median"]
        r["last_losses"] = probe.losses()
        res[exp] = r
    res["hidden_fusion_over_full_forward"] = res["hidden_fusion"]["median"] / res["full_forward"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):
        main(arguments())
