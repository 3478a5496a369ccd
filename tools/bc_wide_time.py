#!/usr/bin/env python3
"""developer tool: the BC forward at network_dim = 128 against eager torch and against the 64-wide forward.

B = 512, A = 128, R = 5, num_layer (4, 3), head 2, C = 6 (the reference sweep's model), synthetic observations, 40 % padding.
    (a) the wide `DeviceBCPolicy` forward with out= (gd_bc_forward_dim, csrc/bc_policy.hip at T = 4)
    (b) the eager float32 stand-in at 128 on the same GPU, same weights and inputs (tests/bc_cases.StandIn)
    (c) the 64-wide `DeviceBCPolicy` forward at the same layer counts, for scale
Device events around 10 calls after a warm-up of 3, three runs of each in alternation; peak allocated memory of (a) and (b) from
torch's allocator statistics (a fresh peak per side; the inputs and weights are allocated before).  Writes
profiles/bc_wide_forward.json (or argv[1]) and prints it."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpudrive_lab_amd.bc_policy import DeviceBCPolicy, obs_width  # noqa: E402
from tests import bc_cases as BC  # noqa: E402

B, A, R = 512, 128, 5
CFG = BC._cfg((4, 3), 2, 6, -20.0)
WARMUP, CALLS, RUNS = 3, 10, 3


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bc_wide_forward.json")
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.uniform(-1, 1, (B, R, obs_width(A))).astype(np.float32)).cuda()
    pm = torch.from_numpy(rng.random((B, R, A - 1)) < 0.4).cuda()
    rm = torch.from_numpy(rng.random((B, R, 200)) < 0.4).cuda()
    sd_w, sd_n = BC.state_dict(R, CFG, network_dim=128), BC.state_dict(R, CFG, network_dim=64)
    wide = DeviceBCPolicy.from_state_dict(sd_w, max_agents=A, num_stack=R, network_dim=128, **CFG)
    narrow = DeviceBCPolicy.from_state_dict(sd_n, max_agents=A, num_stack=R, **CFG)
    eager = BC.StandIn(sd_w, A, CFG, torch.float32, "cuda")
    out_w, out_n = torch.empty((B, 1, 3), device="cuda"), torch.empty((B, 1, 3), device="cuda")
    sides = {
        "wide_hip": lambda: wide(obs, pm, rm, deterministic=True, out=out_w),
        "wide_eager_torch": lambda: eager.forward(obs, pm, rm),
        "narrow_hip": lambda: narrow(obs, pm, rm, deterministic=True, out=out_n),
    }
    ms = {k: [] for k in sides}
    for _ in range(RUNS):
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    e = eager.forward(obs, pm, rm)
    ctx = wide.context(obs, pm, rm)
    res = dict(B=B, A=A, R=R, cfg=dict(num_layer=list(CFG["num_layer"]), head_num_layers=2, n_components=6), padding=0.4,
               warmup=WARMUP, calls=CALLS, runs=RUNS, device=torch.cuda.get_device_name(0),
               ms_per_call={k: [round(v, 4) for v in vs] for k, vs in ms.items()},
               ms_median={k: round(float(np.median(vs)), 4) for k, vs in ms.items()},
               peak_bytes=dict(wide_hip=peak(sides["wide_hip"]), wide_eager_torch=peak(sides["wide_eager_torch"])),
               wide_policy_nbytes=wide.nbytes(B), narrow_policy_nbytes=narrow.nbytes(B),
               max_abs_context_difference_hip_vs_eager=float((ctx - e["context"]).abs().max()))
    res["eager_over_hip"] = round(res["ms_median"]["wide_eager_torch"] / res["ms_median"]["wide_hip"], 3)
    res["wide_over_narrow"] = round(res["ms_median"]["wide_hip"] / res["ms_median"]["narrow_hip"], 3)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
