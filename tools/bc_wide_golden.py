#!/usr/bin/env python3
"""developer tool: run the reference's EarlyFusionAttnBCNet on the CPU in float64 at network_dim = 128, head_dim = 64 with the
seeded weights and inputs of tests/bc_wide_cases.py and write tests/golden/bc_wide_forward_<name>.npz for the three cases that
are not about chunks: the module's parameter names and shapes, and its context, means, covariances, weights, deterministic
action, ego_attn_score and gmm_loss's per-row value.  Outputs and names only: the weights and the inputs come from the seeds.

    tools/bc_wide_golden.py /path/to/reference/checkout

The reference's modules are loaded in isolation as tools/bc_reference_golden.py loads them."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bc_reference_golden import load_reference  # noqa: E402
from tests import bc_cases as BC  # noqa: E402
from tests import bc_wide_cases as WC  # noqa: E402


def main():
    mods = load_reference(sys.argv[1])
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name in WC.GOLDEN_CASES:
        B, A, R, cfg = WC.CASES[name]
        env = types.SimpleNamespace(ego_state=True, partner_obs=True, road_map_obs=True, max_num_agents_in_scene=A,
                                    roadgraph_top_k=200)
        exp = types.SimpleNamespace(network_dim=WC.DIM, network_num_layers=4, act_func="tanh", dropout=0.0,
                                    num_layer=cfg["num_layer"], num_head=4, head_dim=64, head_num_layers=cfg["head_num_layers"],
                                    n_components=cfg["n_components"], action_dim=3, clip_value=cfg["clip_value"])
        net = mods["model"].EarlyFusionAttnBCNet(env, exp, num_stack=R).double().eval()
        names = list(net.state_dict().keys())
        shapes = [tuple(v.shape) for v in net.state_dict().values()]
        net.load_state_dict({k: v.double() for k, v in WC.state_dict(R, cfg).items()})
        obs, pm, rm, expert, _, _, _ = BC.inputs(B, A, R)
        with torch.no_grad():
            t_obs, t_exp = torch.from_numpy(obs).double(), torch.from_numpy(expert).double()
            context, score, _ = net.get_context(t_obs, [torch.from_numpy(pm), torch.from_numpy(rm)])
            means, cov, weights, _ = net.head.get_gmm_params(context)
            action = net.get_action(context, deterministic=True)
            _, nll = mods["loss"].gmm_loss(net, context, t_exp)
        path = os.path.join(out_dir, "bc_wide_forward_%s.npz" % name)
        np.savez_compressed(path, names=np.array(names), shapes=np.array([",".join(map(str, s)) for s in shapes]),
                            context=context.numpy(), means=means.numpy(), covariances=cov.numpy(), weights=weights.numpy(),
                            action=action.numpy(), ego_attn_score=score.numpy(), nll=nll.numpy())
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
