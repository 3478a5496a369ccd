#!/usr/bin/env python3
"""developer tool: run the reference's EarlyFusionAttnBCNet on the CPU in float64 with the seeded weights and inputs of
tests/bc_cases.py (network_dim 64) and of the cases of tests/bc_wide_cases.py that are not about chunks, with `wide_top` of its
edge configurations (network_dim 128, head_dim 64) and write tests/golden/bc_forward_<B>_<A>_<R>.npz and bc_wide_forward_<name>.npz: the module's parameter names and
shapes, and its context, means, covariances, weights, deterministic action, ego_attn_score and gmm_loss's per-row value.
Outputs and names only: the weights and the inputs come from the seeds.

    tools/bc_reference_golden.py /path/to/reference/checkout [output directory, default tests/golden]

The reference's `gpudrive` package needs a built simulator to import, so networks.py, model.py, constants.py and loss.py are
loaded in isolation under their own module names; any attribute object serves as their config."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bc_cases as BC  # noqa: E402
from tests import bc_wide_cases as WC  # noqa: E402


def load_reference(ref):
    il = os.path.join(ref, "gpudrive", "integrations", "il")
    for pkg in ("gpudrive", "gpudrive.integrations", "gpudrive.integrations.il", "gpudrive.integrations.il.model"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    mods = {}
    for name, path in (("gpudrive.integrations.il.constants", "constants.py"),
                       ("gpudrive.integrations.il.model.networks", os.path.join("model", "networks.py")),
                       ("gpudrive.integrations.il.model.model", os.path.join("model", "model.py")),
                       ("gpudrive.integrations.il.loss", "loss.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(il, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        setattr(sys.modules[parent], leaf, mod)
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods


def main():
    mods = load_reference(sys.argv[1])
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden")
    cases = [("bc_forward_%d_%d_%d.npz" % (B, A, R), B, A, R, BC.CFG, 64, 1) for B, A, R in BC.SHAPES]
    cases += [("bc_wide_forward_%s.npz" % name, *WC.lookup(name), WC.DIM, WC.SEEDS[name]) for name in WC.GOLDEN_CASES + WC.EDGE_GOLDEN_CASES]
    for fname, B, A, R, cfg, dim, seed in cases:
        env = types.SimpleNamespace(ego_state=True, partner_obs=True, road_map_obs=True, max_num_agents_in_scene=A,
                                    roadgraph_top_k=200)
        exp = types.SimpleNamespace(network_dim=dim, network_num_layers=4, act_func="tanh", dropout=0.0, num_layer=cfg["num_layer"],
                                    num_head=4, head_dim=64, head_num_layers=cfg["head_num_layers"],
                                    n_components=cfg["n_components"], action_dim=3, clip_value=cfg["clip_value"])
        net = mods["model"].EarlyFusionAttnBCNet(env, exp, num_stack=R).double().eval()
        names = list(net.state_dict().keys())
        shapes = [tuple(v.shape) for v in net.state_dict().values()]
        net.load_state_dict({k: v.double() for k, v in BC.state_dict(R, cfg, network_dim=dim).items()})
        obs, pm, rm, expert, _, _, _ = BC.inputs(B, A, R, seed=seed)
        with torch.no_grad():
            t_obs, t_exp = torch.from_numpy(obs).double(), torch.from_numpy(expert).double()
            context, score, _ = net.get_context(t_obs, [torch.from_numpy(pm), torch.from_numpy(rm)])
            means, cov, weights, _ = net.head.get_gmm_params(context)
            action = net.get_action(context, deterministic=True)
            _, nll = mods["loss"].gmm_loss(net, context, t_exp)
        path = os.path.join(out_dir, fname)
        np.savez_compressed(path, names=np.array(names), shapes=np.array([",".join(map(str, s)) for s in shapes]),
                            context=context.numpy(), means=means.numpy(), covariances=cov.numpy(), weights=weights.numpy(),
                            action=action.numpy(), ego_attn_score=score.numpy(), nll=nll.numpy())
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
