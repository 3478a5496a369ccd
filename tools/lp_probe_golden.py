#!/usr/bin/env python3
"""developer tool: run the reference's EarlyFusionAttnBCNet and LinearProbPosition on the CPU in float64 with the seeded
weights, inputs, head and labels of tests/bc_cases.py and tests/probe_cases.py, and write
tests/golden/lp_probe_<B>_<A>_<R>.npz: what a linear probe reads and computes -- the last_hidden_state of `fusion_attn` and
`ro_attn` (tokens 0 .. A - 1), the head's logits on both for 'other' and 'ego', and LinearProbPosition.loss's loss and
accuracy on the rows the seeded masks select.  Outputs and names only: weights, inputs and labels come from the seeds.

    tools/lp_probe_golden.py /path/to/reference/checkout

The hidden states are taken by forward hooks this tool puts on `net.fusion_attn` and `net.ro_attn` themselves.  It also
registers hooks on all their descendants in the order baselines/il/linear_probing.py:77-95 does and asserts that the LAST
entry of that ordered dict -- what the reference reads as `layers[nth_layer]` -- is that same tensor."""
import importlib.util
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import bc_cases as BC  # noqa: E402
from tests import probe_cases as PC  # noqa: E402
import bc_reference_golden as BG  # noqa: E402
import types  # noqa: E402


def load_probe(ref):
    path = os.path.join(ref, "gpudrive", "integrations", "il", "linear_probing", "lp_model.py")
    spec = importlib.util.spec_from_file_location("lp_model_isolated", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hook_block(block):
    """(the block's own output holder, the ordered dict of its descendants' outputs keyed as the reference keys them)."""
    own, layers = {}, OrderedDict()

    def value(output):
        return (output if isinstance(output, torch.Tensor) else output["last_hidden_state"]).detach()

    block.register_forward_hook(lambda m, i, o: own.__setitem__("out", value(o)))

    def register(module, prefix=""):
        for name, layer in module.named_children():
            full = "%s.%s" % (prefix, name) if prefix else name
            layer.register_forward_hook(lambda m, i, o, full=full: layers.__setitem__(full, value(o)))
            register(layer, full)

    register(block)
    return own, layers


def main():
    ref = sys.argv[1]
    mods = BG.load_reference(ref)
    lp = load_probe(ref)
    cfg = BC.CFG
    for B, A, R in PC.GOLDEN_SHAPES:
        env = types.SimpleNamespace(ego_state=True, partner_obs=True, road_map_obs=True, max_num_agents_in_scene=A, roadgraph_top_k=200)
        exp_cfg = types.SimpleNamespace(network_dim=64, network_num_layers=4, act_func="tanh", dropout=0.0, num_layer=cfg["num_layer"],
                                        num_head=4, head_dim=64, head_num_layers=cfg["head_num_layers"],
                                        n_components=cfg["n_components"], action_dim=3, clip_value=cfg["clip_value"])
        net = mods["model"].EarlyFusionAttnBCNet(env, exp_cfg, num_stack=R).double().eval()
        net.load_state_dict({k: v.double() for k, v in BC.state_dict(R, cfg).items()})
        hooks = {"fusion_attn": hook_block(net.fusion_attn), "ro_attn": hook_block(net.ro_attn)}
        obs, pm, rm = BC.inputs(B, A, R)[:3]
        with torch.no_grad():
            net.get_context(torch.from_numpy(obs).double(), [torch.from_numpy(pm), torch.from_numpy(rm)])
        probe = lp.LinearProbPosition(64, 64).double()
        probe.load_state_dict({k: v.double() for k, v in PC.head(64).items()})
        out = {"names": np.array(list(probe.state_dict().keys()))}
        for tap, (own, layers) in hooks.items():
            last = list(layers.keys())[-1]
            assert torch.equal(layers[last], own["out"]), (tap, last)  # layers[nth_layer] IS the block's last_hidden_state
            hidden = own["out"]
            out[tap] = hidden[:, :A].numpy()
            out[tap + "_last_hook"] = np.array(last)
            for exp in PC.EXPS:
                x = hidden[:, 0, :] if exp == "ego" else hidden[:, 1:A, :]
                mask, lab = PC.labels(B, A, exp)
                with torch.no_grad():
                    z = probe(x)
                    sel = ~torch.from_numpy(mask) if exp == "other" else torch.from_numpy(mask)
                    loss, acc, _ = probe.loss(z[sel], torch.from_numpy(lab)[sel])
                out["%s_%s_logits" % (tap, exp)] = z.numpy()
                out["%s_%s_loss" % (tap, exp)] = np.array([float(loss), float(acc)])
        path = os.path.join(ROOT, "tests", "golden", "lp_probe_%d_%d_%d.npz" % (B, A, R))
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
