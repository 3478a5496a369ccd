#!/usr/bin/env python3
"""developer tool: run the reference's EarlyFusionAttnBCNet on the CPU in float64 with the seeded weights and inputs of
tests/bc_grad_reference.py, call `gmm_loss(net, context, expert)[0].backward()`, and write tests/golden/bc_grad_<B>_<A>_<R>.npz:
per parameter tensor of the module, in its own order, the gradient's sum, its L2 norm and its values at 32 seeded positions
(not whole gradients), and the loss.  Results and names only: the weights and the inputs come from the seeds.
With --dim 128 the same at network_dim 128 (head_dim 64) on bc_wide_cases' `wide_min` and `wide_top` with the inputs of
tests/bc_wide_grad_reference.py: tests/golden/bc_wide_grad_wide_min.npz and bc_wide_grad_wide_top.npz.

    tools/bc_grad_golden.py /path/to/reference/checkout [--dim 128]
    tools/bc_grad_golden.py --seeds        # no reference needed: search the input seeds that keep the margins, print the table

Runs where the reference checkout is; never part of a test run.  The file is float64 autograd's output, whose summation order
depends on the host's CPU and BLAS: bc_wide_grad_wide_min.npz regenerates to 1e-15 relative of the committed file, not to its
bytes, on a host other than the one that wrote it (the tests compare at 1e-12); keep the committed file unless the case changes."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import bc_cases as BC  # noqa: E402
from tests import bc_grad_reference as GR  # noqa: E402
from tests import bc_wide_cases as WC  # noqa: E402
from tests import bc_wide_grad_reference as WGR  # noqa: E402

GOLDEN_CASE = (3, 64, 1)  # samples a, b and c; the smallest of bc_cases.SHAPES
WIDE_GOLDEN_CASES = ("wide_min", "wide_top")  # the same three samples at network_dim 128: the smallest model and the largest
POSITIONS = 32


def positions(name_index, numel):
    return np.random.default_rng([97, name_index]).integers(0, numel, POSITIONS)


def seeds():
    todo = [(B, A, R, BC.CFG) for B, A, R in BC.SHAPES] + [(5, 64, 5, BC.CFG), (8, 64, 5, BC.CFG)]
    todo += [(3, 64, 1, GR.MINIMAL)] + [(B, A, R, cfg) for _, B, A, R, cfg in BC.EDGE_CASES]
    for B, A, R, cfg in todo:
        sd = GR.state_dict(R, cfg)
        for seed in range(1, 400):
            obs, pm, rm, expert, _, _, _ = BC.inputs(B, A, R, seed=seed)
            net = GR.Net(sd, A, cfg)
            with torch.no_grad():
                net.nll(obs, pm, rm, expert[:, 0])
            if min(net.margins.values()) > GR.MARGIN:
                print("    %r: %d,  # margins clamp %.3g relu %.3g" % (GR.case_key(B, A, R, cfg), seed, net.margins["clamp"],
                                                                      net.margins["relu"]))
                break
        else:
            raise SystemExit("no seed keeps the margins for %r" % ((B, A, R),))


def main():
    if sys.argv[1] == "--seeds":
        return seeds()
    from bc_reference_golden import load_reference
    mods = load_reference(sys.argv[1])
    dim = int(sys.argv[sys.argv.index("--dim") + 1]) if "--dim" in sys.argv else 64
    if dim == 128:
        for name in WIDE_GOLDEN_CASES:
            sd, obs, pm, rm, expert, _, A, cfg = WGR.case_inputs(name)
            write(mods, dim, sd, obs, pm, rm, expert, A, WC.lookup(name)[2], cfg, os.path.join(ROOT, "tests", "golden", "bc_wide_grad_%s.npz" % name))
    else:
        B, A, R = GOLDEN_CASE
        sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R)
        write(mods, dim, sd, obs, pm, rm, expert, A, R, BC.CFG, os.path.join(ROOT, "tests", "golden", "bc_grad_%d_%d_%d.npz" % GOLDEN_CASE))


def write(mods, dim, sd, obs, pm, rm, expert, A, R, cfg, path):
    env = types.SimpleNamespace(ego_state=True, partner_obs=True, road_map_obs=True, max_num_agents_in_scene=A, roadgraph_top_k=200)
    exp = types.SimpleNamespace(network_dim=dim, network_num_layers=4, act_func="tanh", dropout=0.0, num_layer=cfg["num_layer"],
                                num_head=4, head_dim=64, head_num_layers=cfg["head_num_layers"], n_components=cfg["n_components"],
                                action_dim=3, clip_value=cfg["clip_value"])
    net = mods["model"].EarlyFusionAttnBCNet(env, exp, num_stack=R).double().train()  # dropout 0.0: train mode is eval mode
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    context, _, _ = net.get_context(torch.from_numpy(obs).double(), [torch.from_numpy(pm), torch.from_numpy(rm)])
    loss, _ = mods["loss"].gmm_loss(net, context, torch.from_numpy(expert).double())
    loss.backward()
    names, sums, norms, at, vals = [], [], [], [], []
    for i, (name, p) in enumerate(net.named_parameters()):
        g = p.grad.numpy().reshape(-1)
        pos = positions(i, g.size)
        names.append(name), sums.append(g.sum()), norms.append(np.sqrt((g * g).sum())), at.append(pos), vals.append(g[pos])
    np.savez_compressed(path, names=np.array(names), sums=np.array(sums), norms=np.array(norms), positions=np.array(at),
                        values=np.array(vals), loss=np.array(float(loss.detach())))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
