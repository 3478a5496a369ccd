"""The reference of the device BC update at network_dim 128 (gpudrive_lab_amd.bc_opt.DeviceBCDim; gd_bc_adamw_dim,
gd_bc_update_dim): tests/bc_update_reference.py's step -- `clip_grad_norm_(.., 20)`, the restated `get_grad_norm`,
`torch.optim.AdamW(foreach=False)`, the rule's host program -- on the 128-wide layout, and the whole step of the differentiable
restatement at that width (tests/bc_wide_grad_reference.py).  Nothing of the rule depends on the width: what is new here is the
layout (more and larger tensors) and the structs of the junk-pointer tests.  Test infrastructure for test_bc_wide_update.py and
test_gpu_bc_wide_update.py."""
import numpy as np
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from gpudrive_lab_amd import bc_train as BT

from . import bc_update_reference as UR
from . import bc_wide_cases as WC
from . import bc_wide_grad_reference as WGR

DIM = WC.DIM
ADAMW = UR.ADAMW
LARGEST = "head.input_layer.0.weight"  # 64 x 3 network_dim: the largest tensor at either width
SWEEP_G, SWEEP_T = 1399274, 252        # the reference sweep's model: network_dim 128, num_layer (4, 3), R = 5, 6 components


def layout_args(R, cfg):
    return R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"]


def layout(name, network_dim=DIM):
    """(names, tensor_end int32 [T], G) of the flat layout of the case `name` of bc_wide_cases at network_dim."""
    _, _, R, cfg = WC.lookup(name)
    shapes = WC.shapes(R, cfg, network_dim)
    end = np.cumsum([int(np.prod(s)) for s in shapes.values()]).astype(np.int32)
    return tuple(shapes), end, int(end[-1])


_PLANTED = {}


def planted_gradients(name):
    """bc_update_reference.gradients on the case's 128-wide layout with the largest tensor planted as the tensor of the largest
    norm (its values doubled) and one whole 64 x 64 tensor of zeros: (gradients, zero tensor, largest tensor).  Computed once
    and shared: leave it unchanged."""
    if name not in _PLANTED:
        names, end, _ = layout(name)
        largest = names.index(LARGEST)
        sizes = np.diff(np.concatenate([[0], end]))
        assert sizes[largest] == sizes.max() == 64 * 3 * DIM
        zt = UR.zero_tensor(end)
        _PLANTED[name] = (UR.gradients(end, largest=largest), zt, largest)
    return _PLANTED[name]


def flat_params(sd, names):
    return np.concatenate([sd[k].numpy().reshape(-1) for k in names])


def pipeline(c, dtype=torch.float64, steps=1, **adamw):
    """bc_update_reference.pipeline on the wide restatement: the reference's whole step on the CPU in `dtype` on the case c of
    bc_wide_grad_reference.case.  Returns (parameters after the last step by name as float64 numpy, the loss of every step)."""
    ad = dict(ADAMW, **adamw)
    net = WGR.Net(c["sd"], c["A"], c["cfg"], dtype)
    params = list(net.params.values())
    opt = torch.optim.AdamW(params, lr=ad["lr"], betas=ad["betas"], eps=ad["eps"], weight_decay=ad["weight_decay"], foreach=False)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = net.nll(c["obs"], c["pm"], c["rm"], c["expert"]).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, ad["max_norm"], foreach=False)
        opt.step()
        losses.append(float(loss.detach()))
    return {k: v.detach().double().numpy() for k, v in net.params.items()}, losses


_SIZES = {}
OK = 0x1000  # a junk pointer that passes every alignment check and is never read


def structs(dim, name="wide_sweep", max_rows=8, chunk=2, **kw):
    """(gd_bc_policy_dim, gd_bc_grad, gd_bc_opt) of the case's configuration at width dim with junk pointers: everything the
    checks of gd_bc_update_dim and gd_bc_adamw_dim read, in order.  kw: fields of the gd_bc_opt to overwrite."""
    _, A, R, cfg = WC.lookup(name)
    if (dim, name) not in _SIZES:
        lay = layout_args(R, cfg)
        _SIZES[dim, name] = BT.grad_floats(*lay, network_dim=dim), int(BP.pack_index(*lay, network_dim=dim).size)
    G, blob = _SIZES[dim, name]
    pd, g, o = _capi.GdBCPolicyDim(), _capi.GdBCGrad(), _capi.GdBCOpt()
    pd.network_dim, pd.reserved = dim, 0
    p = pd.base
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers = A, R, *cfg["num_layer"]
    p.head_layers, p.n_components, p.clip_value, p.chunk_rows = cfg["head_num_layers"], cfg["n_components"], cfg["clip_value"], chunk
    p.blob, p.blob_floats, p.scratch, p.scratch_floats = OK, blob, OK, BP.scratch_floats(A, chunk, dim)
    g.scratch, g.scratch_floats = OK, BT.grad_scratch_floats(A, chunk, cfg["num_layer"], blob, network_dim=dim)
    g.partials, g.grad_floats, g.num_partials = OK, G, 4
    o.max_grad_norm, o.eps, o.weight_decay, o.stats_scale, o.beta1, o.beta2 = 20.0, 1e-4, 0.01, 1.0, 0.9, 0.999
    o.grad_floats, o.blob_floats = G, blob
    o.num_stack, o.fusion_layers, o.branch_layers = R, *cfg["num_layer"]
    o.head_layers, o.n_components, o.max_rows = cfg["head_num_layers"], cfg["n_components"], max_rows
    o.num_tensors = len(WC.shapes(R, cfg, dim))
    for field, _ in _capi.GdBCOpt._fields_[16:]:
        setattr(o, field, OK)
    for k, v in kw.items():
        setattr(o, k, v)
    return pd, g, o
