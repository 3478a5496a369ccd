"""The BC policy's training loss written differentiably at the state dict's width: bc_grad_reference.Net with the two places
that carry a width restated -- the LayerNorm (over as many features as its gain has) and the attention (4 heads of D / 4
channels, q scaled by (D / 4)^-1/2).  On a 64-wide state dict it is bc_grad_reference.Net; at 128 its nll is
tests/bc_reference.py's (tests/test_bc_wide_grad.py pins both), and its float64 autograd is what the device backward at
network_dim 128 is held to, its float32 autograd the yardstick E_p.  tests/golden/bc_wide_grad_*.npz (tools/bc_grad_golden.py
--dim 128) pins it to the reference module's own `gmm_loss(...)[0].backward()`.

`wrong=` takes bc_grad_reference's rules and one more, the mistake a copy of the 64-wide kernels makes:
    "quarter_scale"   the value of q uses (D / 4)^-1/2, the gradient path multiplies by 0.25 (the 64-wide scale)"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from . import bc_cases as BC
from . import bc_grad_reference as GR
from . import bc_wide_cases as WC

WRONG = GR.WRONG + ("quarter_scale",)


class Net(GR.Net):
    def __init__(self, sd, max_agents, cfg=BC.CFG, dtype=torch.float64, wrong=None, device="cpu"):
        assert wrong is None or wrong in WRONG + GR.WRONG_AT_EDGES
        super().__init__(sd, max_agents, cfg, dtype, None, device)
        self.wrong = wrong

    def _ln(self, x, name):
        g = self.params[name + ".weight"]
        return F.layer_norm(x, (int(g.shape[0]),), g, self.params[name + ".bias"], 1e-5)

    def _attention(self, xq, xkv, mask, name):
        B, N, J, D = xq.shape[0], xq.shape[1], xkv.shape[1], xq.shape[2]
        ch = D // 4
        split = lambda t, n: t.reshape(B, n, 4, ch).permute(0, 2, 1, 3)  # noqa: E731
        q = split(self._lin(xq, name + ".q_proj"), N)
        if self.wrong == "quarter_scale":
            q = GR._straight_through(q * ch ** -0.5, q * 0.25)
        else:
            q = q * ch ** -0.5
        k, v = split(self._lin(xkv, name + ".k_proj"), J), split(self._lin(xkv, name + ".v_proj"), J)
        attn = torch.einsum("bhic,bhjc->bhij", q, k)
        filled = attn.masked_fill(mask[:, None, None, :], -torch.finfo(attn.dtype).max)
        if self.wrong == "additive_mask":
            filled = GR._straight_through(filled, attn)
        attn = filled.softmax(dim=-1)
        o = torch.einsum("bhij,bhjc->bhic", attn, v).permute(0, 2, 1, 3).reshape(B, N, D)
        return self._lin(o, name + ".o_proj")


def gradients(sd, obs, pm, rm, expert, grad_nll, max_agents, cfg=BC.CFG, dtype=torch.float64, wrong=None):
    """bc_grad_reference.gradients on this module: (gradients per parameter name as float64 numpy, nll [B], margins)."""
    net = Net(sd, max_agents, cfg, dtype, wrong)
    nll = net.nll(obs, pm, rm, expert)
    (nll * torch.as_tensor(grad_nll).to(dtype)).sum().backward()
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad  # noqa: E731
    return (OrderedDict((k, zero(v).double().numpy()) for k, v in net.params.items()), nll.detach().double().numpy(),
            dict(net.margins))


_CASE = {}


def case_inputs(name):
    """(state dict, obs, pm, rm, expert [B, 3], kinds, A, cfg) of the case of bc_wide_cases.CASES or EDGE_CASES."""
    B, A, R, cfg = WC.lookup(name)
    obs, pm, rm, expert, _, _, kinds = BC.inputs(B, A, R, seed=WC.SEEDS[name])
    return BC.state_dict(R, cfg, network_dim=WC.DIM), obs, pm, rm, expert[:, 0], kinds, A, cfg


def case(name, kind="mean", rows=None):
    """The case with its float64 gradients, nll, margins and the yardstick E_p under the upstream gradient `kind`
    (bc_grad_reference.grad_weights), computed once and shared: leave it unchanged.  rows: a subset of the case's rows."""
    key = (name, kind, None if rows is None else tuple(rows))
    if key not in _CASE:
        sd, obs, pm, rm, expert, kinds, A, cfg = case_inputs(name)
        if rows is not None:
            obs, pm, rm, expert, kinds = obs[rows], pm[rows], rm[rows], expert[rows], [kinds[i] for i in rows]
        w = GR.grad_weights(len(obs), kind)
        g64, nll, margins = gradients(sd, obs, pm, rm, expert, w, A, cfg)
        g32, _, _ = gradients(sd, obs, pm, rm, expert, w, A, cfg, dtype=torch.float32)
        _CASE[key] = dict(sd=sd, obs=obs, pm=pm, rm=rm, expert=expert, kinds=kinds, A=A, R=WC.lookup(name)[2], cfg=cfg, w=w, g64=g64,
                          g32=g32, nll=nll, margins=margins, E=GR.yardstick(g32, g64))
    return _CASE[key]


assert np.float32(32.0 ** -0.5).view(np.uint32) == 0x3E3504F3  # the constant the kernels multiply q by (csrc/bc_tile.hpp QSCALE)
