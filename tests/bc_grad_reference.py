"""The BC policy's training loss written differentiably: the stand-in of EarlyFusionAttnBCNet (bc_cases.StandIn's arithmetic,
the reference module's state-dict names) with an out-of-place masked_fill and no no_grad, followed by gmm_loss's per-row
value in closed form.  Run under torch autograd in float64 on the CPU this is what the device backward's parameter
gradients are held to; run in float32 it is the yardstick E_p.  tests/test_bc_grad.py pins it to the reference module's own
`gmm_loss(...)[0].backward()` (tests/golden/bc_grad_*.npz, written by tools/bc_grad_golden.py).

`wrong=` switches ONE rule to a plausible mistake, so that the tests can show the comparison catches it (the first three
leave the forward's values what they are and change the backward alone):
    "additive_mask"   the mask is added to the scores instead of filled in, so gradient flows through masked scores: a row
                      whose keys are all masked (p uniform) then sends gradient into q and k
    "soft_clamp"      the covariance clamp passes the gradient outside its bounds
    "tanh_gelu"       GELU's derivative is that of the tanh approximation
    "normed_residual" the attention residual adds the LayerNorm'ed input instead of the input
and four that are the right rule at bc_cases.CFG and wrong only at configurations of bc_cases.EDGE_CASES (bc_reference.py
states them for the forward):
    "head_one_trip"   the head's outputs of index >= 64 stay at their bias: their rows of head.head get no gradient
    "rg_at_ro"        rg_attn layer i runs on ro_attn layer i's weights for i >= min(fusion, branch)
    "floor_m20"       the covariance clamp's floor is -20 whatever clip_value says
    "kin_three_tiles" the road embedder's first layer reads its inputs 0 .. 95 only (three 32-column tiles; right for
                      num_stack <= 7): at num_stack 8 columns 96 .. 103 of road_graph_net.0.weight get no gradient

Also here: the host program of csrc/bc_grad_rule.hpp and the float64 autograd of the mixture nll it is compared with."""
import math
import os
import subprocess
import tempfile
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from gpudrive_lab_amd import bc_policy as BP

from . import bc_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))
COV_MAX = 3.58352
ROADS = 200
WRONG = ("additive_mask", "soft_clamp", "tanh_gelu", "normed_residual")
WRONG_AT_EDGES = ("head_one_trip", "rg_at_ro", "floor_m20", "kin_three_tiles")
MINIMAL = dict(num_layer=(1, 1), head_num_layers=0, n_components=1, clip_value=-20.0)
MARGIN = 1e-3


def _straight_through(value, grad_path):
    """value's number, grad_path's gradient"""
    return grad_path + (value - grad_path).detach()


class Net:
    """The module in one dtype on one device (the CPU for every reference; tools/bc_backward.py times it on the GPU) with every
    parameter a leaf."""

    def __init__(self, sd, max_agents, cfg=BC.CFG, dtype=torch.float64, wrong=None, device="cpu"):
        assert wrong is None or wrong in WRONG + WRONG_AT_EDGES
        self.params = OrderedDict((k, v.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)) for k, v in sd.items())
        self.A, self.cfg, self.dtype, self.wrong, self.device = max_agents, cfg, dtype, wrong, device
        self.margins = {}

    def _lin(self, x, name):
        return F.linear(x, self.params[name + ".weight"], self.params[name + ".bias"])

    def _ln(self, x, name):
        return F.layer_norm(x, (64,), self.params[name + ".weight"], self.params[name + ".bias"], 1e-5)

    def _embed(self, x, net):
        for i in range(4):
            if self.wrong == "kin_three_tiles" and i == 0 and net == "road_graph_net" and x.shape[-1] > 96:
                y = F.linear(x[..., :96], self.params[net + ".0.weight"][:, :96], self.params[net + ".0.bias"])
            else:
                y = self._lin(x, "%s.%d" % (net, 4 * i))
            x = torch.tanh(self._ln(y, "%s.%d" % (net, 4 * i + 2)))
        return x

    def _gelu(self, x):
        if self.wrong == "tanh_gelu":
            return _straight_through(F.gelu(x), F.gelu(x, approximate="tanh"))
        return F.gelu(x)

    def _attention(self, xq, xkv, mask, name):
        B, N, J = xq.shape[0], xq.shape[1], xkv.shape[1]
        split = lambda t, n: t.reshape(B, n, 4, 16).permute(0, 2, 1, 3)  # noqa: E731
        q = split(self._lin(xq, name + ".q_proj"), N) * 16 ** -0.5
        k, v = split(self._lin(xkv, name + ".k_proj"), J), split(self._lin(xkv, name + ".v_proj"), J)
        attn = torch.einsum("bhic,bhjc->bhij", q, k)
        m = mask[:, None, None, :]
        filled = attn.masked_fill(m, -torch.finfo(attn.dtype).max)
        if self.wrong == "additive_mask":
            filled = _straight_through(filled, attn)
        attn = filled.softmax(dim=-1)
        o = torch.einsum("bhij,bhjc->bhic", attn, v).permute(0, 2, 1, 3).reshape(B, N, 64)
        return self._lin(o, name + ".o_proj")

    def _mlp(self, x, name):
        return x + self._lin(self._gelu(self._lin(self._ln(x, name + ".0"), name + ".1")), name + ".3")

    def _residual(self, o, x, h):
        return o + (h if self.wrong == "normed_residual" else x)

    def _self(self, x, mask, name):
        h = self._ln(x, name + ".0.module.norm")
        return self._mlp(self._residual(self._attention(h, h, mask, name + ".0.module.attention"), x, h), name + ".1.module")

    def _cross(self, xq, xkv, mask, name):
        h = self._ln(xq, name + ".0.module.q_norm")
        o = self._attention(h, self._ln(xkv, name + ".0.module.kv_norm"), mask, name + ".0.module.attention")
        return self._mlp(self._residual(o, xq, h), name + ".1.module")

    def nll(self, obs, partner_mask, road_mask, expert):
        """obs [B, R, D], masks [B, R, *], expert [B, 1, 3] or [B, 3] (numpy or tensors) -> nll [B], differentiable in the
        parameters.  Sets self.margins: `clamp` the smallest distance of any raw covariance from either clamp bound, `relu`
        the smallest distance of any head ReLU pre-activation from 0."""
        A, cfg, C = self.A, self.cfg, self.cfg["n_components"]
        obs = torch.as_tensor(obs).to(device=self.device, dtype=self.dtype)
        B, R, _ = obs.shape
        pm, rm = (torch.as_tensor(m).to(self.device)[:, -1].bool() for m in (partner_mask, road_mask))
        ego = obs[..., :6].reshape(B, R * 6)
        ro = obs[..., 6:6 + 6 * (A - 1)].view(B, R, A - 1, 6).permute(0, 2, 1, 3).reshape(B, A - 1, R * 6)
        rg = obs[..., 6 + 6 * (A - 1):].view(B, R, ROADS, 13).permute(0, 2, 1, 3).reshape(B, ROADS, R * 13)
        x = torch.cat([self._embed(ego, "ego_state_net").unsqueeze(1), self._embed(ro, "road_object_net"),
                       self._embed(rg, "road_graph_net")], dim=1)
        ego_mask = torch.zeros(B, 1, dtype=torch.bool, device=self.device)
        all_mask, obj_mask = torch.cat([ego_mask, pm, rm], -1), torch.cat([ego_mask, pm], -1)
        for i in range(cfg["num_layer"][0]):
            x = self._self(x, all_mask, "fusion_attn.%d" % i)
        objs, roads = x[:, :A], x[:, A:]
        for i in range(cfg["num_layer"][1]):
            objs = self._self(objs, obj_mask, "ro_attn.%d" % i)
        for i in range(cfg["num_layer"][1]):
            blk = "ro_attn" if self.wrong == "rg_at_ro" and i >= min(cfg["num_layer"]) else "rg_attn"
            roads = self._self(roads, rm, "%s.%d" % (blk, i))
        ego_tok = objs[:, :1]
        ego_ro = self._cross(ego_tok, objs[:, 1:], pm, "ego_ro_attn")
        ego_rg = self._cross(ego_tok, roads, rm, "ego_rg_attn")
        context = torch.cat([ego_tok[:, 0], ego_ro[:, 0], ego_rg[:, 0]], dim=1)
        pre = [self._lin(context, "head.input_layer.0")]
        h = torch.relu(pre[0])
        for i in range(cfg["head_num_layers"]):
            pre.append(self._lin(h, "head.residual_block.%d.0" % i))
            h = h + torch.relu(pre[-1])
        raw = self._lin(h, "head.head")
        if self.wrong == "head_one_trip":
            raw = torch.cat([raw[:, :64], self.params["head.head.bias"][64:].expand(B, -1)], dim=1)
        rc = raw[:, 3 * C:6 * C].detach()
        self.margins = dict(clamp=float(torch.minimum((rc - cfg["clip_value"]).abs(), (rc - COV_MAX).abs()).min()),
                            relu=float(torch.stack(pre).detach().abs().min()))
        return mixture_nll(raw, torch.as_tensor(expert).to(device=self.device, dtype=self.dtype), C,
                           -20.0 if self.wrong == "floor_m20" else cfg["clip_value"], soft_clamp=self.wrong == "soft_clamp")


def mixture_nll(raw, expert, C, clip_value, cov_max=COV_MAX, soft_clamp=False):
    """gmm_loss's per-row value from the head's raw outputs [B, 7 C] as torch writes it: clamp, exp, softmax, log(w + 1e-8),
    logsumexp."""
    B = raw.shape[0]
    means = raw[:, :3 * C].view(B, C, 3)
    rc = raw[:, 3 * C:6 * C]
    logcov = torch.clamp(rc, clip_value, cov_max)
    if soft_clamp:
        logcov = _straight_through(logcov, rc)
    logcov = logcov.view(B, C, 3)
    weights = torch.softmax(raw[:, 6 * C:], -1)
    a = expert.reshape(B, 1, 3)
    lp = -0.5 * ((a - means) ** 2 / torch.exp(logcov)).sum(-1) - 0.5 * logcov.sum(-1) - 1.5 * math.log(2 * math.pi)
    return -torch.logsumexp(lp + torch.log(weights + 1e-8), dim=-1)


def gradients(sd, obs, pm, rm, expert, grad_nll, max_agents, cfg=BC.CFG, dtype=torch.float64, wrong=None):
    """(gradients of sum_b grad_nll[b] nll[b] per parameter name as float64 numpy, nll [B] float64 numpy, margins)."""
    net = Net(sd, max_agents, cfg, dtype, wrong)
    nll = net.nll(obs, pm, rm, expert)
    (nll * torch.as_tensor(grad_nll).to(dtype)).sum().backward()
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad  # noqa: E731  (a wrong rule may leave a tensor unused)
    return (OrderedDict((k, zero(v).double().numpy()) for k, v in net.params.items()), nll.detach().double().numpy(),
            dict(net.margins))


def yardstick(g32, g64):
    """E_p per parameter tensor: the float32 stand-in's maximum absolute gradient error, floored at 2^-23 max |g|."""
    return {k: max(float(np.abs(g32[k] - g64[k]).max()), 2.0 ** -23 * float(np.abs(g64[k]).max())) for k in g64}


def grad_weights(B, kind, seed=11):
    """The upstream gradient: 1 / B (`mean`), or seeded unequal weights of both signs (`seeded`)."""
    if kind == "mean":
        return np.full(B, 1.0 / B, dtype=np.float32)
    return (np.random.default_rng([seed, B]).uniform(0.25, 1.5, B) * np.where(np.arange(B) % 3 == 1, -1.0, 1.0)).astype(np.float32)


def case_key(B, A, R, cfg=BC.CFG):
    return (B, A, R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], cfg["clip_value"])


# The seed of bc_cases.inputs per case: the first (from 1) with which both margins of `Net.nll` exceed MARGIN in float64 on
# bc_cases.state_dict(R, cfg), so that no clamp and no ReLU of the head can flip between float32 and float64
# (tools/bc_grad_golden.py --seeds prints this table).  bc_cases.SHAPES at bc_cases.CFG, the chunked case, one minimal model.
# The key carries clip_value: two of the edge cases differ from another key in the clamp alone.
INPUT_SEEDS = {
    (1, 64, 5, (3, 2), 2, 6, -20.0): 1,  # margins clamp 0.404 relu 0.00157
    (3, 64, 1, (3, 2), 2, 6, -20.0): 1,  # margins clamp 0.0548 relu 0.00793
    (17, 64, 5, (3, 2), 2, 6, -20.0): 1,  # margins clamp 0.00452 relu 0.00188
    (2, 128, 5, (3, 2), 2, 6, -20.0): 2,  # margins clamp 0.145 relu 0.0206
    (5, 64, 5, (3, 2), 2, 6, -20.0): 1,  # margins clamp 0.0181 relu 0.0033
    (8, 64, 5, (3, 2), 2, 6, -20.0): 1,  # margins clamp 0.0801 relu 0.00103
    (3, 64, 1, (1, 1), 0, 1, -20.0): 1,  # margins clamp 1.87 relu 0.0153
    # bc_cases.EDGE_CASES: top, sweep, c9, c10, deep_branch, deep_fusion, defaults
    (3, 64, 8, (4, 4), 4, 16, -20.0): 1,  # margins clamp 0.0729 relu 0.00105
    (3, 64, 5, (4, 3), 2, 6, -10.0): 1,  # margins clamp 0.0303 relu 0.0158
    (3, 64, 1, (1, 1), 0, 9, -20.0): 1,  # margins clamp 0.0173 relu 0.0153
    (3, 64, 1, (1, 1), 0, 10, -20.0): 1,  # margins clamp 0.0147 relu 0.0153
    (2, 128, 2, (1, 4), 1, 2, -20.0): 1,  # margins clamp 2.64 relu 0.00612
    (3, 64, 2, (4, 1), 3, 3, 2.0): 1,  # margins clamp 0.304 relu 0.0159
    (130, 64, 1, (1, 1), 0, 1, -20.0): 2,  # margins clamp 0.271 relu 0.00133
}


def state_dict(R, cfg=BC.CFG):
    """bc_cases.state_dict; for a mixture too small for its two pushed covariances (C = 1) the same fill without them."""
    C = cfg["n_components"]
    if 3 * C + 5 < 6 * C:
        return BC.state_dict(R, cfg)
    rng = np.random.default_rng(0)
    sd = {}
    for name, shape in BP.expected_shapes(R, cfg["num_layer"], cfg["head_num_layers"], C).items():
        n = rng.standard_normal(shape)
        if len(shape) == 2:
            v = n * ((2.0 if (".q_proj." in name or ".k_proj." in name) else 1.0) / np.sqrt(shape[1]))
        else:
            v = 1.0 + 0.3 * n if name.endswith(".weight") else 0.2 * n
        sd[name] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return sd


def case_inputs(B, A, R, cfg=BC.CFG):
    """(state dict, obs, pm, rm, expert [B, 3], kinds) of a case, with the input seed that keeps the margins."""
    obs, pm, rm, expert, _, _, kinds = BC.inputs(B, A, R, seed=INPUT_SEEDS[case_key(B, A, R, cfg)])
    return state_dict(R, cfg), obs, pm, rm, expert[:, 0], kinds


# ---- the host program of csrc/bc_grad_rule.hpp

_HOST = [None]


def grad_rule_host():
    """Compiled once per session with g++ (no contraction)."""
    if _HOST[0] is None:
        out = os.path.join(tempfile.gettempdir(), "gd_bc_grad_rule_host_%d" % os.getuid())
        src = os.path.join(HERE, "bc_grad_rule_host.cpp")
        hdrs = [os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", h) for h in ("bc_rule.hpp", "bc_grad_rule.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, src])
        _HOST[0] = out
    return _HOST[0]


def run_grad_rule_host(raw, clip_value, expert):
    """The host program on float32 raw [N, 7 C] and expert [N, 3]: (d nll / d raw [N, 7 C], nll [N]), float32."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    expert = np.ascontiguousarray(expert, dtype=np.float32)
    n, C = raw.shape[0], raw.shape[1] // 7
    assert expert.shape == (n, 3)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, C], dtype=np.int32).tobytes() + np.float32(clip_value).tobytes() + raw.tobytes() + expert.tobytes())
        subprocess.check_call([grad_rule_host(), fin, fout])
        rows = np.frombuffer(open(fout, "rb").read(), np.float32).reshape(n, 7 * C + 1)
    return rows[:, :7 * C], rows[:, 7 * C]


assert BP.ROADS == ROADS
