"""The reference of the training-mode dropout of the device policy (gpudrive_lab_amd.dropout.DropoutRule; csrc/dropout_rule.hpp):
a plain Python statement of Philox4x32-10, the host program of the rule (tests/dropout_rule_host.cpp), and the stand-in module
of tests/policy_cases.py with its four `nn.Dropout` layers replaced by a multiply with GIVEN masks.  Test infrastructure for
test_dropout_rule.py, test_policy_dropout.py, test_gpu_policy_dropout.py and test_gpu_ppo_dropout.py."""
import os
import subprocess
import tempfile

import numpy as np
import torch
from torch import nn

from tests import policy_cases as PC
from tests import policy_grad_reference as GR

HERE = os.path.dirname(os.path.abspath(__file__))
SITES = ("ego", "partner", "road", "shared")  # site numbers 0..3
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds on Python ints: counter (4 words) and key (2 words) -> 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def kept_python(seed, call, row, site, entity, feature, threshold):
    """The rule of csrc/dropout_rule.hpp for one element, in plain Python."""
    block = ((feature >> 4) << 1) | ((feature >> 2) & 1)
    field = (((feature >> 3) & 1) << 2) | (feature & 3)
    o = philox4x32_10((call & M32, call >> 32, row, (site << 24) | (entity << 8) | block), (seed & M32, seed >> 32))
    return ((o[field >> 1] >> (16 * (field & 1))) & 0xFFFF) >= threshold


_HOST = [None]


def rule_host():
    """The host program of csrc/dropout_rule.hpp, compiled once per session with g++."""
    if _HOST[0] is None:
        out = os.path.join(tempfile.gettempdir(), "gd_dropout_rule_host_%d" % os.getuid())
        src = os.path.join(HERE, "dropout_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "dropout_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, src])
        _HOST[0] = out
    return _HOST[0]


def host_philox(counter, key):
    out = subprocess.check_output([rule_host(), "philox"] + ["%x" % w for w in tuple(counter) + tuple(key)], text=True)
    return tuple(int(w, 16) for w in out.split())


def host_map():
    """(block, field) of the features 0..127 as an int array [128, 2]."""
    out = subprocess.check_output([rule_host(), "map"], text=True)
    return np.array([[int(v) for v in ln.split()] for ln in out.splitlines()])


def host_mask(seed, call, threshold, site, rows, entities, features):
    """The host program's keep mask as a bool array [rows, entities, features]."""
    with tempfile.TemporaryDirectory() as d:
        fout = os.path.join(d, "mask.bin")
        subprocess.check_call([rule_host(), "mask"] + [str(int(v)) for v in (seed, call, threshold, site, rows, entities, features)]
                              + [fout])
        raw = np.fromfile(fout, np.uint8)
    assert raw.size == rows * entities * features
    return raw.reshape(rows, entities, features).astype(bool)


def host_masks(seed, call, threshold, n, max_agents):
    """The four keep masks of one call on n rows: ego [n, 64], partner [n, A - 1, 64], road [n, 200, 64], shared [n, 128]."""
    return {"ego": host_mask(seed, call, threshold, 0, n, 1, 64)[:, 0],
            "partner": host_mask(seed, call, threshold, 1, n, max_agents - 1, 64),
            "road": host_mask(seed, call, threshold, 2, n, PC.ROADS, 64),
            "shared": host_mask(seed, call, threshold, 3, n, 1, 128)[:, 0]}


def all_kept(n, max_agents):
    return {"ego": np.ones((n, 64), bool), "partner": np.ones((n, max_agents - 1, 64), bool),
            "road": np.ones((n, PC.ROADS, 64), bool), "shared": np.ones((n, 128), bool)}


class GivenMask(nn.Module):
    """nn.Dropout with the mask given: in train mode x * m, m = keep * scale (kept: x * 1 / (1 - p), dropped: 0); in eval mode
    the identity."""

    def __init__(self):
        super().__init__()
        self.m = None

    def forward(self, x):
        return x * self.m if self.training and self.m is not None else x


def masked_stand_in(sd, max_agents, ego_width, dtype, keep=None, scale=1.0):
    """`policy_cases.StandIn` with its four Dropouts replaced by `GivenMask` (the Dropouts hold no parameters, so the state
    dict is the same), the weights of `sd` in `dtype`, in train mode.  keep: the four bool masks (see `host_masks`); scale: the
    float32 value 1 / (1 - p)."""
    net = PC.StandIn(max_agents, ego_width, sd["actor.weight"].shape[0], dropout=0.0)
    for seq, at in ((net.ego_embed, 3), (net.partner_embed, 3), (net.road_map_embed, 3), (net.shared_embed, 1)):
        assert isinstance(seq[at], nn.Dropout)
        seq[at] = GivenMask()
    net = net.to(dtype)
    net.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in sd.items()})
    net.train()
    if keep is not None:
        set_masks(net, keep, scale)
    return net


def set_masks(net, keep, scale):
    dtype = net.actor.weight.dtype
    for name, mod in zip(SITES, (net.ego_embed[3], net.partner_embed[3], net.road_map_embed[3], net.shared_embed[1])):
        mod.m = torch.from_numpy(np.asarray(keep[name])).to(dtype) * torch.tensor(float(np.float32(scale)), dtype=dtype)


def forward(sd, obs, max_agents, ego_width, dtype, keep, scale):
    """(logits, value [N]) of the masked stand-in in train mode, computed in `dtype`, as float64 numpy."""
    net = masked_stand_in(sd, max_agents, ego_width, dtype, keep, scale)
    with torch.no_grad():
        logits, value = net(torch.from_numpy(np.asarray(obs)).to(dtype))
    return logits.double().numpy(), value.double().numpy()[:, 0]


def forward_yardstick(sd, obs, max_agents, ego_width, keep, scale):
    """(logits64, value64, E): E is the float32 computation's maximum absolute error against float64 over logits and value,
    floored at 2^-23 max |.|."""
    l64, v64 = forward(sd, obs, max_agents, ego_width, torch.float64, keep, scale)
    l32, v32 = forward(sd, obs, max_agents, ego_width, torch.float32, keep, scale)
    E = max(np.abs(l32 - l64).max(), np.abs(v32 - v64).max(), 2.0 ** -23 * max(np.abs(l64).max(), np.abs(v64).max()))
    return l64, v64, float(E)


def evaluate(sd, obs, max_agents, ego_width, actions, winners, dtype, keep, scale):
    """`policy_grad_reference.evaluate` (the pools gathered at GIVEN winners) of the masked stand-in; returns (net, logprob,
    entropy, value) with a graph."""
    net = masked_stand_in(sd, max_agents, ego_width, dtype, keep, scale)
    lp, ent, val, _, _ = GR.evaluate(net, obs, actions, winners)
    return net, lp, ent, val


def gradients(sd, obs, max_agents, ego_width, actions, ups, winners, dtype, keep, scale):
    """`policy_grad_reference.gradients` with the masks injected."""
    net, lp, ent, val = evaluate(sd, obs, max_agents, ego_width, actions, winners, dtype, keep, scale)
    d = [torch.as_tensor(np.asarray(u)).to(dtype) for u in ups]
    (d[0] * lp + d[1] * ent + d[2] * val).sum().backward()
    return {k: p.grad.double().numpy() for k, p in net.named_parameters()}
