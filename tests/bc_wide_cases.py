"""Cases for the BC policy forward at network_dim = 128: a seeded wide state dict (tests/bc_cases.py's scaling rules), the
width-parameterised eager float32 stand-in (the yardstick's float32 side), and the four cases.  Inputs, masks, the yardstick and
the rule's host program are tests/bc_cases.py's own."""
import numpy as np
import torch
import torch.nn.functional as F

from gpudrive_lab_amd import bc_policy as BP
from tests import bc_cases as BC
from tests import bc_reference as REF
from tests import bc_wide_reference as WREF

DIM = 128

# name -> (B, A, R, cfg).  wide_min: samples a, b, c (every partner masked, every road masked, one key left), L = 264, 63 and 200
# keys (no multiples of 32), odd first-layer kin (6 and 13).  wide_sweep: the reference sweep's model itself.  wide_a128: 127 keys,
# L = 328, branch > fusion (the rg_attn layers sit past ro_attn's in the blob), sample d (the zero-prefix window).  wide_chunks:
# more rows than a small chunk, for chunk_rows 2 against 8.
CASES = {
    "wide_min": (3, 64, 1, BC._cfg((1, 1), 0, 1, -20.0)),
    "wide_sweep": (3, 64, 5, BC._cfg((4, 3), 2, 6, -20.0)),
    "wide_a128": (2, 128, 2, BC._cfg((1, 2), 1, 2, -20.0)),
    "wide_chunks": (5, 64, 1, BC._cfg((1, 1), 0, 6, -20.0)),
}
GOLDEN_CASES = ("wide_min", "wide_sweep", "wide_a128")


def shapes(R, cfg, network_dim=DIM):
    return BP.expected_shapes(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], network_dim=network_dim)


def state_dict(num_stack, cfg, seed=0, network_dim=DIM):
    """bc_cases.state_dict at another width: a numpy default_rng fills each tensor in list order; Linear weights scale with
    1 / sqrt(fan-in), twice that for q and k (softmax rows with a clear maximum); LayerNorm gains 1 + 0.3 n, biases 0.2 n; two
    raw covariances pushed below clip_value and above 3.58352 through the head's bias."""
    rng = np.random.default_rng(seed)
    C = cfg["n_components"]
    sd = {}
    for name, shape in shapes(num_stack, cfg, network_dim).items():
        n = rng.standard_normal(shape)
        if len(shape) == 2:
            v = n * ((2.0 if (".q_proj." in name or ".k_proj." in name) else 1.0) / np.sqrt(shape[1]))
        elif name.endswith(".weight"):  # a LayerNorm gain
            v = 1.0 + 0.3 * n
        else:
            v = 0.2 * n
        sd[name] = v
    b = sd["head.head.bias"]
    b[3 * C + 1] = cfg["clip_value"] - 10.0
    if C > 1:
        b[3 * C + 5] = 10.0
    else:
        b[3 * C + 2] = 10.0
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in sd.items()}


class WideStandIn(BC.StandIn):
    """bc_cases.StandIn with the width taken from the state dict: LayerNorm over D features, 4 heads of D / 4 channels."""

    def __init__(self, sd, max_agents, cfg, dtype=torch.float32, device="cpu"):
        super().__init__(sd, max_agents, cfg, dtype, device)
        self.D = int(sd["ego_state_net.2.weight"].shape[0])

    def _ln(self, x, name):
        return F.layer_norm(x, (self.D,), self.sd[name + ".weight"], self.sd[name + ".bias"], 1e-5)

    def _attention(self, xq, xkv, mask, name):
        B, N, J, ch = xq.shape[0], xq.shape[1], xkv.shape[1], self.D // 4
        split = lambda t, n: t.reshape(B, n, 4, ch).permute(0, 2, 1, 3)  # noqa: E731
        q = split(self._lin(xq, name + ".q_proj"), N) * ch ** -0.5
        k, v = split(self._lin(xkv, name + ".k_proj"), J), split(self._lin(xkv, name + ".v_proj"), J)
        attn = torch.einsum("bhic,bhjc->bhij", q, k)
        attn.masked_fill_(mask[:, None, None, :], -torch.finfo(attn.dtype).max)
        attn = attn.softmax(dim=-1)
        o = torch.einsum("bhij,bhjc->bhic", attn, v).permute(0, 2, 1, 3).reshape(B, N, self.D)
        return self._lin(o, name + ".o_proj"), attn


def standin_float32(sd, obs, pm, rm, A, cfg, expert=None):
    """torch's float32 CPU forward of the wide stand-in, as float64 numpy arrays."""
    out = WideStandIn(sd, A, cfg).forward(torch.from_numpy(obs), torch.from_numpy(pm), torch.from_numpy(rm),
                                          None if expert is None else torch.from_numpy(expert))
    return {k: v.double().numpy() for k, v in out.items()}


_CASE = {}


def case(name):
    """Everything a test needs of one case, computed once and shared (leave it unchanged): the state dict, the inputs, the
    float64 restatement with its nll, the float32 stand-in and the yardstick E per output."""
    if name not in _CASE:
        B, A, R, cfg = CASES[name]
        sd = state_dict(R, cfg)
        obs, pm, rm, expert, u, z, kinds = BC.inputs(B, A, R)
        ref = WREF.forward(sd, obs, pm, rm, A, **cfg)
        ref["nll"] = REF.nll(ref["means"], ref["log_covariances"], ref["weights"], expert[:, 0])
        f32 = standin_float32(sd, obs, pm, rm, A, cfg, expert)
        _CASE[name] = dict(B=B, A=A, R=R, cfg=cfg, sd=sd, obs=obs, pm=pm, rm=rm, expert=expert, u=u, z=z, kinds=kinds, ref=ref,
                           f32=f32, E=BC.yardstick(f32, ref))
    return _CASE[name]
