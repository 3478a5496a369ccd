"""Cases for the device BC policy forward: a seeded state dict of the reference's names and shapes, seeded inputs with the
constructed samples of the issue, a torch stand-in of the module (the yardstick's float32 forward and the eager side of
tools/bc_forward.py), and the host program of csrc/bc_rule.hpp."""
import os
import subprocess
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

from gpudrive_lab_amd import bc_policy as BP

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(num_layer=(3, 2), head_num_layers=2, n_components=6, clip_value=-20.0)
# (B, A, R): L = 264 and 328 and the key counts 63, 127 and 200 are no multiples of 32; B = 17 crosses a wave of rows
SHAPES = ((1, 64, 5), (3, 64, 1), (17, 64, 5), (2, 128, 5))
ROADS = 200


def _cfg(num_layer, head, C, clip):
    return dict(num_layer=num_layer, head_num_layers=head, n_components=C, clip_value=clip)


# (name, B, A, R, cfg): the configurations the host checks accept beyond CFG, each at the smallest shape that reaches what it
# is named for.  top: 288 parameter tensors (bc_opt_rule::MAX_TENSORS), 112 head outputs, head depth 4, road kin 104, every
# count at its limit.  sweep: the reference sweep's model, 252 tensors, the clip10 clamp.  c9 / c10: 63 and 70 head outputs,
# either side of one wave.  deep_branch / deep_fusion: asymmetric layer counts in both directions, A = 128 and even kin, a
# clamp floor above 0.  defaults: more rows than the default chunk_rows = partials = 128 (chunks of 128 + 2).
EDGE_CASES = (
    ("top", 3, 64, 8, _cfg((4, 4), 4, 16, -20.0)),
    ("sweep", 3, 64, 5, _cfg((4, 3), 2, 6, -10.0)),
    ("c9", 3, 64, 1, _cfg((1, 1), 0, 9, -20.0)),
    ("c10", 3, 64, 1, _cfg((1, 1), 0, 10, -20.0)),
    ("deep_branch", 2, 128, 2, _cfg((1, 4), 1, 2, -20.0)),
    ("deep_fusion", 3, 64, 2, _cfg((4, 1), 3, 3, 2.0)),
    ("defaults", 130, 64, 1, _cfg((1, 1), 0, 1, -20.0)),
)
EDGE = {name: (B, A, R, cfg) for name, B, A, R, cfg in EDGE_CASES}


def state_dict(num_stack, cfg=CFG, seed=0, network_dim=64):
    """A numpy default_rng fills each tensor in list order.  Scaled so that attention is not flat: the q / k weights are large
    enough that softmax rows have a clear maximum (scores of standard deviation about 4), LayerNorm gains and biases are not
    1 / 0, biases are not 0.  Two raw covariances are pushed below clip_value and above 3.58352 through the head's bias."""
    rng = np.random.default_rng(seed)
    C = cfg["n_components"]
    sd = {}
    for name, shape in BP.expected_shapes(num_stack, cfg["num_layer"], cfg["head_num_layers"], C, network_dim=network_dim).items():
        n = rng.standard_normal(shape)
        if len(shape) == 2:
            v = n * ((2.0 if (".q_proj." in name or ".k_proj." in name) else 1.0) / np.sqrt(shape[1]))
        elif name.endswith(".weight"):  # a LayerNorm gain
            v = 1.0 + 0.3 * n
        else:
            v = 0.2 * n
        sd[name] = v
    b = sd["head.head.bias"]
    b[3 * C + 1] = cfg["clip_value"] - 10.0  # case (f): below the clamp
    b[3 * C + (5 if C > 1 else 2)] = 10.0    # case (f): above 3.58352
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in sd.items()}


def with_tied_weights(sd, cfg=CFG):
    """Case (e): the raw mixture weights of components 1 and 3 tie exactly at the top in every row (zero weight rows, equal
    biases), so the first index must win."""
    C = cfg["n_components"]
    sd = {k: v.clone() for k, v in sd.items()}
    for c in (1, 3):
        sd["head.head.weight"][6 * C + c] = 0.0
        sd["head.head.bias"][6 * C + c] = 50.0
    return sd


def sample_kinds(B):
    """Which constructed sample each row is: a every partner masked, b every road masked, c exactly one unmasked partner and
    one unmasked road, d a window with a zero prefix (prefix masks True), r random masks."""
    base = {1: ["c"], 2: ["ab", "d"], 3: ["a", "b", "c"]}.get(B, ["a", "b", "c", "d", "ab"])
    return (base + ["r"] * B)[:B]


def inputs(B, A, R, seed=1):
    """obs [B, R, D] float32, partner_mask [B, R, A - 1] bool, road_mask [B, R, 200] bool, expert [B, 1, 3] float32, u [B],
    z [B, 3], kinds."""
    rng = np.random.default_rng([seed, B, A, R])
    D = BP.obs_width(A)
    obs = rng.uniform(-1.0, 1.0, (B, R, D)).astype(np.float32)
    pm = rng.random((B, R, A - 1)) < 0.4
    rm = rng.random((B, R, ROADS)) < 0.4
    kinds = sample_kinds(B)
    for i, kind in enumerate(kinds):
        if "a" in kind:
            pm[i, -1] = True
        if "b" in kind:
            rm[i, -1] = True
        if kind == "c":
            pm[i, -1], rm[i, -1] = True, True
            pm[i, -1, (A - 1) // 2], rm[i, -1, ROADS - 1] = False, False
        if kind == "d" and R > 1:
            pre = max(1, R // 2)
            obs[i, :pre], pm[i, :pre], rm[i, :pre] = 0.0, True, True
    expert = (rng.standard_normal((B, 1, 3)) * np.array([3.0, 0.05, 0.03])).astype(np.float32)
    u = rng.random(B).astype(np.float32)
    z = rng.standard_normal((B, 3)).astype(np.float32)
    return obs, pm, rm, expert, u, z, kinds


def edge_uniforms(B):
    """Case (g): u = 0 and the largest float32 below 1, alternating."""
    u = np.zeros(B, dtype=np.float32)
    u[1::2] = np.nextafter(np.float32(1.0), np.float32(0.0))
    return u


def overwrite_masked(obs, pm, rm, A, seed=7):
    """obs with the features of the partners and roads masked at the LAST time index replaced, at every time, by other
    finite values."""
    rng = np.random.default_rng(seed)
    B, R, D = obs.shape
    out = obs.copy()
    p = out[:, :, 6:6 + 6 * (A - 1)].reshape(B, R, A - 1, 6)
    g = out[:, :, 6 + 6 * (A - 1):].reshape(B, R, ROADS, 13)
    mp, mg = np.broadcast_to(pm[:, -1][:, None, :], (B, R, A - 1)), np.broadcast_to(rm[:, -1][:, None, :], (B, R, ROADS))
    p[mp] = rng.uniform(-3, 3, (int(mp.sum()), 6)).astype(np.float32)
    g[mg] = rng.uniform(-3, 3, (int(mg.sum()), 13)).astype(np.float32)
    out[:, :, 6:6 + 6 * (A - 1)] = p.reshape(B, R, -1)
    out[:, :, 6 + 6 * (A - 1):] = g.reshape(B, R, -1)
    return out


class StandIn:
    """The module as eager torch in one dtype on one device: the project's own stand-in for EarlyFusionAttnBCNet in eval mode
    (same state dict names; F.layer_norm, F.gelu, masked_fill with -finfo.max, softmax, einsum, as the reference writes it).
    The width is the state dict's: LayerNorm over D features, 4 heads of D / 4 channels."""

    def __init__(self, sd, max_agents, cfg=CFG, dtype=torch.float32, device="cpu"):
        self.sd = {k: v.detach().to(device=device, dtype=dtype) for k, v in sd.items()}
        self.A, self.cfg, self.dtype, self.device = max_agents, cfg, dtype, device
        self.D = int(sd["ego_state_net.2.weight"].shape[0])

    def _lin(self, x, name):
        return F.linear(x, self.sd[name + ".weight"], self.sd[name + ".bias"])

    def _ln(self, x, name):
        return F.layer_norm(x, (self.D,), self.sd[name + ".weight"], self.sd[name + ".bias"], 1e-5)

    def _embed(self, x, net):
        for i in range(4):
            x = torch.tanh(self._ln(self._lin(x, "%s.%d" % (net, 4 * i)), "%s.%d" % (net, 4 * i + 2)))
        return x

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

    def _mlp(self, x, name):
        return x + self._lin(F.gelu(self._lin(self._ln(x, name + ".0"), name + ".1")), name + ".3")

    def _self(self, x, mask, name):
        h = self._ln(x, name + ".0.module.norm")
        return self._mlp(self._attention(h, h, mask, name + ".0.module.attention")[0] + x, name + ".1.module")

    def _cross(self, xq, xkv, mask, name):
        o, p = self._attention(self._ln(xq, name + ".0.module.q_norm"), self._ln(xkv, name + ".0.module.kv_norm"), mask,
                               name + ".0.module.attention")
        return self._mlp(o + xq, name + ".1.module"), p[:, :, 0]

    @torch.no_grad()
    def forward(self, obs, partner_mask, road_mask, expert=None):
        """obs [B, R, D], masks [B, R, *] (tensors on the device) -> dict of context, ego_attn_score, means, log_covariances,
        covariances, weights, and with expert [B, 1, 3] the nll (gmm_loss's closed form in this dtype)."""
        A, cfg, C = self.A, self.cfg, self.cfg["n_components"]
        obs = obs.to(self.dtype)
        B, R, _ = obs.shape
        pm, rm = partner_mask[:, -1].bool(), road_mask[:, -1].bool()
        ego = obs[..., :6].reshape(B, R * 6)
        ro = obs[..., 6:6 + 6 * (A - 1)].view(B, R, A - 1, 6).permute(0, 2, 1, 3).reshape(B, A - 1, R * 6)
        rg = obs[..., 6 + 6 * (A - 1):].view(B, R, ROADS, 13).permute(0, 2, 1, 3).reshape(B, ROADS, R * 13)
        x = torch.cat([self._embed(ego, "ego_state_net").unsqueeze(1), self._embed(ro, "road_object_net"),
                       self._embed(rg, "road_graph_net")], dim=1)
        ego_mask = torch.zeros(B, 1, dtype=torch.bool, device=obs.device)
        all_mask, obj_mask = torch.cat([ego_mask, pm, rm], -1), torch.cat([ego_mask, pm], -1)
        for i in range(cfg["num_layer"][0]):
            x = self._self(x, all_mask, "fusion_attn.%d" % i)
        objs, roads = x[:, :A], x[:, A:]
        for i in range(cfg["num_layer"][1]):
            objs = self._self(objs, obj_mask, "ro_attn.%d" % i)
        for i in range(cfg["num_layer"][1]):
            roads = self._self(roads, rm, "rg_attn.%d" % i)
        ego_tok = objs[:, :1]
        ego_ro, score = self._cross(ego_tok, objs[:, 1:], pm, "ego_ro_attn")
        ego_rg, _ = self._cross(ego_tok, roads, rm, "ego_rg_attn")
        context = torch.cat([ego_tok[:, 0], ego_ro[:, 0], ego_rg[:, 0]], dim=1)
        h = torch.relu(self._lin(context, "head.input_layer.0"))
        for i in range(cfg["head_num_layers"]):
            h = h + torch.relu(self._lin(h, "head.residual_block.%d.0" % i))
        raw = self._lin(h, "head.head")
        logcov = torch.clamp(raw[:, 3 * C:6 * C], cfg["clip_value"], 3.58352).view(B, C, 3)
        out = dict(context=context, ego_attn_score=score / score.sum(-1, keepdim=True), means=raw[:, :3 * C].view(B, C, 3),
                   log_covariances=logcov, covariances=torch.exp(logcov), weights=torch.softmax(raw[:, 6 * C:], -1))
        if expert is not None:
            a = expert.to(self.dtype).reshape(B, 1, 3)
            lp = -0.5 * ((a - out["means"]) ** 2 / out["covariances"]).sum(-1) - 0.5 * logcov.sum(-1) - 1.5 * np.log(2 * np.pi)
            out["nll"] = -torch.logsumexp(lp + torch.log(out["weights"] + 1e-8), dim=-1)
        return out


COMPARED = ("context", "means", "log_covariances", "weights")


def standin_float32(sd, obs, pm, rm, A, cfg=CFG, expert=None):
    """torch's float32 CPU forward of the stand-in, as float64 numpy arrays."""
    out = StandIn(sd, A, cfg, torch.float32, "cpu").forward(torch.from_numpy(obs), torch.from_numpy(pm), torch.from_numpy(rm),
                                                            None if expert is None else torch.from_numpy(expert))
    return {k: v.double().numpy() for k, v in out.items()}


def yardstick(f32, ref):
    """E per compared output: the maximum absolute error of the float32 stand-in against the float64 restatement (nll and
    ego_attn_score too where both sides carry them)."""
    return {k: float(np.abs(f32[k] - ref[k]).max()) for k in COMPARED + ("nll", "ego_attn_score") if k in f32 and k in ref}


_HOST = [None]


def rule_host():
    """The host program of csrc/bc_rule.hpp, compiled once per session with g++ (no contraction)."""
    if _HOST[0] is None:
        out = os.path.join(tempfile.gettempdir(), "gd_bc_rule_host_%d" % os.getuid())
        src = os.path.join(HERE, "bc_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "bc_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, src])
        _HOST[0] = out
    return _HOST[0]


def run_rule_host(raw, clip_value, u, z, expert, deterministic):
    """The host program on float32 raw [N, 7 C]: dict of log_covariances, covariances [N, C, 3], weights [N, C], component [N],
    actions [N, 3], nll [N]."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    n, C = raw.shape[0], raw.shape[1] // 7
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (u, z, expert)]
    assert arrs[0].shape == (n,) and arrs[1].shape == (n, 3) and arrs[2].shape == (n, 3)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, C, int(deterministic)], dtype=np.int32).tobytes() + np.float32(clip_value).tobytes()
                    + raw.tobytes() + b"".join(a.tobytes() for a in arrs))
        subprocess.check_call([rule_host(), fin, fout])
        buf = open(fout, "rb").read()
    per = 3 * C + 3 * C + C + 1 + 3 + 1
    rows = np.frombuffer(buf, np.float32).reshape(n, per)
    o = 0
    out = {}
    for name, k in (("log_covariances", 3 * C), ("covariances", 3 * C), ("weights", C), ("component", 1), ("actions", 3), ("nll", 1)):
        out[name] = rows[:, o:o + k]
        o += k
    out["log_covariances"], out["covariances"] = out["log_covariances"].reshape(n, C, 3), out["covariances"].reshape(n, C, 3)
    out["component"], out["nll"] = out["component"][:, 0].astype(np.int64), out["nll"][:, 0]
    return out
