"""The BC policy restated in float64 numpy with the encoder's width as a parameter: what the 128-wide forward
(gd_bc_forward_dim, csrc/bc_policy.hip at T = 4) is held to.  tests/bc_reference.py fixes DIM = 64; this is the same restatement,
in this repository's own words, for `network_dim` D and head_dim 64: every embedder, LayerNorm and attention Linear is D wide,
the 4 heads have D / 4 channels and q is scaled by (D / 4)^-1/2, the context is 3 D wide, and the GMM head behind
head.input_layer (3 D -> 64) is as at 64.  tests/test_bc_wide.py pins it to the reference module itself at D = 128
(tests/golden/bc_wide_forward_*.npz); at D = 64 it is tests/bc_reference.py's forward.

`wrong=` switches ONE rule to a mistake the 128 case invites:
    "scale16"      q * 0.25, the 64-wide kernel's constant, instead of q * 32^-1/2
    "heads_of_16"  eight heads of 16 channels (the 64-wide head size kept) instead of four of 32
    "ctx192"       the head reads the first 192 context inputs only (the 64-wide CTX kept)
    "ln64"         LayerNorm statistics over the first 64 features only (one lane per feature, one wave)"""
import numpy as np

from tests import bc_reference as REF

HEADS, HEAD_DIM = 4, 64


def layer_norm(x, sd, name, wrong=None):
    stat = x[..., :64] if wrong == "ln64" else x
    mean = stat.mean(-1, keepdims=True)
    var = ((stat - mean) ** 2).mean(-1, keepdims=True)  # biased
    return (x - mean) / np.sqrt(var + 1e-5) * sd[name + ".weight"] + sd[name + ".bias"]


def embed(x, sd, net, wrong=None):
    for i in range(4):  # Linear -> LayerNorm -> tanh
        x = np.tanh(layer_norm(REF.linear(x, sd, "%s.%d" % (net, 4 * i)), sd, "%s.%d" % (net, 4 * i + 2), wrong))
    return x


def attention(xq, xkv, mask, sd, name, wrong=None):
    """xq [B, N, D], xkv [B, J, D] (both already normed), mask [B, J] bool (True: padding).  Returns (o_proj's output [B, N, D],
    the probabilities [B, heads, N, J])."""
    B, N, D = xq.shape
    J = xkv.shape[1]
    heads = D // 16 if wrong == "heads_of_16" else HEADS
    ch = D // heads
    split = lambda t, n: t.reshape(B, n, heads, ch).transpose(0, 2, 1, 3)  # noqa: E731
    q = split(REF.linear(xq, sd, name + ".q_proj"), N) * (0.25 if wrong == "scale16" else ch ** -0.5)
    k = split(REF.linear(xkv, sd, name + ".k_proj"), J)
    v = split(REF.linear(xkv, sd, name + ".v_proj"), J)
    s = np.einsum("bhic,bhjc->bhij", q, k)
    s = np.where(np.broadcast_to(mask[:, None, None, :], s.shape), -REF.FLT_MAX, s)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    o = np.einsum("bhij,bhjc->bhic", p, v).transpose(0, 2, 1, 3).reshape(B, N, D)
    return REF.linear(o, sd, name + ".o_proj"), p


def mlp(x, sd, name, wrong=None):
    z = REF.linear(layer_norm(x, sd, name + ".0", wrong), sd, name + ".1")
    return x + REF.linear(REF.gelu(z), sd, name + ".3")


def self_layer(x, mask, sd, name, wrong=None):
    h = layer_norm(x, sd, name + ".0.module.norm", wrong)
    o, _ = attention(h, h, mask, sd, name + ".0.module.attention", wrong)
    return mlp(o + x, sd, name + ".1.module", wrong)


def cross_layer(xq, xkv, mask, sd, name, wrong=None):
    q = layer_norm(xq, sd, name + ".0.module.q_norm", wrong)
    kv = layer_norm(xkv, sd, name + ".0.module.kv_norm", wrong)
    o, p = attention(q, kv, mask, sd, name + ".0.module.attention", wrong)
    return mlp(o + xq, sd, name + ".1.module", wrong), p[:, :, 0, :]


def head(sd, context, head_num_layers, C, clip_value, wrong=None):
    w, b = sd["head.input_layer.0.weight"], sd["head.input_layer.0.bias"]
    if wrong == "ctx192":
        x = context[:, :192] @ w[:, :192].T + b
    else:
        x = context @ w.T + b
    x = np.maximum(x, 0.0)
    for i in range(head_num_layers):
        x = x + np.maximum(REF.linear(x, sd, "head.residual_block.%d.0" % i), 0.0)
    return REF.mixture(REF.linear(x, sd, "head.head"), C, clip_value)


def forward(sd, obs, partner_mask, road_mask, max_agents, num_layer, head_num_layers, n_components, clip_value, wrong=None):
    """Everything the module computes for a batch, float64; the width is the state dict's: context [B, 3 D], ego_attn_score
    [B, 4, A - 1], raw [B, 7 C], means, log_covariances and covariances [B, C, 3], weights [B, C]."""
    sd = REF._sd64(sd)
    obs = np.asarray(obs, dtype=np.float64)
    A, C = max_agents, n_components
    B = obs.shape[0]
    pm = np.asarray(partner_mask).astype(bool)[:, -1]
    rm = np.asarray(road_mask).astype(bool)[:, -1]
    ego, ro, rg = REF.unpack(obs, A)
    x = np.concatenate([embed(ego, sd, "ego_state_net", wrong)[:, None], embed(ro, sd, "road_object_net", wrong),
                        embed(rg, sd, "road_graph_net", wrong)], axis=1)
    ego_mask = np.zeros((B, 1), dtype=bool)
    all_mask, obj_mask = np.concatenate([ego_mask, pm, rm], 1), np.concatenate([ego_mask, pm], 1)
    for i in range(num_layer[0]):
        x = self_layer(x, all_mask, sd, "fusion_attn.%d" % i, wrong)
    objs, roads = x[:, :A], x[:, A:]
    for i in range(num_layer[1]):
        objs = self_layer(objs, obj_mask, sd, "ro_attn.%d" % i, wrong)
    for i in range(num_layer[1]):
        roads = self_layer(roads, rm, sd, "rg_attn.%d" % i, wrong)
    ego_tok = objs[:, :1]
    ego_ro, score = cross_layer(ego_tok, objs[:, 1:], pm, sd, "ego_ro_attn", wrong)
    ego_rg, _ = cross_layer(ego_tok, roads, rm, sd, "ego_rg_attn", wrong)
    context = np.concatenate([ego_tok[:, 0], ego_ro[:, 0], ego_rg[:, 0]], axis=1)
    score = score / score.sum(-1, keepdims=True)
    out = head(sd, context, head_num_layers, C, clip_value, wrong)
    out.update(context=context, ego_attn_score=score)
    return out
