"""Float64 numpy statement of the device policy forward (gd_policy_forward): the late-fusion actor-critic in eval mode from a
state dict, and the action rule given logits.  No torch module, no pufferlib: test infrastructure for test_policy.py and
test_gpu_policy.py."""
import numpy as np

ROADS, ROAD_K, PARTNER_K = 200, 13, 6
LN_EPS = 1e-5


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def _embed(sd, name, x):
    """Linear, LayerNorm (biased variance, affine), tanh, [dropout: identity], Linear over the last axis of x."""
    w1, b1 = _np(sd[name + ".0.weight"]), _np(sd[name + ".0.bias"])
    g, b = _np(sd[name + ".1.weight"]), _np(sd[name + ".1.bias"])
    w2, b2 = _np(sd[name + ".4.weight"]), _np(sd[name + ".4.bias"])
    h = x @ w1.T + b1
    mean = h.mean(-1, keepdims=True)
    var = ((h - mean) ** 2).mean(-1, keepdims=True)
    h = (h - mean) * (1.0 / np.sqrt(var + LN_EPS)) * g + b
    return np.tanh(h) @ w2.T + b2


def forward(sd, obs, max_agents, ego_width):
    """(logits [N, n_actions], value [N], features [N, 192]) in float64.  The max-pools run over all A - 1 partner rows and
    all 200 road rows: nothing is masked."""
    obs = _np(obs)
    n = obs.shape[0]
    p0 = ego_width
    r0 = p0 + PARTNER_K * (max_agents - 1)
    assert obs.shape[1] == r0 + ROAD_K * ROADS
    ego = _embed(sd, "ego_embed", obs[:, :p0])
    partner = _embed(sd, "partner_embed", obs[:, p0:r0].reshape(n, max_agents - 1, PARTNER_K)).max(1)
    road = _embed(sd, "road_map_embed", obs[:, r0:].reshape(n, ROADS, ROAD_K)).max(1)
    feat = np.concatenate([ego, partner, road], 1)
    hidden = feat @ _np(sd["shared_embed.0.weight"]).T + _np(sd["shared_embed.0.bias"])
    logits = hidden @ _np(sd["actor.weight"]).T + _np(sd["actor.bias"])
    value = (hidden @ _np(sd["critic.weight"]).T + _np(sd["critic.bias"]))[:, 0]
    return logits, value, feat


def cumulative(logits):
    """The float64 cumulative softmax [N, n] in ascending k."""
    l = np.asarray(logits, dtype=np.float64)
    p = np.exp(l - l.max(-1, keepdims=True))
    return np.cumsum(p, -1) / p.sum(-1, keepdims=True)


def action_rule(logits, u=None, deterministic=False):
    """(actions int64 [N], logprob [N], entropy [N]) of csrc/policy_rule.hpp in float64: the first k whose running sum of
    exp(l - m) in ascending k exceeds u * S (the last k if none does), or the first index of the maximum."""
    l = np.asarray(logits, dtype=np.float64)
    n, na = l.shape
    m = l.max(-1, keepdims=True)
    p = np.exp(l - m)
    run = np.cumsum(p, -1)
    S = run[:, -1:]
    if deterministic:
        a = np.argmax(l, -1)  # the first occurrence
    else:
        over = run > np.asarray(u, dtype=np.float64).reshape(n, 1) * S
        a = np.where(over.any(-1), over.argmax(-1), na - 1)
    q = l - m - np.log(S)
    logprob = q[np.arange(n), a]
    entropy = -(q * np.exp(q)).sum(-1)
    return a.astype(np.int64), logprob, entropy
