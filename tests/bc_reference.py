"""The BC policy (the reference's EarlyFusionAttnBCNet in eval mode) restated in float64 numpy from a state dict, in this
repository's own words: what gd_bc_forward and gd_bc_forward_dim are held to.  The width is the state dict's: for `network_dim`
D and head_dim 64 every embedder, LayerNorm and attention Linear is D wide, the 4 heads have D / 4 channels and q is scaled by
(D / 4)^-1/2, the context is 3 D wide, and the GMM head behind head.input_layer (3 D -> 64) is 64 wide at either width.
tests/test_bc_policy.py pins this restatement to the reference module itself at 64 (tests/golden/bc_forward_*.npz),
tests/test_bc_wide.py at 128 (tests/golden/bc_wide_forward_*.npz).

`wrong=` switches ONE rule to a plausible mistake, so that the tests can show the comparison catches it:
    "inf_fill"        masked keys are excluded (probability 0; a row with no key left gives a zero attention output) instead of
                      scoring -FLT_MAX, under which a row with every key masked attends uniformly
    "normed_residual" the attention residual adds the LayerNorm'ed input instead of the input
    "entity_major"    a token's R rows are taken by reshaping [R, n, k] to [n, R k] without the permute
    "tanh_gelu"       the tanh approximation of GELU instead of the erf form
and five that are the right rule at bc_cases.CFG and wrong only at the configurations of bc_cases.EDGE_CASES:
    "head_one_trip"   the head's outputs of index >= 64 stay at their bias (one trip of a 64-lane loop over the 7 C outputs)
    "rg_at_ro"        rg_attn layer i is read at ro_attn's offset (ro_attn layer i's weights) for i >= min(fusion, branch):
                      it needs branch > fusion to show (a model with one branch layer has no such i)
    "floor_m20"       the covariance clamp's floor is -20 whatever clip_value says
    "eval_one_trip"   `evaluate` sums the rows below 64 of a batch only (one trip of a 64-lane loop over the rows)
    "kin_three_tiles" the road embedder's first layer reads its inputs 0 .. 95 only (three 32-column tiles): every input for
                      num_stack <= 7 (13 R <= 91), wrong at num_stack 8 (kin 104, a fourth tile)
and four that the 128 case invites (the right rule at 64):
    "scale16"         q * 0.25, the 64-wide kernel's constant, instead of q * 32^-1/2
    "heads_of_16"     eight heads of 16 channels (the 64-wide head size kept) instead of four of 32
    "ctx192"          the head reads the first 192 context inputs only (the 64-wide CTX kept)
    "ln64"            LayerNorm statistics over the first 64 features only (one lane per feature, one wave)"""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
COV_MAX = 3.58352
ROADS, EGO_K, PARTNER_K, ROAD_K, DIM, HEADS = 200, 6, 6, 13, 64, 4  # DIM: the narrow width, and the GMM head's at either
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _sd64(sd):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for k, v in sd.items()}


def layer_norm(x, sd, name, wrong=None):
    stat = x[..., :64] if wrong == "ln64" else x
    mean = stat.mean(-1, keepdims=True)
    var = ((stat - mean) ** 2).mean(-1, keepdims=True)  # biased
    return (x - mean) / np.sqrt(var + 1e-5) * sd[name + ".weight"] + sd[name + ".bias"]


def linear(x, sd, name):
    return x @ sd[name + ".weight"].T + sd[name + ".bias"]


def gelu(x, wrong=None):
    if wrong == "tanh_gelu":
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def unpack(obs, A, wrong=None):
    """obs [B, R, D] -> ego [B, 6 R], partners [B, A - 1, 6 R], roads [B, 200, 13 R]: time is the slow index inside a token."""
    B, R, _ = obs.shape
    ego = obs[:, :, :EGO_K].reshape(B, R * EGO_K)
    out = [ego]
    at = EGO_K
    for n, k in ((A - 1, PARTNER_K), (ROADS, ROAD_K)):
        x = obs[:, :, at:at + n * k].reshape(B, R, n, k)
        at += n * k
        out.append(x.reshape(B, n, R * k) if wrong == "entity_major" else x.transpose(0, 2, 1, 3).reshape(B, n, R * k))
    return out


def embed(x, sd, net, wrong=None):
    for i in range(4):  # Linear -> [dropout: identity] -> LayerNorm -> tanh
        if wrong == "kin_three_tiles" and i == 0 and net == "road_graph_net" and x.shape[-1] > 96:
            y = x[..., :96] @ sd[net + ".0.weight"][:, :96].T + sd[net + ".0.bias"]
        else:
            y = linear(x, sd, "%s.%d" % (net, 4 * i))
        x = np.tanh(layer_norm(y, sd, "%s.%d" % (net, 4 * i + 2), wrong))
    return x


def attention(xq, xkv, mask, sd, name, wrong=None):
    """xq [B, N, D], xkv [B, J, D] (both already normed), mask [B, J] bool (True: padding).  Returns (o_proj output
    [B, N, D], the attention probabilities [B, 4, N, J])."""
    B, N, D = xq.shape
    J = xkv.shape[1]
    heads = D // 16 if wrong == "heads_of_16" else HEADS
    ch = D // heads
    split = lambda t, n: t.reshape(B, n, heads, ch).transpose(0, 2, 1, 3)  # noqa: E731
    q = split(linear(xq, sd, name + ".q_proj"), N) * (0.25 if wrong == "scale16" else ch ** -0.5)
    k = split(linear(xkv, sd, name + ".k_proj"), J)
    v = split(linear(xkv, sd, name + ".v_proj"), J)
    s = np.einsum("bhic,bhjc->bhij", q, k)
    m = np.broadcast_to(mask[:, None, None, :], s.shape)
    if wrong == "inf_fill":
        s = np.where(m, -np.inf, s)
        top = s.max(-1, keepdims=True)
        e = np.where(m, 0.0, np.exp(s - np.where(np.isfinite(top), top, 0.0)))
        tot = e.sum(-1, keepdims=True)
        p = e / np.where(tot > 0, tot, 1.0)
    else:
        s = np.where(m, -FLT_MAX, s)
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    o = np.einsum("bhij,bhjc->bhic", p, v).transpose(0, 2, 1, 3).reshape(B, N, D)
    return linear(o, sd, name + ".o_proj"), p


def mlp(x, sd, name, wrong=None):
    z = linear(layer_norm(x, sd, name + ".0", wrong), sd, name + ".1")
    return x + linear(gelu(z, wrong), sd, name + ".3")


def self_layer(x, mask, sd, name, wrong=None):
    h = layer_norm(x, sd, name + ".0.module.norm", wrong)
    o, _ = attention(h, h, mask, sd, name + ".0.module.attention", wrong)
    x = o + (h if wrong == "normed_residual" else x)
    return mlp(x, sd, name + ".1.module", wrong)


def cross_layer(xq, xkv, mask, sd, name, wrong=None):
    q = layer_norm(xq, sd, name + ".0.module.q_norm", wrong)
    kv = layer_norm(xkv, sd, name + ".0.module.kv_norm", wrong)
    o, p = attention(q, kv, mask, sd, name + ".0.module.attention", wrong)
    x = o + (q if wrong == "normed_residual" else xq)
    return mlp(x, sd, name + ".1.module", wrong), p[:, :, 0, :]


def clamp_logcov(raw, clip_value):
    return np.minimum(np.maximum(raw, clip_value), COV_MAX)


def forward(sd, obs, partner_mask, road_mask, max_agents, num_layer, head_num_layers, n_components, clip_value, wrong=None):
    """Everything the module computes for a batch, float64; the width is the state dict's: context [B, 3 D], ego_attn_score
    [B, 4, A - 1], raw [B, 7 C], means and log_covariances and covariances [B, C, 3], weights [B, C]."""
    sd = _sd64(sd)
    obs = np.asarray(obs, dtype=np.float64)
    A, C = max_agents, n_components
    B = obs.shape[0]
    pm = np.asarray(partner_mask).astype(bool)[:, -1]
    rm = np.asarray(road_mask).astype(bool)[:, -1]
    ego, ro, rg = unpack(obs, A, wrong)
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
        blk = "ro_attn" if wrong == "rg_at_ro" and i >= min(num_layer) else "rg_attn"
        roads = self_layer(roads, rm, sd, "%s.%d" % (blk, i), wrong)
    ego_tok = objs[:, :1]
    ego_ro, score = cross_layer(ego_tok, objs[:, 1:], pm, sd, "ego_ro_attn", wrong)
    ego_rg, _ = cross_layer(ego_tok, roads, rm, sd, "ego_rg_attn", wrong)
    context = np.concatenate([ego_tok[:, 0], ego_ro[:, 0], ego_rg[:, 0]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = score / score.sum(-1, keepdims=True)
    out = head(sd, context, head_num_layers, C, clip_value, wrong)
    out.update(context=context, ego_attn_score=score)
    return out


def head(sd, context, head_num_layers, C, clip_value, wrong=None):
    sd = _sd64(sd)
    w, b = sd["head.input_layer.0.weight"], sd["head.input_layer.0.bias"]
    x = np.maximum((context[:, :192] @ w[:, :192].T if wrong == "ctx192" else context @ w.T) + b, 0.0)
    for i in range(head_num_layers):
        x = x + np.maximum(linear(x, sd, "head.residual_block.%d.0" % i), 0.0)
    raw = linear(x, sd, "head.head")
    if wrong == "head_one_trip":
        raw[:, 64:] = sd["head.head.bias"][64:]
    return mixture(raw, C, -20.0 if wrong == "floor_m20" else clip_value)


def mixture(raw, C, clip_value):
    """The rule's mixture parameters from the head's raw outputs [B, 7 C] (csrc/bc_rule.hpp)."""
    raw = np.asarray(raw, dtype=np.float64)
    B = raw.shape[0]
    means = raw[:, :3 * C].reshape(B, C, 3)
    logcov = clamp_logcov(raw[:, 3 * C:6 * C], clip_value).reshape(B, C, 3)
    w = raw[:, 6 * C:]
    e = np.exp(w - w.max(-1, keepdims=True))
    return dict(raw=raw, means=means, log_covariances=logcov, covariances=np.exp(logcov), weights=e / e.sum(-1, keepdims=True))


def deterministic_action(means, weights):
    """(component, action [B, 3]): the mean of the FIRST component of maximal weight."""
    c = np.argmax(weights, axis=-1)  # numpy's argmax returns the first maximum
    return c, means[np.arange(len(c)), c]


def running_sums(weights):
    return np.cumsum(np.asarray(weights, dtype=np.float64), axis=-1)


def sampled_action(means, covariances, weights, u, z):
    """(component, action): the first k whose running weight sum exceeds u, the last if none does; mean + sqrt(cov) z."""
    run = running_sums(weights)
    over = run > np.asarray(u, dtype=np.float64)[:, None]
    c = np.where(over.any(-1), over.argmax(-1), weights.shape[-1] - 1)
    r = np.arange(len(c))
    return c, means[r, c] + np.sqrt(covariances[r, c]) * np.asarray(z, dtype=np.float64)


def nll(means, log_covariances, weights, expert):
    """gmm_loss's per-row value in closed form; expert [B, 3]."""
    a = np.asarray(expert, dtype=np.float64).reshape(-1, 1, 3)
    lp = (-0.5 * ((a - means) ** 2 / np.exp(log_covariances)).sum(-1) - 0.5 * log_covariances.sum(-1)
          - 1.5 * math.log(2.0 * math.pi))
    wl = lp + np.log(weights + 1e-8)
    M = wl.max(-1, keepdims=True)
    return -(M[:, 0] + np.log(np.exp(wl - M).sum(-1)))


def evaluate_sums(batches, wrong=None):
    """evaluate()'s running sums, float64 [11]: the sum over batches of the batch's mean nll [0] and mean |pred - expert| per
    dimension [1..3]; the sums of |pred - expert| over the rows whose expert magnitude exceeds the dimension's threshold [4..6]
    and their counts [7..9]; the number of batches [10]."""
    thr = tuple(float(np.float32(v)) for v in (2.0, 0.035, 0.023))  # torch compares a float32 tensor with the scalar in float32
    acc = np.zeros(11)
    for row_nll, pred, expert in batches:
        n = len(row_nll)
        keep = slice(0, 64 if wrong == "eval_one_trip" else n)
        expert = np.asarray(expert, np.float64)[keep]
        err = np.abs(np.asarray(pred, np.float64)[keep] - expert)
        acc[0] += float(np.sum(np.asarray(row_nll, np.float64)[keep])) / n
        acc[1:4] += err.sum(0) / n
        for k in range(3):
            big = np.abs(expert[:, k]) > thr[k]
            acc[4 + k] += err[big, k].sum()
            acc[7 + k] += big.sum()
        acc[10] += 1
    return acc


def evaluate(batches, wrong=None):
    """The reference's evaluate() (baselines/il/il.py:99-180) from per-batch (nll [B], predicted [B, 3], expert [B, 3]): its eight
    numbers.  Per-batch means averaged over batches; the std2 figures are global sums over global counts."""
    a = evaluate_sums(batches, wrong)
    nb = a[10]
    with np.errstate(invalid="ignore", divide="ignore"):
        return [a[0] / nb, a[1] / nb, a[2] / nb, a[3] / nb, a[4] / a[7], a[5] / a[8], a[6] / a[9], 0.0]
