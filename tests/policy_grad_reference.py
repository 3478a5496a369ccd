"""The reference of the device policy backward (gpudrive_lab_amd.policy.TrainablePolicy; gd_policy_evaluate and
gd_policy_backward): torch autograd on the CPU over the stand-in module of tests/policy_cases.py with dropout 0, the two
max-pools replaced by a `gather` at GIVEN winners, in float64 (the reference) and in float32 (the yardstick).  Also the
reference's own PPO loss (gpudrive/integrations/puffer/ppo.py:282-324), the constructed cases of the backward, and the host
program of csrc/policy_grad_rule.hpp.  Test infrastructure for test_policy_grad.py and test_gpu_policy_grad.py."""
import os
import subprocess
import tempfile

import numpy as np
import torch

from tests import policy_cases as PC
from tests import policy_reference as REF

HERE = os.path.dirname(os.path.abspath(__file__))
ROADS, ROAD_K, PARTNER_K = REF.ROADS, REF.ROAD_K, REF.PARTNER_K


def stand_in(sd, max_agents, ego_width, dtype):
    net = PC.StandIn(max_agents, ego_width, sd["actor.weight"].shape[0], dropout=0.0).to(dtype)
    net.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in sd.items()})
    return net


def evaluate(net, obs, actions, winners=None):
    """(logprob, entropy, value, partner embeddings [N, A-1, 64], road embeddings [N, 200, 64]) of the stand-in `net` as
    torch tensors with a graph.  winners: None for the plain max-pools, or [N, 128] (64 partner indices, then 64 road
    indices): feature j of a pool is then read at entity winners[j]."""
    dtype = net.actor.weight.dtype
    x = torch.as_tensor(np.asarray(obs)).to(dtype)
    n, p0 = x.shape[0], net.ego_width
    r0 = p0 + PARTNER_K * (net.max_agents - 1)
    ego = net.ego_embed(x[:, :p0])
    pe = net.partner_embed(x[:, p0:r0].reshape(n, net.max_agents - 1, PARTNER_K))
    re = net.road_map_embed(x[:, r0:].reshape(n, ROADS, ROAD_K))
    if winners is None:
        partner, road = pe.max(dim=1)[0], re.max(dim=1)[0]
    else:
        w = torch.as_tensor(np.asarray(winners)).long()
        partner, road = pe.gather(1, w[:, None, :64])[:, 0], re.gather(1, w[:, None, 64:])[:, 0]
    hidden = net.shared_embed(torch.cat([ego, partner, road], dim=1))
    logits, value = net.actor(hidden), net.critic(hidden)[:, 0]
    q = torch.log_softmax(logits, dim=-1)
    logprob = q.gather(1, torch.as_tensor(np.asarray(actions)).long()[:, None])[:, 0]
    entropy = -(q.exp() * q).sum(-1)
    return logprob, entropy, value, pe, re


def gradients(sd, obs, max_agents, ego_width, actions, ups, winners, dtype):
    """d/d(parameters) of sum_r (ups[0][r] logprob[r] + ups[1][r] entropy[r] + ups[2][r] value[r]) at the given winners,
    computed in `dtype`, as a dict of float64 numpy arrays under the state dict's names."""
    net = stand_in(sd, max_agents, ego_width, dtype)
    lp, ent, val, _, _ = evaluate(net, obs, actions, winners)
    d = [torch.as_tensor(np.asarray(u)).to(dtype) for u in ups]
    (d[0] * lp + d[1] * ent + d[2] * val).sum().backward()
    return {k: p.grad.double().numpy() for k, p in net.named_parameters()}


def yardstick(g64, g32):
    """E_p per tensor: the float32 computation's maximum absolute error against float64, floored at 2^-23 max |g64_p|."""
    return {k: max(float(np.abs(g32[k] - g64[k]).max()), 2.0 ** -23 * float(np.abs(g64[k]).max())) for k in g64}


def ppo_loss(newlogprob, entropy, newvalue, log_probs, adv, ret, val, clip_coef=0.2, vf_clip_coef=0.2, ent_coef=0.01,
             vf_coef=0.5, norm_adv=True):
    """The reference's minibatch loss, line for line (ppo.py:282-324, clip_vloss on), on torch tensors of any device and
    dtype."""
    logratio = newlogprob - log_probs.reshape(-1)
    ratio = logratio.exp()
    adv = adv.reshape(-1)
    if norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg_loss1 = -adv * ratio
    pg_loss2 = -adv * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()
    newvalue = newvalue.view(-1)
    v_loss_unclipped = (newvalue - ret) ** 2
    v_clipped = val + torch.clamp(newvalue - val, -vf_clip_coef, vf_clip_coef)
    v_loss_clipped = (v_clipped - ret) ** 2
    v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    return pg_loss - ent_coef * entropy.mean() + v_loss * vf_coef


def minibatch(seed, logprob, value):
    """Old logprobs, advantages, returns and old values [N] float32 around the given new logprob and value: the old logprobs
    are perturbed by +-0.5 and +-0.01 in turn, so that ratios fall both outside and inside the clip range 0.2 (whether a row
    clips then follows the sign of its advantage), and the old values likewise."""
    rng = np.random.default_rng(seed)
    n = len(logprob)
    step = np.array([0.5, 0.01, -0.5, -0.01])[np.arange(n) % 4]
    old_lp = (np.asarray(logprob, dtype=np.float64) + step).astype(np.float32)
    old_v = (np.asarray(value, dtype=np.float64) + np.roll(step, 1)).astype(np.float32)
    adv = rng.normal(0.0, 1.0, n).astype(np.float32)
    ret = (np.asarray(value, dtype=np.float64) + rng.normal(0.0, 0.5, n)).astype(np.float32)
    return old_lp, adv, ret, old_v


def ppo_upstream(seed, logprob, entropy, value):
    """The three upstream gradients [N] float32 of the reference's loss at the given (new) logprob, entropy and value, in
    float64 autograd.  For N = 1, where adv.std() is undefined, seeded gradients of size 1 / N instead."""
    n = len(logprob)
    if n == 1:
        return [np.random.default_rng(seed).normal(0.0, 1.0 / n, n).astype(np.float32) for _ in range(3)]
    old_lp, adv, ret, old_v = minibatch(seed, logprob, value)
    leaves = [torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True) for t in (logprob, entropy, value)]
    ppo_loss(*leaves, *(torch.tensor(np.asarray(t, dtype=np.float64)) for t in (old_lp, adv, ret, old_v))).backward()
    return [t.grad.numpy().astype(np.float32) for t in leaves]


# ---- the constructed cases (the numbering is the issue's)

def all_padding_partners(obs, max_agents, ego_width):
    """Case (iii): every partner row of every observation is zero."""
    obs = np.array(obs, dtype=np.float32)
    obs[:, ego_width:ego_width + PARTNER_K * (max_agents - 1)] = 0.0
    return obs


def copied_winner(sd, obs, max_agents, ego_width, feature=0):
    """Case (iv): in every row and both sets, the entity that attains the pooled maximum of `feature` (moved to index 0
    first if it is the last one) is copied over the LAST entity, so that two bit-identical rows attain the maximum; the
    winner must stay the lower index.  Returns (observations, the lower indices [N, 2])."""
    obs = np.array(obs, dtype=np.float32)
    n, a1 = obs.shape[0], max_agents - 1
    p0, r0 = ego_width, ego_width + PARTNER_K * a1
    low = np.zeros((n, 2), dtype=np.int64)
    for s, (name, lo, hi, cnt, k) in enumerate((("partner_embed", p0, r0, a1, PARTNER_K),
                                                 ("road_map_embed", r0, obs.shape[1], ROADS, ROAD_K))):
        rows = obs[:, lo:hi].reshape(n, cnt, k)
        for i in range(n):
            best = int(REF._embed(sd, name, rows[i].astype(np.float64))[:, feature].argmax())
            if best == cnt - 1:
                rows[i, [0, best]] = rows[i, [best, 0]]
                best = 0
            rows[i, cnt - 1] = rows[i, best]
            low[i, s] = best
        obs[:, lo:hi] = rows.reshape(n, -1)
    return obs, low


def lifted_actor_bias(sd, index=3, lift=120.0):
    """Case (v): one actor bias lifted by 120, so that every other action's expf underflows to zero."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["actor.bias"][index] += lift
    return sd


def first_identical_row(rows):
    """For entity rows [cnt, K]: per entity, the lowest index holding a bit-identical row."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    keys = [r.tobytes() for r in rows.view(np.int32)]
    first = {}
    return np.array([first.setdefault(k, i) for i, k in enumerate(keys)])


# ---- the rule's host program

_HOST = {}


def rule_host(sanitize=False):
    """The compiled host program; sanitize: a second, stand-alone executable with -fsanitize=address,undefined."""
    if sanitize not in _HOST:
        out = os.path.join(tempfile.gettempdir(), "gd_policy_grad_rule_host%s_%d" % ("_san" if sanitize else "", os.getuid()))
        src = os.path.join(HERE, "policy_grad_rule_host.cpp")
        hdrs = [os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", h) for h in ("policy_grad_rule.hpp", "policy_rule.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src] + hdrs)):
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
            subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out, src])
        _HOST[sanitize] = out
    return _HOST[sanitize]


def run_rule_host(logits, actions, d_logprob, d_entropy, sanitize=False):
    """dlogits [N, n] float32 of the host program."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n, na = logits.shape
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, na], dtype=np.int32).tobytes() + logits.tobytes() +
                    np.ascontiguousarray(actions, dtype=np.int32).tobytes() +
                    np.ascontiguousarray(d_logprob, dtype=np.float32).tobytes() +
                    np.ascontiguousarray(d_entropy, dtype=np.float32).tobytes())
        subprocess.check_call([rule_host(sanitize), fin, fout])
        raw = open(fout, "rb").read()
    assert len(raw) == 4 * n * na
    return np.frombuffer(raw, np.float32).reshape(n, na)


def rule64(logits, actions, d_logprob, d_entropy):
    """The rule in float64: dl[k] = d_logprob (1[k = a] - p[k]) - d_entropy p[k] (q[k] + H)."""
    l = np.asarray(logits, dtype=np.float64)
    n = len(l)
    q = l - l.max(-1, keepdims=True)
    q = q - np.log(np.exp(q).sum(-1, keepdims=True))
    p = np.exp(q)
    H = -(p * q).sum(-1, keepdims=True)
    hot = np.zeros_like(l)
    hot[np.arange(n), np.asarray(actions)] = 1.0
    return np.asarray(d_logprob, np.float64)[:, None] * (hot - p) - np.asarray(d_entropy, np.float64)[:, None] * p * (q + H)
