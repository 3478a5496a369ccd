"""Seeded state dicts, observations and uniforms for the device policy forward, the constructed cases, and the stand-in
module (plain torch.nn layers under the reference module's key names).  Test infrastructure for test_policy.py and
test_gpu_policy.py.

Weights are N(0, 1 / fan_in), the actor at the same scale, so that the logits spread over several units: with the reference's
std-0.01 actor every logit is ~0 and an error hides.  LayerNorm gains and biases are perturbed.  Observations are uniform in
[-1, 1] with zeroed columns and several all-zero (padding) entity rows."""
import os
import subprocess
import tempfile

import numpy as np
import torch
from torch import nn

from tests import policy_reference as REF

HERE = os.path.dirname(os.path.abspath(__file__))
ROADS, ROAD_K, PARTNER_K = REF.ROADS, REF.ROAD_K, REF.PARTNER_K
EMBEDDERS = ("ego_embed", "partner_embed", "road_map_embed")
SHAPES = [(n, a, ew, na) for n in (1, 3, 70) for a in (64, 128) for ew in (6, 9) for na in (91, 7)]
# The action counts at which the tiling of the heads changes -- (n_actions + 1 + 31) / 32 output tiles, the value being output
# n_actions, and [Wa; Wc] walked eight rows at a time in the backward: 1 (a softmax of one number), 8 (the critic's row opens a
# group of eight), 31 (the value is the last output of the one tile), 32 (the value sits alone in a second tile), 33, and 1024
# (33 tiles, the largest count the API takes).  n = 33 is one full wave of k_policy_tail and a single row.  Not a matrix: one
# list, with 1, 32 and 1024 at both n and (max_agents, ego_width) alternating.
EDGE_SHAPES = [(3, 64, 6, 1), (33, 128, 9, 1), (3, 128, 9, 32), (33, 64, 6, 32), (3, 64, 6, 1024), (33, 128, 9, 1024),
               (33, 64, 6, 8), (3, 128, 9, 33), (33, 64, 6, 31), (3, 128, 9, 31)]
EDGE_ACTIONS = sorted({s[3] for s in EDGE_SHAPES})


def obs_width(max_agents, ego_width):
    return ego_width + PARTNER_K * (max_agents - 1) + ROAD_K * ROADS


def state_dict(seed, ego_width, n_actions):
    rng = np.random.default_rng(seed)
    sd = {}

    def linear(name, out, inp):
        sd[name + ".weight"] = rng.normal(0.0, 1.0 / np.sqrt(inp), (out, inp))
        sd[name + ".bias"] = rng.normal(0.0, 0.1, (out,))

    for name, k in zip(EMBEDDERS, (ego_width, PARTNER_K, ROAD_K)):
        linear(name + ".0", 64, k)
        sd[name + ".1.weight"] = 1.0 + rng.normal(0.0, 0.2, (64,))
        sd[name + ".1.bias"] = rng.normal(0.0, 0.1, (64,))
        linear(name + ".4", 64, 64)
    linear("shared_embed.0", 128, 192)
    linear("actor", n_actions, 128)
    linear("critic", 1, 128)
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in sd.items()}


def observations(seed, n, max_agents, ego_width):
    rng = np.random.default_rng(seed)
    a1 = max_agents - 1
    obs = rng.uniform(-1.0, 1.0, (n, obs_width(max_agents, ego_width))).astype(np.float32)
    partners = obs[:, ego_width:ego_width + PARTNER_K * a1].reshape(n, a1, PARTNER_K)
    roads = obs[:, ego_width + PARTNER_K * a1:].reshape(n, ROADS, ROAD_K)
    partners[:, :, 4] = 0.0   # zeroed columns
    roads[:, :, 11] = 0.0
    obs[:, 2] = 0.0
    for i in range(n):        # padding rows: a tail of each set and a few in the middle
        partners[i, a1 - int(rng.integers(0, 9)):] = 0.0
        roads[i, ROADS - int(rng.integers(0, 40)):] = 0.0
        partners[i, rng.integers(0, a1, 3)] = 0.0
        roads[i, rng.integers(0, ROADS, 5)] = 0.0
    return obs


def uniforms(seed, n):
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def edge_uniforms(n):
    """Case (iv): u = 0 and u = the largest float32 below 1, alternating."""
    u = np.zeros(n, dtype=np.float32)
    u[1::2] = np.nextafter(np.float32(1), np.float32(0))
    if n == 1:
        u[0] = np.nextafter(np.float32(1), np.float32(0))
    return u


def clear_of_boundaries(logits, u, margin=1e-4):
    """u moved (deterministically, by 2.5 margins at a time) until it is at least `margin` from every value of the float64
    cumulative softmax, so that a float32 and a float64 evaluation of the rule agree on the action.  Zero stays zero."""
    c = REF.cumulative(logits)
    u = np.array(u, dtype=np.float32)
    for i in range(len(u)):
        while u[i] != 0 and np.abs(c[i] - np.float64(u[i])).min() < margin:
            u[i] = np.float32((np.float64(u[i]) + 2.5 * margin) % 1.0)
    return u


def negative_pool_state(sd):
    """Case (i): the second Linear's bias of each embedder is -5, so every pooled embedding is negative and an unmasked tail
    lane holding 0 would win the max."""
    sd = {k: v.clone() for k, v in sd.items()}
    for name in EMBEDDERS:
        sd[name + ".4.bias"].fill_(-5.0)
    return sd


def last_entity_wins(sd, obs, max_agents, ego_width, feature=0):
    """Case (ii): in every row, the partner row and the road row that attain the pooled maximum of `feature` are swapped with
    the LAST partner (index A - 2) and with road 199, which then alone attain it (rows within 1e-3 of the winner are
    overwritten first).  Returns the new observations."""
    obs = np.array(obs, dtype=np.float32)
    n, a1 = obs.shape[0], max_agents - 1
    p0, r0 = ego_width, ego_width + PARTNER_K * a1
    for name, lo, hi, cnt, k in (("partner_embed", p0, r0, a1, PARTNER_K), ("road_map_embed", r0, obs.shape[1], ROADS, ROAD_K)):
        rows = obs[:, lo:hi].reshape(n, cnt, k)
        for i in range(n):
            emb = REF._embed(sd, name, rows[i].astype(np.float64))[:, feature]
            best = int(emb.argmax())
            close = emb > emb[best] - 1e-3  # rivals (copies of the winner among the padding rows, near ties) take the loser's row
            close[best] = False
            rows[i, close] = rows[i, int(emb.argmin())]
            rows[i, [best, cnt - 1]] = rows[i, [cnt - 1, best]]
            emb = REF._embed(sd, name, rows[i].astype(np.float64))[:, feature]
            assert emb.argmax() == cnt - 1 and (emb[:-1] < emb[-1] - 1e-4).all(), "case (ii) needs a clear winner"
        obs[:, lo:hi] = rows.reshape(n, -1)
    return obs


def tied_actor_state(sd, first=3, second=5, lift=10.0):
    """Case (iii): actor row `second` is a copy of row `first` and both biases are lifted, so the two logits are exactly equal
    and maximal in every row; `deterministic` must return `first`."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["actor.bias"][first] += lift
    sd["actor.weight"][second] = sd["actor.weight"][first]
    sd["actor.bias"][second] = sd["actor.bias"][first]
    return sd


class StandIn(nn.Module):
    """The late-fusion actor-critic out of plain torch.nn layers, under the reference module's key names."""

    def __init__(self, max_agents, ego_width, n_actions, dropout=0.01):
        super().__init__()
        self.max_agents, self.ego_width = max_agents, ego_width

        def embed(k):
            return nn.Sequential(nn.Linear(k, 64), nn.LayerNorm(64), nn.Tanh(), nn.Dropout(dropout), nn.Linear(64, 64))

        self.ego_embed, self.partner_embed, self.road_map_embed = embed(ego_width), embed(PARTNER_K), embed(ROAD_K)
        self.shared_embed = nn.Sequential(nn.Linear(192, 128), nn.Dropout(dropout))
        self.actor, self.critic = nn.Linear(128, n_actions), nn.Linear(128, 1)

    def forward(self, obs):
        n, p0 = obs.shape[0], self.ego_width
        r0 = p0 + PARTNER_K * (self.max_agents - 1)
        ego = self.ego_embed(obs[:, :p0])
        partner, _ = self.partner_embed(obs[:, p0:r0].view(n, self.max_agents - 1, PARTNER_K)).max(dim=1)
        road, _ = self.road_map_embed(obs[:, r0:].view(n, ROADS, ROAD_K)).max(dim=1)
        hidden = self.shared_embed(torch.cat([ego, partner, road], dim=1))
        return self.actor(hidden), self.critic(hidden)


def stand_in_forward(sd, obs, max_agents, ego_width, dtype):
    """(logits, value [N]) of the stand-in module in eval mode on the CPU, in `dtype`, as float64 numpy."""
    net = StandIn(max_agents, ego_width, sd["actor.weight"].shape[0]).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    net.eval()
    with torch.no_grad():
        logits, value = net(torch.from_numpy(np.asarray(obs)).to(dtype))
    return logits.double().numpy(), value.double().numpy()[:, 0]


_HOST = {}


def rule_host(sanitize=False):
    """The host program of csrc/policy_rule.hpp, compiled once per session with g++ (no contraction).  sanitize: a second,
    stand-alone executable with -fsanitize=address,undefined."""
    if sanitize not in _HOST:
        out = os.path.join(tempfile.gettempdir(), "gd_policy_rule_host%s_%d" % ("_san" if sanitize else "", os.getuid()))
        src = os.path.join(HERE, "policy_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "policy_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
            subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out, src])
        _HOST[sanitize] = out
    return _HOST[sanitize]


def run_rule_host(logits, u, deterministic, sanitize=False):
    """(actions int64, logprob f32, entropy f32) of the host program on float32 logits [N, n] and uniforms [N]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    n, na = logits.shape
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, na, int(deterministic)], dtype=np.int32).tobytes() + logits.tobytes() + u.tobytes())
        subprocess.check_call([rule_host(sanitize), fin, fout])
        raw = open(fout, "rb").read()
    assert len(raw) == 16 * n
    return (np.frombuffer(raw, np.int64, n), np.frombuffer(raw, np.float32, n, 8 * n), np.frombuffer(raw, np.float32, n, 12 * n))
