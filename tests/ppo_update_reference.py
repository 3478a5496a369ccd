"""The reference of the device PPO update (gpudrive_lab_amd.ppo.DevicePPO; gd_ppo_loss, gd_ppo_adam, gd_ppo_update): the
reference's minibatch loss (gpudrive/integrations/puffer/ppo.py:282-324) under torch autograd, `clip_grad_norm_` and
`torch.optim.Adam(foreach=False)` on the CPU, in float64 (the reference) and in float32 (the yardstick); the seeded inputs with
their gap condition; and the host program of csrc/ppo_rule.hpp.  Test infrastructure for test_ppo_update.py and
test_gpu_ppo_update.py."""
import os
import subprocess
import tempfile

import numpy as np
import torch

from tests import policy_grad_reference as GR

HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ("policy_loss", "value_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac")
HYPER = dict(clip_coef=0.2, vf_clip_coef=0.2, ent_coef=0.01, vf_coef=0.5)  # `policy_grad_reference.ppo_loss`'s
ROWS = (2, 3, 70, 257, 1025)
FLAGS = [(True, True), (True, False), (False, True), (False, False)]  # (norm_adv, clip_vloss)
GAP = 1e-3
# the seed of `loss_inputs` per M: the first one whose rows all keep the gap condition (`assert_gaps`)
SEEDS = {}


def ppo_loss(newlogprob, entropy, newvalue, log_probs, adv, ret, val, clip_coef=0.2, vf_clip_coef=0.2, ent_coef=0.01,
             vf_coef=0.5, norm_adv=True, clip_vloss=True):
    """`policy_grad_reference.ppo_loss` with the reference's `clip_vloss` switch (ppo.py:306-317) and its six statistics
    (ppo.py:285-291, 337-342): returns (loss, [policy_loss, value_loss, entropy, old_approx_kl, approx_kl, clipfrac])."""
    logratio = newlogprob - log_probs.reshape(-1)
    ratio = logratio.exp()
    with torch.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > clip_coef).to(ratio.dtype).mean()
    adv = adv.reshape(-1)
    if norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg_loss1 = -adv * ratio
    pg_loss2 = -adv * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()
    newvalue = newvalue.view(-1)
    if clip_vloss:
        v_loss_unclipped = (newvalue - ret) ** 2
        v_clipped = val + torch.clamp(newvalue - val, -vf_clip_coef, vf_clip_coef)
        v_loss_clipped = (v_clipped - ret) ** 2
        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - ret) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - ent_coef * entropy_loss + v_loss * vf_coef
    return loss, [pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl, clipfrac]


def loss_inputs(m, seed=None):
    """(newlogprob, entropy, newvalue, old_logprob, old_value, adv, ret) [m] float32: seeded new values, the old ones by
    `policy_grad_reference.minibatch` (ratios near 0.61, 0.99, 1.65 and 1.01, old values 0.01 and 0.5 away), and every fifth
    row from row 1 on with old logprob EQUAL to the new one (ratio exactly 1)."""
    seed = SEEDS.get(m, 0) if seed is None else seed
    rng = np.random.default_rng(1000 * m + seed)
    nlp = (-0.1 - 2.0 * np.abs(rng.normal(0.0, 1.0, m))).astype(np.float32)
    ent = rng.uniform(0.5, 4.0, m).astype(np.float32)
    nv = rng.normal(0.0, 1.0, m).astype(np.float32)
    old_lp, adv, ret, old_v = GR.minibatch(seed, nlp, nv)
    old_lp[1::5] = nlp[1::5]
    return nlp, ent, nv, old_lp, old_v, adv, ret


def gaps(inputs, clip_coef=0.2, vf_clip_coef=0.2):
    """The smallest distances, in float64, of any row from a branch point of the loss: (|ratio - (1 +- clip)|,
    ||newvalue - old value| - vf_clip|, |v_loss_unclipped - v_loss_clipped| over the rows whose value clamp is active)."""
    nlp, _, nv, old_lp, old_v, _, ret = (np.asarray(t, dtype=np.float64) for t in inputs)
    ratio = np.exp(nlp - old_lp)
    g_ratio = np.minimum(np.abs(ratio - (1 - clip_coef)), np.abs(ratio - (1 + clip_coef))).min()
    d = nv - old_v
    g_clamp = np.abs(np.abs(d) - vf_clip_coef).min()
    active = np.abs(d) > vf_clip_coef
    vcl = old_v + np.clip(d, -vf_clip_coef, vf_clip_coef)
    branch = np.abs((nv - ret) ** 2 - (vcl - ret) ** 2)[active]
    return g_ratio, g_clamp, (branch.min() if active.any() else np.inf)


def assert_gaps(inputs, what, clip_coef=0.2, vf_clip_coef=0.2):
    """The condition on the inputs: no float32 rounding can flip a branch."""
    g = gaps(inputs, clip_coef, vf_clip_coef)
    assert min(g) > GAP, (what, "a row within %g of a branch point" % GAP, g)


def first_clear_seed(m, tries=200):
    for seed in range(tries):
        if min(gaps(loss_inputs(m, seed))) > GAP:
            return seed
    raise AssertionError("no seed keeps the gap condition at m = %d" % m)


SEEDS.update({2: 0, 3: 0, 70: 0, 257: 1, 1025: 0})


def loss_reference(inputs, dtype, norm_adv, clip_vloss, **hyper):
    """(d_logprob, d_entropy, d_value [m], the six statistics [6]) as float64 numpy: the loss in `dtype` under autograd."""
    hy = dict(HYPER, **hyper)
    ts = [torch.tensor(np.asarray(t)).to(dtype) for t in inputs]
    leaves = [t.requires_grad_(True) for t in ts[:3]]
    nlp, ent, nv = leaves
    old_lp, old_v, adv, ret = ts[3:]
    loss, stats = ppo_loss(nlp, ent, nv, old_lp, adv, ret, old_v, norm_adv=norm_adv, clip_vloss=clip_vloss, **hy)
    loss.backward()
    return [t.grad.double().numpy() for t in leaves] + [np.array([float(s.detach().double()) for s in stats])]


def error_floor(got, ref64, ref32):
    """(error, E): the maximum absolute error of `got` against float64, and the yardstick -- the float32 computation's own
    error against float64, floored at 2^-23 max |ref64|."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref64).max())
    E = max(float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max()), 2.0 ** -23 * float(np.abs(ref64).max()))
    return err, E


def ratio_of(err, E):
    return err / E if E > 0 else (0.0 if err == 0 else np.inf)


# ---- clip_grad_norm_ and Adam

ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_norm=0.5)


def adam_gradients(G, seed=0):
    """Three gradients [G] float32, in the order of the steps: magnitudes 10^U(-8, 0), a norm far above 0.5, with a block of
    exact zeros (`zero_block`); magnitudes 10^U(-8, -3), a norm below 0.5 (the clip coefficient is exactly 1); magnitudes
    10^U(-8, 0) again without zeros."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], G)  # noqa: E731
    big = (sign() * 10.0 ** rng.uniform(-8.0, 0.0, G)).astype(np.float32)
    small = (sign() * 10.0 ** rng.uniform(-8.0, -3.0, G)).astype(np.float32)
    holes = (sign() * 10.0 ** rng.uniform(-8.0, 0.0, G)).astype(np.float32)
    holes[zero_block(G)] = 0.0
    return [holes, small, big]


def zero_block(G):
    return slice(G // 3, G // 3 + 1000)


def adam_reference(params, grads, dtype, lr, betas, eps, max_norm):
    """Per step (params, exp_avg, exp_avg_sq as float64 numpy, the norm before clipping): torch's clip_grad_norm_ and
    Adam(foreach=False) on one flat CPU tensor of `dtype`."""
    p = torch.nn.Parameter(torch.tensor(np.asarray(params)).to(dtype))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    out = []
    for g in grads:
        p.grad = torch.tensor(np.asarray(g)).to(dtype)
        total = torch.nn.utils.clip_grad_norm_([p], max_norm, foreach=False)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().double().numpy().copy(), st["exp_avg"].double().numpy().copy(),
                    st["exp_avg_sq"].double().numpy().copy(), float(total.double())))
    return out


def pipeline(sd, max_agents, ego_width, obs, actions, winners, old, dtype, norm_adv, clip_vloss, adam=None, **hyper):
    """One whole update in `dtype` on the CPU: the stand-in at the given winners -> the loss -> clip_grad_norm_ -> Adam.
    old = (old_logprob, adv, ret, old_value).  Returns (parameters after the step, gradients before clipping), dicts of
    float64 numpy arrays under the state dict's names."""
    ad = dict(ADAM, **(adam or {}))
    net = GR.stand_in(sd, max_agents, ego_width, dtype)
    lp, ent, val, _, _ = GR.evaluate(net, obs, actions, winners)
    old_lp, adv, ret, old_v = (torch.tensor(np.asarray(t)).to(dtype) for t in old)
    loss, _ = ppo_loss(lp, ent, val, old_lp, adv, ret, old_v, norm_adv=norm_adv, clip_vloss=clip_vloss, **dict(HYPER, **hyper))
    opt = torch.optim.Adam(net.parameters(), lr=ad["lr"], betas=ad["betas"], eps=ad["eps"], foreach=False)
    opt.zero_grad()
    loss.backward()
    grads = {k: p.grad.double().numpy().copy() for k, p in net.named_parameters()}
    torch.nn.utils.clip_grad_norm_(net.parameters(), ad["max_norm"], foreach=False)
    opt.step()
    return {k: p.detach().double().numpy().copy() for k, p in net.named_parameters()}, grads


# ---- the rule's host program

_HOST = [None]


def rule_host():
    if _HOST[0] is None:
        out = os.path.join(tempfile.gettempdir(), "gd_ppo_rule_host_%d" % os.getuid())
        src = os.path.join(HERE, "ppo_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "ppo_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src, hdr])):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, src])
        _HOST[0] = out
    return _HOST[0]


def _run(mode, payload):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(payload)
        subprocess.check_call([rule_host(), mode, fin, fout])
        return open(fout, "rb").read()


def run_loss_host(inputs, norm_adv, clip_vloss, **hyper):
    """(d_logprob, d_entropy, d_value [m], the six statistics) float32 of the host program."""
    hy = dict(HYPER, **hyper)
    m = len(inputs[0])
    raw = _run("loss", np.array([m, int(norm_adv), int(clip_vloss)], dtype=np.int32).tobytes() +
               np.array([hy["clip_coef"], hy["vf_clip_coef"], hy["ent_coef"], hy["vf_coef"]], dtype=np.float32).tobytes() +
               b"".join(np.ascontiguousarray(t, dtype=np.float32).tobytes() for t in inputs))
    assert len(raw) == 4 * (3 * m + 6)
    a = np.frombuffer(raw, np.float32)
    return [a[:m], a[m:2 * m], a[2 * m:3 * m], a[3 * m:]]


def run_adam_host(params, exp_avg, exp_avg_sq, grads, lr, betas, eps, max_norm, step=0, beta_pow=(1.0, 1.0)):
    """Per step a dict of the host program's params, exp_avg, exp_avg_sq [G] float32, total (float32), step (int32) and
    beta_pow [2] float64.  lr, eps and max_norm are rounded to float32, as the device holds them."""
    G = len(params)
    raw = _run("adam", np.array([G, len(grads), step], dtype=np.int32).tobytes() +
               np.array([max_norm, eps, lr], dtype=np.float32).tobytes() +
               np.array([betas[0], betas[1], beta_pow[0], beta_pow[1]], dtype=np.float64).tobytes() +
               b"".join(np.ascontiguousarray(t, dtype=np.float32).tobytes() for t in [params, exp_avg, exp_avg_sq] + list(grads)))
    per = 12 * G + 4 + 4 + 16
    assert len(raw) == per * len(grads)
    out = []
    for s in range(len(grads)):
        b = raw[s * per:(s + 1) * per]
        f = np.frombuffer(b[:12 * G], np.float32)
        out.append({"params": f[:G], "exp_avg": f[G:2 * G], "exp_avg_sq": f[2 * G:],
                    "total": np.frombuffer(b[12 * G:12 * G + 4], np.float32)[0],
                    "step": int(np.frombuffer(b[12 * G + 4:12 * G + 8], np.int32)[0]),
                    "beta_pow": np.frombuffer(b[12 * G + 8:], np.float64)})
    return out
