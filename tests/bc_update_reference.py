"""The reference of the device BC update (gpudrive_lab_amd.bc_opt.DeviceBC; gd_bc_train_rows, gd_bc_adamw, gd_bc_update): the
reference's gradient step (baselines/il/il.py:267-303) on the CPU under torch -- the row statistics, `clip_grad_norm_(.., 20)`,
the reference's `get_grad_norm` restated, and `torch.optim.AdamW(foreach=False)` -- in float64 (the reference) and in float32
(the yardstick); the synthetic gradients of the real layout; the whole step of the differentiable stand-in
(tests/bc_grad_reference.py); and the driver of the host program of csrc/bc_opt_rule.hpp.  Test infrastructure for
test_bc_update.py and test_gpu_bc_update.py."""
import os
import subprocess
import tempfile

import numpy as np
import torch

from gpudrive_lab_amd import bc_policy as BP

from . import bc_cases as BC
from . import bc_grad_reference as GR
from .ppo_update_reference import error_floor, ratio_of  # noqa: F401  (the project's yardstick, shared)

HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ("loss", "dx_loss", "dy_loss", "dyaw_loss")
ADAMW = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01, max_norm=20.0)  # il.yaml, il.py:210, 286
ROWS = (1, 3, 257)


def layout(R=1, cfg=BC.CFG):
    """(names, tensor_end int32 [T], G) of the state dict's flat layout."""
    shapes = BP.expected_shapes(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"])
    end = np.cumsum([int(np.prod(s)) for s in shapes.values()]).astype(np.int32)
    return tuple(shapes), end, int(end[-1])


def zero_tensor(end, start=None):
    """The tensor the first gradient zeroes whole: a 64 x 64 weight a third of the way in (or the first from `start`)."""
    sizes = np.diff(np.concatenate([[0], end]))
    t = len(end) // 3 if start is None else start
    while sizes[t] != 64 * 64:
        t += 1
    return t


def gradients(end, seed=0, zero_from=None, largest=None):
    """Three gradients [G] float32, in the order of the steps: magnitudes 10^U(-8, 0), a norm far above 20, with one whole
    tensor of exact zeros (`zero_tensor(end, zero_from)`); magnitudes 10^U(-8, -3), a norm below 20 (the clip coefficient is
    exactly 1); magnitudes 10^U(-8, 0) again without zeros.  largest: a tensor index whose values are doubled (exact in
    float32) in all three, so that a tensor that is already among the largest has the largest norm by a factor."""
    G = int(end[-1])
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], G)  # noqa: E731
    big = (sign() * 10.0 ** rng.uniform(-8.0, 0.0, G)).astype(np.float32)
    small = (sign() * 10.0 ** rng.uniform(-8.0, -3.0, G)).astype(np.float32)
    holes = (sign() * 10.0 ** rng.uniform(-8.0, 0.0, G)).astype(np.float32)
    t = zero_tensor(end, zero_from)
    holes[(end[t - 1] if t else 0):end[t]] = 0.0
    if largest is not None:
        assert largest != t
        for g in (holes, small, big):
            g[end[largest - 1]:end[largest]] *= np.float32(2.0)
    return [holes, small, big]


SECOND_TRIP = 256  # k_bc_step's workgroup: tensors from this index on are loaded in its second trip


def top_gradients(end):
    """`gradients` for a layout of more than SECOND_TRIP tensors (bc_cases' `top`: 288): the tensor of zeros and the tensor of
    the largest norm (head.input_layer.0.weight, the largest tensor of all, doubled) both have an index >= SECOND_TRIP.
    Returns (gradients, zero tensor, largest tensor)."""
    sizes = np.diff(np.concatenate([[0], end]))
    largest = SECOND_TRIP + int(np.argmax(sizes[SECOND_TRIP:]))
    zt = zero_tensor(end, SECOND_TRIP)
    assert len(end) > SECOND_TRIP and zt >= SECOND_TRIP and sizes[largest] == sizes.max()
    return gradients(end, zero_from=SECOND_TRIP, largest=largest), zt, largest


def tensor_norms64(g, end):
    """The per-tensor L2 norms of a flat gradient, float64."""
    sq = np.asarray(g, dtype=np.float64) ** 2
    return np.sqrt(np.add.reduceat(sq, np.concatenate([[0], end[:-1]])))


def get_grad_norm(params):
    """The reference's `get_grad_norm` (il.py:59-68) restated: the largest per-tensor gradient norm, by a strict comparison
    from 0 in the parameters' order, and the index of the tensor that has it (None when every norm is 0)."""
    best, arg = 0.0, None
    for t, p in enumerate(params):
        n = float(p.grad.reshape(-1).norm(2))
        if n > best:
            best, arg = n, t
    return best, arg


def adamw_reference(params, grads, end, dtype, lr, betas, eps, weight_decay, max_norm, wrong=None):
    """Per step a dict of params, exp_avg, exp_avg_sq (flat float64 numpy), total (the norm before clipping), max_grad_norm and
    max_grad_tensor (get_grad_norm after the clip): torch's clip_grad_norm_ and AdamW(foreach=False) over the T tensors of the
    layout, on the CPU in `dtype`.  wrong="first_256": the tensors from SECOND_TRIP on are left out of the clip norm and out of
    the largest tensor norm (every gradient is still scaled by the coefficient and every parameter stepped) -- the right rule
    for a layout of at most SECOND_TRIP tensors."""
    assert wrong in (None, "first_256")
    cuts = [int(e) for e in end[:-1]]
    ps = [torch.nn.Parameter(torch.tensor(a).to(dtype)) for a in np.split(np.asarray(params), cuts)]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    flat = lambda ts: np.concatenate([t.detach().double().numpy().reshape(-1) for t in ts])  # noqa: E731
    seen = ps[:SECOND_TRIP] if wrong else ps
    out = []
    for g in grads:
        for p, a in zip(ps, np.split(np.asarray(g), cuts)):
            p.grad = torch.tensor(a).to(dtype)
        if wrong:
            total = torch.linalg.vector_norm(torch.stack([p.grad.reshape(-1).norm(2) for p in seen]), 2)
            coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
            for p in ps:
                p.grad.mul_(coef)
        else:
            total = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        best, arg = get_grad_norm(seen)
        opt.step()
        out.append(dict(params=flat(ps), exp_avg=flat([opt.state[p]["exp_avg"] for p in ps]),
                        exp_avg_sq=flat([opt.state[p]["exp_avg_sq"] for p in ps]), total=float(total.double()),
                        max_grad_norm=best, max_grad_tensor=arg))
    return out


def row_inputs(n, seed=3):
    """(nll [n], actions [n, 3], expert [n, 3]) float32, seeded: nll of both signs over three decades, actions and experts at
    the scales of the three action dimensions."""
    rng = np.random.default_rng([seed, n])
    nll = (rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-1.0, 2.0, n)).astype(np.float32)
    scale = np.array([3.0, 0.05, 0.03])
    return nll, (rng.normal(0.0, 1.0, (n, 3)) * scale).astype(np.float32), (rng.normal(0.0, 1.0, (n, 3)) * scale).astype(np.float32)


def rows_reference(nll, actions, expert, dtype):
    """(loss, dx, dy, dyaw) as float64 numpy [4] and the upstream gradient of loss.mean() [n], in `dtype` under autograd."""
    x = torch.tensor(np.asarray(nll)).to(dtype).requires_grad_(True)
    loss = x.mean()
    loss.backward()
    err = torch.abs(torch.tensor(np.asarray(actions)).to(dtype) - torch.tensor(np.asarray(expert)).to(dtype))
    stats = [loss.detach()] + [err[..., d].mean() for d in range(3)]
    return np.array([float(s.double()) for s in stats]), x.grad.double().numpy()


def pipeline(c, A, cfg, dtype=torch.float64, steps=1, **adamw):
    """The reference's whole step on the CPU in `dtype`: the differentiable stand-in's nll on the case c (sd, obs, pm, rm,
    expert), .mean(), clip_grad_norm_, AdamW.  Returns (parameters after the last step by name as float64 numpy, the loss of
    every step)."""
    ad = dict(ADAMW, **adamw)
    net = GR.Net(c["sd"], A, cfg, dtype)
    params = list(net.params.values())
    opt = torch.optim.AdamW(params, lr=ad["lr"], betas=ad["betas"], eps=ad["eps"], weight_decay=ad["weight_decay"], foreach=False)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = net.nll(c["obs"], c["pm"], c["rm"], c["expert"]).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, ad["max_norm"], foreach=False)
        opt.step()
        losses.append(float(loss.detach()))
    return {k: v.detach().double().numpy() for k, v in net.params.items()}, losses


# ---- the rule's host program

_HOST = [None]


def rule_host():
    if _HOST[0] is None:
        out = os.path.join(tempfile.gettempdir(), "gd_bc_opt_rule_host_%d" % os.getuid())
        src = os.path.join(HERE, "bc_opt_rule_host.cpp")
        hdrs = [os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", h) for h in ("bc_opt_rule.hpp", "ppo_rule.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, [src] + hdrs)):
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


def run_rows_host(nll, actions, expert):
    """(the four statistics, grad_nll [n]) float32 of the host program."""
    n = len(nll)
    raw = _run("rows", np.array([n], dtype=np.int32).tobytes() +
               b"".join(np.ascontiguousarray(t, dtype=np.float32).tobytes() for t in (nll, actions, expert)))
    assert len(raw) == 4 * (4 + n)
    a = np.frombuffer(raw, np.float32)
    return a[:4], a[4:]


def run_adamw_host(params, exp_avg, exp_avg_sq, grads, end, lr, betas, eps, weight_decay, max_norm, step=0, beta_pow=(1.0, 1.0)):
    """Per step a dict of the host program's params, exp_avg, exp_avg_sq [G] and tensor_norms [T] float32, total and
    max_grad_norm (float32), step and max_grad_tensor (int) and beta_pow [2] float64.  lr, eps, weight_decay and max_norm are
    rounded to float32, as the device holds them."""
    G, T = len(params), len(end)
    raw = _run("adamw", np.array([G, T, len(grads), step], dtype=np.int32).tobytes() +
               np.array([max_norm, eps, lr, weight_decay], dtype=np.float32).tobytes() +
               np.array([betas[0], betas[1], beta_pow[0], beta_pow[1]], dtype=np.float64).tobytes() +
               np.ascontiguousarray(end, dtype=np.int32).tobytes() +
               b"".join(np.ascontiguousarray(t, dtype=np.float32).tobytes() for t in [params, exp_avg, exp_avg_sq] + list(grads)))
    per = 12 * G + 4 * T + 16 + 16
    assert len(raw) == per * len(grads)
    out = []
    for s in range(len(grads)):
        b = raw[s * per:(s + 1) * per]
        f = np.frombuffer(b[:12 * G + 4 * T + 8], np.float32)
        i = np.frombuffer(b[12 * G + 4 * T + 8:12 * G + 4 * T + 16], np.int32)
        out.append({"params": f[:G], "exp_avg": f[G:2 * G], "exp_avg_sq": f[2 * G:3 * G], "tensor_norms": f[3 * G:3 * G + T],
                    "total": f[3 * G + T], "max_grad_norm": f[3 * G + T + 1], "step": int(i[0]), "max_grad_tensor": int(i[1]),
                    "beta_pow": np.frombuffer(b[12 * G + 4 * T + 16:], np.float64)})
    return out
