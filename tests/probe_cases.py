"""Cases for the device linear probe: a seeded head, seeded labels and masks with the constructed batches of the issue (no
row selected, one row selected, a sample whose partners are all masked, a label out of range) on top of bc_cases.inputs, the
float32 yardstick built from bc_cases.StandIn's own layers, and the host program of csrc/lp_rule.hpp."""
import os
import subprocess
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

from . import bc_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = 64
EXPS = ("other", "ego")
TAPS = ("fusion_attn", "ro_attn")
TAP_OF = {"early_lp": "fusion_attn", "late_lp": "ro_attn"}
GOLDEN_SHAPES = ((3, 64, 1), (2, 128, 5))
BASELINE_SHAPES = ((3, 64, 1), (17, 64, 5))
PART_INTS, N_HEAD = 392, 8
STATS = ("loss", "accuracy", "f1_macro", "ood_loss_sum", "ood_correct", "ood_rows", "rows", "bad_labels")


def head(K=64, seed=3):
    """'head.weight' [64, K] and 'head.bias' [64] float32: logits of standard deviation about 2, so rows have a clear maximum
    but no class is certain."""
    rng = np.random.default_rng([seed, K])
    w = rng.standard_normal((CLASSES, K)) * (2.0 / np.sqrt(K)) * (1.0 if K == 64 else 2.0)
    b = 0.2 * rng.standard_normal(CLASSES)
    return {"head.weight": torch.from_numpy(w.astype(np.float32)), "head.bias": torch.from_numpy(b.astype(np.float32))}


def row_shape(B, A, exp):
    return (B, A - 1) if exp == "other" else (B,)


def labels(B, A, exp, kind="plain", seed=5):
    """(mask bool, labels int64) in the dataset's own convention: for 'other' aux_mask [B, A - 1], True where the row is NOT
    used; for 'ego' future_valid_mask [B], True where it IS.  kind:
      plain  about half the rows selected; with B >= 2 sample 1 selects nothing (all its partners masked / not valid)
      empty  no row selected (M = 0)
      one    exactly one row selected (M = 1): the last row of the batch
      bad    plain, with the label of the first selected row 64 and, where more than two are selected, of the last one -3"""
    rng = np.random.default_rng([seed, B, A, EXPS.index(exp)])
    shape = row_shape(B, A, exp)
    use = rng.random(shape) < 0.5
    lab = rng.integers(0, CLASSES, shape).astype(np.int64)
    if exp == "ego":
        use[0] = True
    else:
        use[0, 0], use[0, -1] = True, True   # the first and the last partner column: both ends of the offset tiles
    if B >= 2:
        use[1] = False
    if B >= 3 or exp == "other":
        use.reshape(-1)[-1] = True
    if kind == "empty":
        use[...] = False
    elif kind == "one":
        use[...] = False
        use.reshape(-1)[-1] = True
    elif kind == "bad":
        at = np.flatnonzero(use.reshape(-1))
        lab.reshape(-1)[at[0]] = 64
        if len(at) > 2:
            lab.reshape(-1)[at[-1]] = -3
    else:
        assert kind == "plain"
    mask = ~use if exp == "other" else use
    return np.ascontiguousarray(mask), lab


def selected(mask, exp):
    return ~mask if exp == "other" else mask.copy()


def standin_taps(sd, obs, pm, rm, A, dtype=torch.float32, cfg=BC.CFG):
    """Both taps by bc_cases.StandIn's own layers in one dtype on the CPU: {tap: [B, A, 64] float64 numpy}, and under (tap, i)
    the same tokens after layer i of the block."""
    s = BC.StandIn(sd, A, cfg, dtype, "cpu")
    with torch.no_grad():
        o = torch.from_numpy(obs).to(dtype)
        B, R, _ = o.shape
        pmt, rmt = torch.from_numpy(pm)[:, -1].bool(), torch.from_numpy(rm)[:, -1].bool()
        ego = o[..., :6].reshape(B, R * 6)
        ro = o[..., 6:6 + 6 * (A - 1)].view(B, R, A - 1, 6).permute(0, 2, 1, 3).reshape(B, A - 1, R * 6)
        rg = o[..., 6 + 6 * (A - 1):].view(B, R, BC.ROADS, 13).permute(0, 2, 1, 3).reshape(B, BC.ROADS, R * 13)
        x = torch.cat([s._embed(ego, "ego_state_net").unsqueeze(1), s._embed(ro, "road_object_net"), s._embed(rg, "road_graph_net")], 1)
        ego_mask = torch.zeros(B, 1, dtype=torch.bool)
        all_mask, obj_mask = torch.cat([ego_mask, pmt, rmt], -1), torch.cat([ego_mask, pmt], -1)
        out = {}
        for i in range(cfg["num_layer"][0]):
            x = s._self(x, all_mask, "fusion_attn.%d" % i)
            out[("fusion_attn", i)] = x[:, :A].double().numpy().copy()
        out["fusion_attn"] = x[:, :A].double().numpy().copy()
        objs = x[:, :A]
        for i in range(cfg["num_layer"][1]):
            objs = s._self(objs, obj_mask, "ro_attn.%d" % i)
            out[("ro_attn", i)] = objs.double().numpy().copy()
        out["ro_attn"] = objs.double().numpy().copy()
    return out


def float32_head(x, hd, mask, lab, exp):
    """torch's float32 CPU run of the head on float32 rows x [N, K] (the yardstick's last step): logits, and the gradient of the
    mean cross-entropy over the selected rows with a label in range, as float64 numpy (grad None when no row is left)."""
    w = hd["head.weight"].clone().requires_grad_(True)
    b = hd["head.bias"].clone().requires_grad_(True)
    z = F.linear(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), w, b)
    use = selected(mask, exp).reshape(-1) & (lab.reshape(-1) >= 0) & (lab.reshape(-1) < CLASSES)
    grad = None
    if use.any():
        u = torch.from_numpy(use)
        F.cross_entropy(z[u], torch.from_numpy(lab.reshape(-1))[u]).backward()
        grad = np.concatenate([w.grad.double().numpy().reshape(-1), b.grad.double().numpy()])
    return z.detach().double().numpy(), grad


_HOST = [None]


def rule_host():
    """The host program of csrc/lp_rule.hpp, compiled once per session with g++ (no contraction)."""
    if _HOST[0] is None:
        out = os.path.join(tempfile.gettempdir(), "gd_lp_rule_host_%d" % os.getuid())
        src = os.path.join(HERE, "lp_rule_host.cpp")
        hdrs = [os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", n) for n in ("lp_rule.hpp", "bc_opt_rule.hpp", "ppo_rule.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, src])
        _HOST[0] = out
    return _HOST[0]


def _run(payload):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(payload)
        subprocess.check_call([rule_host(), fin, fout])
        return open(fout, "rb").read()


def host_rows(logits, lab, mask, exp):
    """The row rule and the batch (as one partial) on float32 logits [n, 64]."""
    z = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, CLASSES)
    n = z.shape[0]
    lab = np.ascontiguousarray(lab, dtype=np.int64).reshape(-1)
    m = np.ascontiguousarray(mask).astype(np.uint8).reshape(-1)
    assert lab.shape == (n,) and m.shape == (n,)
    buf = _run(np.array([0, n, EXPS.index(exp)], np.int32).tobytes() + z.tobytes() + lab.tobytes() + m.tobytes())
    per = 4 * 66
    rows = np.frombuffer(buf[:n * per], np.int32).reshape(n, 66)
    o = n * per
    hd5 = np.frombuffer(buf[o:o + 20], np.int32)
    cnt = np.frombuffer(buf[o + 20:o + 20 + 4 * 6 * 64], np.int32).reshape(6, 64)
    o += 20 + 4 * 6 * 64
    st = np.frombuffer(buf[o:o + 12], np.float32)
    d = np.frombuffer(buf[o + 12:o + 28], np.float64)
    return dict(pred=rows[:, 0].copy(), loss_row=rows[:, 1].view(np.float32).copy(), g=rows[:, 2:].view(np.float32).copy(),
                M=int(hd5[0]), correct=int(hd5[1]), bad=int(hd5[2]), ood_correct=int(hd5[3]), ood_rows=int(hd5[4]), counters=cnt.copy(),
                loss=st[0], accuracy=st[1], f1=st[2], loss_sum=float(d[0]), ood_loss_sum=float(d[1]))


def host_reduce(part_f, part_d, part_i, K=64):
    """The reduction of the partials: (M, grad [64 K + 64] float32, stats [8] float32)."""
    P = part_f.shape[0]
    GF = 64 * K + 64
    assert part_f.shape == (P, GF) and part_d.shape == (P, 2) and part_i.shape == (P, PART_INTS)
    buf = _run(np.array([1, P, K], np.int32).tobytes() + np.ascontiguousarray(part_f, dtype=np.float32).tobytes()
               + np.ascontiguousarray(part_d, dtype=np.float64).tobytes() + np.ascontiguousarray(part_i, dtype=np.int32).tobytes())
    return (int(np.frombuffer(buf[:4], np.int32)[0]), np.frombuffer(buf[4:4 + 4 * GF], np.float32).copy(),
            np.frombuffer(buf[4 + 4 * GF:], np.float32).copy())


def host_adamw(weight, exp_avg, exp_avg_sq, step, beta_pow, steps, lr, eps, weight_decay=0.01, betas=(0.9, 0.999), K=64):
    """steps: a list of (M, grad [64 K + 64] float32).  Returns (weight, exp_avg, exp_avg_sq, step, beta_pow)."""
    GF = 64 * K + 64
    parts = [np.array([2, K, len(steps)], np.int32).tobytes(), np.array([lr, eps, weight_decay], np.float32).tobytes(),
             np.array(betas, np.float64).tobytes()]
    parts += [np.ascontiguousarray(a, dtype=np.float32).reshape(GF).tobytes() for a in (weight, exp_avg, exp_avg_sq)]
    parts += [np.array([step], np.int32).tobytes(), np.ascontiguousarray(beta_pow, dtype=np.float64).tobytes()]
    for M, g in steps:
        parts += [np.array([M], np.int32).tobytes(), np.ascontiguousarray(g, dtype=np.float32).reshape(GF).tobytes()]
    buf = _run(b"".join(parts))
    f = np.frombuffer(buf[:12 * GF], np.float32).reshape(3, GF)
    return (f[0].copy(), f[1].copy(), f[2].copy(), int(np.frombuffer(buf[12 * GF:12 * GF + 4], np.int32)[0]),
            np.frombuffer(buf[12 * GF + 4:], np.float64).copy())
