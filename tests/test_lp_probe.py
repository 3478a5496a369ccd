"""The device linear probe without a GPU: the host program of csrc/lp_rule.hpp against torch float64 (and sklearn where it is
installed), the float64 restatement (probe_reference.py) pinned to the reference's own modules
(tests/golden/lp_probe_*.npz, written by tools/lp_probe_golden.py), the surface, and every refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from gpudrive_lab_amd import lp_probe as LP

from . import bc_cases as BC
from . import probe_cases as PC
from . import probe_reference as PREF
from .test_bc_policy import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS = 2.0 ** -24
ULPS = 4  # csrc/lp_rule.hpp: the transcendental steps, against float64


def _batch(n, exp, kind, seed):
    rng = np.random.default_rng([seed, n])
    z = (rng.standard_normal((n, 64)) * 3).astype(np.float32)
    z[0, 7] = z[0, 40] = z[0].max() + 1  # an exact tie at the top: the first index wins
    x = rng.standard_normal((n, 64)).astype(np.float32)
    lab = rng.integers(0, 64, n).astype(np.int64)
    use = rng.random(n) < 0.6
    use[0] = True
    if kind == "empty":
        use[:] = False
    if kind == "bad":
        lab[0], lab[np.flatnonzero(use)[-1]] = 64, -1
    return z, x, (~use if exp == "other" else use), lab


# ---- the rule header on the host

@pytest.mark.parametrize("exp", PC.EXPS)
def test_row_rule_gradients_and_f1_of_the_host_program_equal_float64(exp):
    """Three batches with one that selects nothing in the middle, and one with labels out of range."""
    for step, kind in enumerate(("plain", "empty", "bad", "plain")):
        z, x, mask, lab = _batch(157, exp, kind, step)
        got = PC.host_rows(z, lab, mask, exp)
        ref = PREF.batch(z.astype(np.float64), x.astype(np.float64), mask, lab, exp)
        assert got["M"] == ref["M"] and got["bad"] == ref["bad"] == (2 if kind == "bad" else 0)
        assert np.array_equal(got["pred"], ref["pred"]) and got["pred"][0] == 7
        # loss_row = lse - z[label]: both terms rounded, the sum of 64 exponentials, one logf
        bound = ULPS * EPS * (np.abs(z).max(-1) + np.log(64.0) + 64 * EPS + 1.0)
        assert (np.abs(got["loss_row"] - ref["loss_row"]) <= bound).all()
        if kind == "empty":
            assert got["M"] == 0 and (got["g"] == 0).all() and got["loss"] == 0 and got["f1"] == 0 and (got["counters"] == 0).all()
            continue
        t = torch.from_numpy(z).double().requires_grad_(True)
        u = torch.from_numpy(ref["use"])
        F.cross_entropy(t[u], torch.from_numpy(np.where(ref["use"], np.clip(lab, 0, 63), 0))[u], reduction="sum").backward()
        assert (np.abs(got["g"] - t.grad.numpy()) <= (ULPS + 64) * EPS).all()  # softmax in [0, 1]: 64 terms in the sum
        assert (got["g"][~ref["use"]] == 0).all()
        assert abs(got["loss"] - ref["loss"]) <= 8 * EPS * (abs(ref["loss"]) + np.abs(z).max() + 5)
        assert got["accuracy"] == np.float32(ref["accuracy"]) and got["correct"] == int(round(ref["accuracy"] * ref["M"]))
        assert abs(got["f1"] - ref["f1"]) <= 2 * EPS
        p, l_ = ref["pred"][ref["use"]], lab[ref["use"]]
        want = np.stack([np.bincount(l_[p == l_], minlength=64), np.bincount(p, minlength=64), np.bincount(l_, minlength=64)])
        assert np.array_equal(got["counters"][:3], want)
        od = np.isin(l_, PREF.ood_set(exp))
        assert got["ood_rows"] == ref["ood_rows"] == int(od.sum()) and got["ood_correct"] == ref["ood_correct"]
        assert np.array_equal(got["counters"][3:], np.stack([np.bincount(l_[od & (p == l_)], minlength=64),
                                                            np.bincount(p[od], minlength=64), np.bincount(l_[od], minlength=64)]))
        assert abs(got["ood_loss_sum"] - ref["ood_loss_sum"]) <= 8 * EPS * ref["ood_rows"] * (np.abs(z).max() + 5)
        assert abs(LP.macro_f1(*got["counters"][:3]) - ref["f1"]) <= 1e-12


@pytest.mark.parametrize("exp", PC.EXPS)
def test_f1_of_the_host_program_equals_sklearn(exp):
    sk = pytest.importorskip("sklearn.metrics")
    for step, kind in enumerate(("plain", "bad")):
        z, x, mask, lab = _batch(157, exp, kind, step)
        got = PC.host_rows(z, lab, mask, exp)
        use = PC.selected(mask, exp) & (lab >= 0) & (lab < 64)
        p, l_ = got["pred"][use], lab[use]
        assert abs(got["f1"] - sk.f1_score(l_, p, average="macro")) <= 2 * EPS
        assert abs(sk.f1_score(p, l_, average="macro") - sk.f1_score(l_, p, average="macro")) <= 1e-12  # the reference's swapped call
        assert abs(PREF.macro_f1(p, l_) - sk.f1_score(l_, p, average="macro")) <= 1e-12


def test_ood_sets_are_the_reference_s():
    other = {x * 8 + y for x in range(8) for y in range(8) if x in {0, 1, 6, 7} or y in {0, 1, 6, 7}}
    ego = {x * 8 + y for x in range(8) for y in range(8) if x not in {3, 4}}
    assert set(LP.ood_labels("other")) == other == set(PREF.ood_set("other").tolist()) and len(other) == 48
    assert set(LP.ood_labels("ego")) == ego == set(PREF.ood_set("ego").tolist()) and len(ego) == 48
    z = np.zeros((64, 64), np.float32)
    for exp, want in (("other", other), ("ego", ego)):  # every label once, all selected: the host program's OOD row count
        mask = np.zeros(64, bool) if exp == "other" else np.ones(64, bool)
        got = PC.host_rows(z, np.arange(64), mask, exp)
        assert got["ood_rows"] == 48 and set(np.flatnonzero(got["counters"][5]).tolist()) == want


@pytest.mark.parametrize("K", [64, 12])
def test_adamw_of_the_host_program_equals_torch(K):
    """Three steps with an M = 0 step in the middle against torch.optim.AdamW(lr, eps=1e-4) in float64; the skipped step moves
    nothing, the step count included."""
    rng = np.random.default_rng(K)
    GF = 64 * K + 64
    w0 = rng.standard_normal(GF).astype(np.float32)
    grads = [(5, (rng.standard_normal(GF) * 0.1).astype(np.float32)), (0, np.full(GF, np.nan, np.float32)),
             (3, (rng.standard_normal(GF) * 0.1).astype(np.float32)), (9, (rng.standard_normal(GF) * 0.1).astype(np.float32))]
    lr, eps = 0.0015, 1e-4
    w, m, v, step, pw = PC.host_adamw(w0, np.zeros(GF), np.zeros(GF), 0, [1.0, 1.0], grads, lr, eps, K=K)
    assert step == 3 and np.allclose(pw, [0.9 ** 3, 0.999 ** 3], rtol=1e-15)
    p = torch.nn.Parameter(torch.from_numpy(w0).double())
    opt = torch.optim.AdamW([p], lr=float(np.float32(lr)), eps=float(np.float32(eps)))
    for M, g in grads:
        if M:
            p.grad = torch.from_numpy(g).double()
            opt.step()
    assert np.abs(w - p.detach().numpy()).max() <= 16 * EPS * (np.abs(w0).max() + 1)
    st = opt.state[p]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 8 * EPS and np.abs(v - st["exp_avg_sq"].numpy()).max() <= 8 * EPS
    # an M = 0 step alone changes no bit
    w2, m2, v2, step2, pw2 = PC.host_adamw(w, m, v, step, pw, grads[1:2], lr, eps, K=K)
    assert step2 == step and np.array_equal(pw2, pw)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in ((w, w2), (m, m2), (v, v2)))


def test_reduce_of_the_host_program():
    rng = np.random.default_rng(2)
    P, K = 5, 64
    pf = rng.standard_normal((P, 64 * K + 64)).astype(np.float32)
    pd = rng.random((P, 2))
    pi = np.zeros((P, PC.PART_INTS), np.int32)
    M, grad, st = PC.host_reduce(pf, pd, pi)
    assert M == 0 and (grad == 0).all() and (st == 0).all()
    pi[:, 1] = [3, 0, 4, 1, 2]
    pi[:, 0] = [1, 0, 2, 0, 1]
    M, grad, st = PC.host_reduce(pf, pd, pi)
    s = pf[0]
    for w in range(1, P):
        s = s + pf[w]
    assert M == 10 and np.array_equal(grad, s / np.float32(10))
    assert st[0] == np.float32(pd[:, 0].cumsum()[-1] / 10.0) and st[1] == np.float32(0.4) and st[6] == 10


# ---- the pin to the reference's modules

@pytest.mark.parametrize("B,A,R", PC.GOLDEN_SHAPES)
def test_restatement_equals_the_reference_modules(B, A, R):
    g = np.load(os.path.join(GOLDEN, "lp_probe_%d_%d_%d.npz" % (B, A, R)))
    assert [str(n) for n in g["names"]] == list(LP.KEYS)
    assert str(g["fusion_attn_last_hook"]) == str(BC.CFG["num_layer"][0] - 1)  # the last SelfAttentionLayer of the block
    assert str(g["ro_attn_last_hook"]) == str(BC.CFG["num_layer"][1] - 1)
    c = case(B, A, R)
    taps = PREF.taps(c["sd"], c["obs"], c["pm"], c["rm"], A, BC.CFG["num_layer"])
    hd = PC.head(64)
    for tap in PC.TAPS:
        assert g[tap].shape == taps[tap].shape == (B, A, 64)
        assert np.abs(g[tap] - taps[tap]).max() <= 1e-12 * np.abs(g[tap]).max(), tap
        for exp in PC.EXPS:
            x = PREF.rows(taps[tap], exp)
            z = PREF.logits(x, hd)
            want = g["%s_%s_logits" % (tap, exp)]
            assert want.shape == z.shape and np.abs(want - z).max() <= 1e-12 * np.abs(want).max(), (tap, exp)
            mask, lab = PC.labels(B, A, exp)
            b = PREF.batch(z, x, mask, lab, exp)
            loss, acc = g["%s_%s_loss" % (tap, exp)]
            assert b["M"] > 0 and abs(b["loss"] - loss) <= 1e-12 * abs(loss) and abs(b["accuracy"] - acc) <= 1e-12, (tap, exp)
    # ro_attn's token 0 is the first third of the context the forward test is held to
    assert np.array_equal(taps["ro_attn"][:, 0], c["ref"]["context"][:, :64])


def test_restatement_s_gradient_equals_autograd_and_baseline_rows_equal_the_reference_s_gather():
    B, A, R = 3, 64, 1
    c = case(B, A, R)
    for exp in PC.EXPS:
        x = PREF.baseline_rows(c["obs"], A, exp)
        obs = torch.from_numpy(c["obs"]).double()
        if exp == "other":  # linear_probing.py:184-191 with A - 1 for 127
            ego = obs[..., :6].unsqueeze(2).repeat(1, 1, A - 1, 1)
            want = torch.cat([ego, obs[..., 6:6 * A].reshape(B, R, A - 1, 6)], dim=-1).permute(0, 2, 1, 3).reshape(B, A - 1, -1)
        else:
            want = obs[..., :6].reshape(-1, 6 * R)
        assert np.array_equal(x, want.numpy())
        hd = PC.head(x.shape[-1])
        mask, lab = PC.labels(B, A, exp, "bad")
        b = PREF.batch(PREF.logits(x, hd), x, mask, lab, exp)
        w = hd["head.weight"].double().requires_grad_(True)
        bias = hd["head.bias"].double().requires_grad_(True)
        u = torch.from_numpy(b["use"])
        z = F.linear(torch.from_numpy(x).reshape(-1, x.shape[-1]), w, bias)
        F.cross_entropy(z[u], torch.from_numpy(lab.reshape(-1))[u]).backward()
        want = np.concatenate([w.grad.numpy().reshape(-1), bias.grad.numpy()])
        assert b["bad"] >= 1 and np.abs(b["grad"] - want).max() <= 1e-12


# ---- the surface

def test_symbols_header_and_structs():
    names = {"gd_bc_hidden", "gd_lp_forward", "gd_lp_update", "gd_lp_eval_accumulate"}
    assert names <= set(_capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    for n in names:
        assert re.search(r"\bint %s\(" % n, header)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_bc_hidden.argtypes) == 8 and len(L.gd_lp_forward.argtypes) == 8
    assert len(L.gd_lp_update.argtypes) == 10 and len(L.gd_lp_eval_accumulate.argtypes) == 11
    assert C.sizeof(_capi.GdLPProbe) == 8 * 4 + 2 * 4 + 2 * 8 + 15 * 8 and _capi.GdLPProbe.weight.offset == 56
    assert C.sizeof(_capi.GdLPRows) == 24 and C.sizeof(_capi.GdBCOutputs) == 72
    assert "GD_LP_EVAL_WORDS = %d" % _capi.LP_EVAL_WORDS in header and "[num_partials][%d]" % _capi.LP_PART_INTS in header
    rule = open(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "lp_rule.hpp")).read()
    assert "PART_INTS = N_HEAD + N_COUNTERS * CLASSES" in rule and _capi.LP_PART_INTS == 8 + 6 * 64
    import gpudrive_lab_amd
    assert gpudrive_lab_amd.DeviceLinearProbe is LP.DeviceLinearProbe


def _structs(model=_capi.LP_EARLY, exp=_capi.IL_FUTURE_OTHER):
    p, lp = _capi.GdBCPolicy(), _capi.GdLPProbe()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers, p.head_layers, p.n_components = 64, 5, 3, 2, 2, 6
    p.clip_value, p.chunk_rows, p.blob, p.scratch = -20.0, 8, 4096, 4096
    p.blob_floats = int(BP.pack_index(5, (3, 2), 2, 6).size)
    p.scratch_floats = BP.scratch_floats(64, 8)
    lp.model, lp.exp, lp.in_features, lp.num_partials, lp.max_agents, lp.num_stack = model, exp, 64, 16, 64, 5
    lp.eps, lp.weight_decay, lp.beta1, lp.beta2 = 1e-4, 0.01, 0.9, 0.999
    for name, _ in _capi.GdLPProbe._fields_[11:]:
        setattr(lp, name, 4096)
    return p, lp


def test_c_entries_refuse_before_the_device():
    """The checkers return a message for a bad struct or argument; the pointers are never read (they are junk here)."""
    L = _capi.lib()
    p, lp = _structs()
    rows = _capi.GdLPRows()

    def err():
        return L.gd_last_error().decode()

    def hidden(tap=0, out=4096, n=4):
        return L.gd_bc_hidden(C.byref(p), 4096, 4096, 4096, n, tap, out, None)

    assert hidden(tap=2) == _capi.GD_ERR_INVALID and "tap" in err()
    assert hidden(out=None) == _capi.GD_ERR_INVALID and "out" in err()
    assert hidden(out=4100) == _capi.GD_ERR_INVALID and "aligned" in err()
    assert hidden(n=0) == _capi.GD_ERR_INVALID and "gd_bc_hidden" in err()
    p.max_agents = 96
    assert hidden() == _capi.GD_ERR_INVALID and "max_agents" in err()
    p.max_agents = 64

    def update(mask=4096, labels=4096, n=4):
        return L.gd_lp_update(C.byref(p), C.byref(lp), 4096, 4096, 4096, n, mask, labels, C.byref(rows), None)

    for field, bad, word in (("model", 3, "model"), ("exp", 2, "exp"), ("in_features", 32, "in_features"), ("num_partials", 0, "num_partials"),
                             ("num_partials", 5000, "num_partials"), ("max_agents", 128, "policy's"), ("num_stack", 4, "policy's"),
                             ("eps", 0.0, "eps"), ("weight_decay", -1.0, "weight_decay"), ("beta1", 1.0, "betas"), ("packed", 4100, "packed"),
                             ("packed", None, "packed"), ("weight", None, "weight"), ("part_d", 4100, "part_d"), ("beta_pow", 4100, "beta_pow"),
                             ("sums", None, "sums"), ("scal", None, "scal")):
        keep = getattr(lp, field)
        setattr(lp, field, bad)
        assert update() == _capi.GD_ERR_INVALID and word in err() and "gd_lp_update" in err(), (field, err())
        setattr(lp, field, keep)
    lp.reserved[1] = 1
    assert update() == _capi.GD_ERR_INVALID and "reserved" in err()
    lp.reserved[1] = 0
    assert update(mask=None) == _capi.GD_ERR_INVALID and "labels" in err()
    assert update(labels=4100) == _capi.GD_ERR_INVALID and "labels" in err()
    assert update(n=0) == _capi.GD_ERR_INVALID
    p.blob_floats += 1
    assert update() == _capi.GD_ERR_INVALID and "blob_floats" in err()  # whatever gd_bc_forward refuses
    p.blob_floats -= 1
    rows.logits = 4100
    assert update() == _capi.GD_ERR_INVALID and "logits" in err()
    rows.logits = None
    # the forward needs an output and takes no loss_row; the evaluation needs acc
    assert L.gd_lp_forward(C.byref(p), C.byref(lp), 4096, 4096, 4096, 4, C.byref(rows), None) == _capi.GD_ERR_INVALID and "logits or pred" in err()
    rows.pred, rows.loss_row = 4096, 4096
    assert L.gd_lp_forward(C.byref(p), C.byref(lp), 4096, 4096, 4096, 4, C.byref(rows), None) == _capi.GD_ERR_INVALID and "loss_row" in err()
    rows.loss_row = None
    assert L.gd_lp_forward(C.byref(p), None, 4096, 4096, 4096, 4, C.byref(rows), None) == _capi.GD_ERR_INVALID
    ev = lambda acc: L.gd_lp_eval_accumulate(C.byref(p), C.byref(lp), 4096, 4096, 4096, 4, 4096, 4096, C.byref(rows), acc, None)  # noqa: E731
    assert ev(None) == _capi.GD_ERR_INVALID and "acc" in err() and ev(4100) == _capi.GD_ERR_INVALID
    # the baseline probe: no policy, K = 6 R or 12 R, at most 64
    lp.model = _capi.LP_BASELINE
    assert update() == _capi.GD_ERR_INVALID and "no policy" in err()
    base = lambda: L.gd_lp_update(None, C.byref(lp), 4096, None, None, 4, 4096, 4096, C.byref(rows), None)  # noqa: E731
    assert base() == _capi.GD_ERR_INVALID and "in_features" in err()
    lp.num_stack = 6
    assert base() == _capi.GD_ERR_INVALID and "64" in err()
    lp.model = _capi.LP_EARLY
    assert L.gd_lp_update(None, C.byref(lp), 4096, 4096, 4096, 4, 4096, 4096, C.byref(rows), None) == _capi.GD_ERR_INVALID


def test_pack_index():
    for K in (64, 60, 30, 6, 12):
        idx = LP.pack_index(K)
        zero = 64 * K + 64
        real = idx[idx != zero]
        assert idx.shape == (4160,) and np.array_equal(np.sort(real), np.arange(zero)) and (idx == zero).sum() == 64 * (64 - K)
    # with K = 64 it is bc_policy's `mfma` form of a 64 x 64 Linear followed by its bias
    full = BP.pack_index(1, (1, 1), 0, 1)
    shapes = BP.expected_shapes(1, (1, 1), 0, 1)
    off, name = 0, "fusion_attn.0.0.module.attention.q_proj.weight"
    for k, s in shapes.items():
        if k == name:
            break
        off += int(np.prod(s))
    at = np.flatnonzero(full == off)[0]  # where W[0][0] lands: the start of that Linear's packed block
    assert np.array_equal(full[at:at + 4160] - off, LP.pack_index(64))


# ---- the refusals

def test_every_python_refusal():
    hd = PC.head(64)
    ok = dict(model="baseline", exp="ego", max_agents=64, num_stack=5, device="cuda")
    base = PC.head(30)
    bad = [
        (None, hd, dict(ok, model="mid_lp"), "model"), (None, hd, dict(ok, exp="both"), "exp"),
        (None, hd, dict(ok, max_agents=96), "max_agents"), (None, hd, dict(ok, num_stack=0), "num_stack"),
        (None, PC.head(64), dict(ok), "shape"),  # K is 30 for this probe
        (None, PC.head(72), dict(ok, exp="other", num_stack=6), "at most 64"),
        (None, base, dict(ok, lr=0.0), "lr"), (None, base, dict(ok, eps=-1.0), "eps"), (None, base, dict(ok, betas=(0.9, 1.0)), "betas"),
        (None, base, dict(ok, betas=0.9), "betas"), (None, base, dict(ok, weight_decay=-0.1), "weight_decay"),
        (None, base, dict(ok, partials=0), "partials"), (None, base, dict(ok, partials=5000), "partials"),
        (None, base, dict(ok, chunk_rows=0), "chunk_rows"), (None, base, dict(ok, device="cpu"), "GPU"),
        (None, {"head.weight": base["head.weight"]}, dict(ok), "missing"),
        (None, dict(base, **{"yaw_head.weight": base["head.weight"]}), dict(ok), "unexpected"),
        (None, dict(base, **{"head.bias": base["head.bias"].double()}), dict(ok), "float32"),
        (None, dict(base, **{"head.weight": base["head.weight"].t().contiguous().t()}), dict(ok), "shape|contiguous"),
        (None, [1, 2], dict(ok), "mapping"),
        (None, hd, dict(ok, model="early_lp"), "DeviceBCPolicy"), (object(), hd, dict(ok, model="late_lp"), "DeviceBCPolicy"),
        (object(), base, dict(ok), "no policy"),
    ]
    for policy, sd, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            LP.DeviceLinearProbe(policy, sd, **kw)
    assert LP.in_features("early_lp", "other", 5) == 64 and LP.in_features("baseline", "other", 5) == 60
    assert LP.in_features("baseline", "ego", 5) == 30
