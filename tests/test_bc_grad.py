"""The device BC backward without a GPU: the differentiable restatement (bc_grad_reference.py) pinned to the reference module's
own `gmm_loss(...)[0].backward()` (tests/golden/bc_grad_*.npz), the margins that keep the non-smooth points of every case
from flipping, four wrong backward rules shown caught, the head's gradient rule (csrc/bc_grad_rule.hpp) on the host against
float64 autograd, and `TrainableBCPolicy`'s surface and refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP

from . import bc_cases as BC
from . import bc_grad_reference as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 32  # the bound of the GPU tests: error <= K E_p
_CACHE = {}


def case(B, A, R, cfg=BC.CFG):
    """The seeded case with its float64 and float32 gradients at grad_nll = 1 / B, computed once and shared."""
    key = GR.case_key(B, A, R, cfg)
    if key not in _CACHE:
        sd, obs, pm, rm, expert, kinds = GR.case_inputs(B, A, R, cfg)
        w = GR.grad_weights(B, "mean")
        g64, nll, margins = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg)
        g32, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, dtype=torch.float32)
        _CACHE[key] = dict(sd=sd, obs=obs, pm=pm, rm=rm, expert=expert, kinds=kinds, w=w, g64=g64, g32=g32, nll=nll,
                           margins=margins, E=GR.yardstick(g32, g64))
    return _CACHE[key]


# ---- the pin to the reference module

def test_restatement_equals_the_reference_modules_backward():
    """loss.mean() weighs every row with 1 / B in float64 (the cases below carry it as the float32 the device call takes).  The
    gradient of a k_proj bias is zero in exact arithmetic (a softmax row does not see a constant added to its scores): both
    sides hold only rounding residue there, which is held against the same layer's q_proj bias gradient."""
    B, A, R = 3, 64, 1
    g = np.load(os.path.join(GOLDEN, "bc_grad_%d_%d_%d.npz" % (B, A, R)))
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R)
    g64, nll, _ = GR.gradients(sd, obs, pm, rm, expert, np.full(B, 1.0 / B), A)
    names = [str(n) for n in g["names"]]
    assert names == list(g64)  # the module's own parameter names, in its own order
    assert abs(float(g["loss"]) - nll.mean()) <= 1e-12 * abs(float(g["loss"]))
    for i, (name, grad) in enumerate(g64.items()):
        flat = grad.reshape(-1)
        norm = float(g["norms"][i])
        if name.endswith("k_proj.bias"):
            q = float(g["norms"][names.index(name.replace("k_proj", "q_proj"))])
            assert q > 0 and norm <= 1e-12 * q and np.sqrt((flat * flat).sum()) <= 1e-12 * q, name
            continue
        assert norm > 0, name
        assert abs(np.sqrt((flat * flat).sum()) - norm) <= 1e-12 * norm, name
        assert abs(flat.sum() - float(g["sums"][i])) <= 1e-12 * np.abs(flat).sum(), name
        pos = g["positions"][i]
        assert pos.max() < flat.size
        assert np.abs(flat[pos] - g["values"][i]).max() <= 1e-12 * np.abs(flat).max(), name


# ---- the non-smooth points cannot flip

@pytest.mark.parametrize("key", list(GR.INPUT_SEEDS))
def test_margins_keep_clamps_and_relus_from_flipping(key):
    B, A, R, num_layer, hl, C_, clip = key
    cfg = dict(num_layer=num_layer, head_num_layers=hl, n_components=C_, clip_value=clip)
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R, cfg)
    net = GR.Net(sd, A, cfg)
    with torch.no_grad():
        net.nll(obs, pm, rm, expert)
    assert net.margins["clamp"] > GR.MARGIN and net.margins["relu"] > GR.MARGIN, net.margins


def test_pushed_covariances_and_fully_masked_rows_in_float64():
    """What the GPU test asserts as exact zeros holds in the reference: the two raw covariances pushed outside the clamp give
    zero gradient rows of head.head; with every partner masked, ego_ro_attn's q_proj, k_proj and q_norm get nothing while its
    v_proj, o_proj and kv_norm do."""
    c = case(3, 64, 1)
    C_ = BC.CFG["n_components"]
    for r in (3 * C_ + 1, 3 * C_ + 5):
        assert (c["g64"]["head.head.weight"][r] == 0).all() and c["g64"]["head.head.bias"][r] == 0
    assert np.abs(c["g64"]["head.head.weight"][3 * C_:6 * C_]).max() > 0 and np.abs(c["g64"]["head.head.bias"][3 * C_:6 * C_]).max() > 0
    pm = np.ones_like(c["pm"])
    g, _, _ = GR.gradients(c["sd"], c["obs"], pm, c["rm"], c["expert"], c["w"], 64)
    p = "ego_ro_attn.0.module."
    for name in (p + "attention.q_proj", p + "attention.k_proj", p + "q_norm"):
        assert (g[name + ".weight"] == 0).all() and (g[name + ".bias"] == 0).all(), name
    for name in (p + "attention.v_proj", p + "attention.o_proj", p + "kv_norm"):
        assert np.abs(g[name + ".weight"]).max() > 0 and np.abs(g[name + ".bias"]).max() > 0, name


# ---- wrong backward rules are caught

@pytest.mark.parametrize("wrong", GR.WRONG)
def test_a_wrong_backward_rule_is_caught(wrong):
    """On the B = 17 case (samples a, b, ab have rows with every key masked; two covariances sit outside the clamp) each
    wrong rule moves some parameter gradient by at least 4 K E_p: the GPU comparison (error <= K E_p) tells it from the right
    one with a factor 4 to spare."""
    c = case(17, 64, 5)
    bad, _, _ = GR.gradients(c["sd"], c["obs"], c["pm"], c["rm"], c["expert"], c["w"], 64, wrong=wrong)
    ratio = {k: float(np.abs(bad[k] - c["g64"][k]).max()) / c["E"][k] for k in bad}
    assert max(ratio.values()) >= 4 * K, (wrong, max(ratio.values()))
    if wrong == "soft_clamp":  # it is the pushed rows that move
        assert ratio["head.head.bias"] >= 4 * K
    if wrong == "additive_mask":  # q and k of the layers with fully masked rows
        assert ratio["ego_ro_attn.0.module.attention.q_proj.weight"] >= 4 * K


def test_the_yardstick_is_a_float32_error():
    c = case(17, 64, 5)
    rel = [c["E"][k] / np.abs(c["g64"][k]).max() for k in c["E"] if not k.endswith("k_proj.bias")]  # those are zero in exact arithmetic
    assert 2.0 ** -23 <= min(rel) and max(rel) < 1e-3  # not zero, and no loose bound


# ---- the gradient rule of the head on the host

F32_COV_MAX = float(np.float32(GR.COV_MAX))  # the bound as float32 arithmetic sees it


def _rule_rows(C_, n=64, seed=3):
    rng = np.random.default_rng([seed, C_])
    raw = rng.standard_normal((n, 7 * C_)).astype(np.float32) * 2
    raw[:, 3 * C_:6 * C_] *= 6  # covariances below, inside and above the clamp [-5, 3.58352]
    raw[0, 3 * C_] = -5.0  # exactly on the lower bound: the gradient passes
    raw[1, 3 * C_] = np.float32(GR.COV_MAX)  # exactly on the upper bound: it passes too
    raw[2, 3 * C_] = np.nextafter(np.float32(-5.0), np.float32(-6.0))  # one step outside: exactly 0
    raw[3, 3 * C_] = np.nextafter(np.float32(GR.COV_MAX), np.float32(4.0))
    if C_ > 1:
        raw[4, 6 * C_] = raw[4, 6 * C_ + C_ - 1] = 9.0  # weights tied at the top
    expert = rng.standard_normal((n, 3)).astype(np.float32) * 2
    for r in range(4):  # component 0 of the rows on and beside the bounds carries posterior: its gradient is no underflow
        raw[r, 3 * C_ + 1:3 * C_ + 3], raw[r, 6 * C_] = 0.0, 9.0
        expert[r] = raw[r, :3] + np.float32(0.5)
    return raw, expert


@pytest.mark.parametrize("C_", [1, 2, 6, 16])
def test_grad_rule_header_on_the_host_equals_float64_autograd(C_):
    """Bound, per element.  wl[k] is a sum of terms of magnitude m_k <= |wl[k]| + 2 (15 + 18.5 + 2.8) (the log-covariance sum,
    log(weight + 1e-8) and the constant can cancel against the quadratic form; their sizes are bounded by the clamp and by
    1e-8), so its float32 error is a few eps m_k, and the posterior exp(wl[k] - M) / s carries that as a RELATIVE error.  A
    component more than 104 below M has a posterior below 1e-45 and contributes nothing representable, so m_k <= |M| + 180
    for every component that counts.  The factors that multiply the posterior add a few eps of their own magnitude, where a
    difference (0.5 d^2 / cov - 0.5; g[j] - w[j] G) counts with the sum of its terms' magnitudes.  With 16 for 'a few':
        |error| <= 16 eps (|M| + 180) (magnitude of the element's terms) + 1e-30."""
    raw, expert = _rule_rows(C_)
    clip, n, eps = -5.0, raw.shape[0], 2.0 ** -24
    got, got_nll = GR.run_grad_rule_host(raw, clip, expert)
    t = torch.from_numpy(raw).double().requires_grad_(True)
    nll = GR.mixture_nll(t, torch.from_numpy(expert).double(), C_, clip, cov_max=F32_COV_MAX)
    nll.sum().backward()
    want = t.grad.numpy()
    r64 = raw.astype(np.float64)
    means, rc, rw = r64[:, :3 * C_].reshape(n, C_, 3), r64[:, 3 * C_:6 * C_].reshape(n, C_, 3), r64[:, 6 * C_:]
    lc = np.clip(rc, clip, F32_COV_MAX)
    d = expert.astype(np.float64)[:, None] - means
    w = np.exp(rw - rw.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    wl = -0.5 * (d * d / np.exp(lc)).sum(-1) - 0.5 * lc.sum(-1) - 1.5 * np.log(2 * np.pi) + np.log(w + 1e-8)
    M = wl.max(-1, keepdims=True)
    post = np.exp(wl - M)
    post /= post.sum(-1, keepdims=True)
    gk = post * w / (w + 1e-8)
    mag = np.concatenate([(post[..., None] * np.abs(d) / np.exp(lc)).reshape(n, -1),
                          (post[..., None] * (0.5 * d * d / np.exp(lc) + 0.5)).reshape(n, -1),
                          gk + w * gk.sum(-1, keepdims=True)], axis=1)
    tol = 16 * eps * (np.abs(M) + 180) * mag + 1e-30
    err = np.abs(got - want)
    assert (err <= tol).all(), float((err / tol).max())
    assert np.abs(want).max() > 0.1 and np.isfinite(got).all()
    # the clamp's gradient: exact zeros outside, bounds included inside
    outside = (rc < clip) | (rc > F32_COV_MAX)
    gc = got[:, 3 * C_:6 * C_].reshape(n, C_, 3)
    assert outside.any() and (~outside).any() and (gc[outside] == 0).all()
    assert (want[:, 3 * C_:6 * C_].reshape(n, C_, 3)[outside] == 0).all()
    assert outside[2, 0, 0] and outside[3, 0, 0] and not outside[0, 0, 0] and not outside[1, 0, 0]
    assert want[0, 3 * C_] != 0 and want[1, 3 * C_] != 0 and got[0, 3 * C_] != 0 and got[1, 3 * C_] != 0
    # the nll beside it is bc_rule.hpp's own
    assert np.array_equal(got_nll, BC.run_rule_host(raw, clip, np.zeros(n, np.float32), np.zeros((n, 3), np.float32), expert, True)["nll"])


# ---- the module's surface without a device

def test_trainable_module_names_shapes_and_state_dict():
    from gpudrive_lab_amd import TrainableBCPolicy
    from gpudrive_lab_amd import bc_train as BT
    sd = BC.state_dict(5)
    tbp = TrainableBCPolicy.from_state_dict(sd, max_agents=64, num_stack=5, **BC.CFG)
    want = BP.expected_shapes(5, BC.CFG["num_layer"], BC.CFG["head_num_layers"], BC.CFG["n_components"])
    assert [(k, tuple(p.shape)) for k, p in tbp.named_parameters()] == list(want.items())
    assert list(tbp.state_dict()) == list(want)  # the workspace and the pack index are no part of it
    assert all(p.requires_grad and p.dtype == torch.float32 for p in tbp.parameters())
    assert all(torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr() for k, v in tbp.state_dict().items())
    BP.check_bc_args(tbp.state_dict(), max_agents=64, num_stack=5, **BC.CFG)  # DeviceBCPolicy.load_state_dict's own check
    G = BT.grad_floats(5, BC.CFG["num_layer"], BC.CFG["head_num_layers"], BC.CFG["n_components"])
    assert G == sum(p.numel() for p in tbp.parameters())
    assert tbp.nbytes(17) - tbp.nbytes(3) == 14 * 12  # only the per-row outputs depend on B
    assert tbp.nbytes(1) > 4 * (tbp.partials * G + 3 * G)
    small = TrainableBCPolicy(GR.state_dict(1, GR.MINIMAL), 64, 1, **GR.MINIMAL, partials=1, chunk_rows=1)
    assert small.nbytes(1) < tbp.nbytes(1)


def test_trainable_module_every_refusal():
    from gpudrive_lab_amd import TrainableBCPolicy
    sd = BC.state_dict(5)
    ok = dict(max_agents=64, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2, n_components=6, clip_value=-20.0)
    for name, bad in (("network_dim", 128), ("head_dim", 32), ("num_head", 8), ("network_num_layers", 3), ("act_func", "selu"),
                      ("dropout", 0.1), ("action_dim", 2), ("time_dim", 2), ("use_tom", "guide"), ("max_agents", 96),
                      ("num_stack", 0), ("num_stack", 9), ("num_layer", (0, 2)), ("num_layer", 3), ("head_num_layers", 5),
                      ("n_components", 17), ("clip_value", float("nan")), ("chunk_rows", 0), ("chunk_rows", 5000),
                      ("partials", 0), ("partials", 4097), ("partials", 2.0), ("partials", True)):
        with pytest.raises(ValueError, match="TrainableBCPolicy: .*" + name):
            TrainableBCPolicy(sd, **dict(ok, **{name: bad}))
    with pytest.raises(ValueError, match="unknown argument"):
        TrainableBCPolicy(sd, rotary=True, **ok)
    with pytest.raises(ValueError, match="device"):
        TrainableBCPolicy(sd, device="gpu9", **ok)
    some = "fusion_attn.1.0.module.attention.k_proj.weight"
    with pytest.raises(ValueError, match="missing"):
        TrainableBCPolicy({k: v for k, v in sd.items() if k != some}, **ok)
    with pytest.raises(ValueError, match="unexpected"):
        TrainableBCPolicy(dict(sd, **{"aux_head.0.weight": torch.zeros(64, 64)}), **ok)
    with pytest.raises(ValueError, match="shape"):
        TrainableBCPolicy(dict(sd, **{some: torch.zeros(64, 32)}), **ok)
    with pytest.raises(ValueError, match="float32"):
        TrainableBCPolicy(dict(sd, **{some: sd[some].double()}), **ok)
    tbp = TrainableBCPolicy(sd, **ok)
    obs, pm, rm, expert, _, _, _ = BC.inputs(2, 64, 5)
    t = [torch.from_numpy(a) for a in (obs, pm, rm, expert)]
    with pytest.raises(ValueError, match="no host path"):  # everything below is refused before anything reaches a device
        tbp(*t)
    with pytest.raises(ValueError, match="require grad"):
        tbp(t[0].clone().requires_grad_(True), *t[1:])
    with pytest.raises(ValueError, match="obs must be a"):
        tbp(t[0][:, :4], *t[1:])
    with pytest.raises(ValueError, match="obs must be a"):
        tbp(t[0][0], *t[1:])


def test_c_entry_refuses_before_the_device():
    """gd_bc_backward's checker returns a message for a bad struct; the pointers are never read (they are junk here)."""
    L = _capi.lib()
    p, g = _capi.GdBCPolicy(), _capi.GdBCGrad()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers, p.head_layers, p.n_components = 64, 5, 3, 2, 2, 6
    p.clip_value, p.chunk_rows, p.blob, p.scratch = -20.0, 8, 4096, 4096
    p.blob_floats = int(BP.pack_index(5, (3, 2), 2, 6).size)
    p.scratch_floats = BP.scratch_floats(64, 8)
    from gpudrive_lab_amd import bc_train as BT
    g.scratch, g.partials, g.num_partials = 4096, 4096, 4
    g.grad_floats = BT.grad_floats(5, (3, 2), 2, 6)
    g.scratch_floats = BT.grad_scratch_floats(64, 8, (3, 2), p.blob_floats)
    # (the C side computes the same two sizes: one off either way is refused below, and with the right sizes the NEXT check speaks)

    def call(n=4, expert=4096, gn=4096, grad=4096):
        return L.gd_bc_backward(C.byref(p), C.byref(g), 4096, 4096, 4096, n, expert, gn, None, grad, None)

    for obj, field, bad, word in ((g, "num_partials", 0, "num_partials"), (g, "num_partials", 4097, "num_partials"),
                                  (g, "grad_floats", g.grad_floats + 1, "grad_floats"), (g, "scratch_floats", g.scratch_floats - 1, "scratch_floats"),
                                  (g, "scratch", 4100, "aligned"), (g, "partials", 4100, "aligned"), (g, "reserved", 1, "reserved"),
                                  (g, "scratch", 0, "required"), (p, "max_agents", 96, "max_agents"), (p, "chunk_rows", 0, "chunk_rows"),
                                  (p, "blob_floats", 7, "blob_floats")):
        keep = getattr(obj, field)
        setattr(obj, field, bad)
        assert call() == _capi.GD_ERR_INVALID
        assert word in L.gd_last_error().decode(), (field, L.gd_last_error())
        setattr(obj, field, keep)
    assert call(n=0) == _capi.GD_ERR_INVALID and call(expert=None) == _capi.GD_ERR_INVALID
    assert call(gn=None) == _capi.GD_ERR_INVALID and call(grad=None) == _capi.GD_ERR_INVALID
    assert call(grad=4100) == _capi.GD_ERR_INVALID and "aligned" in L.gd_last_error().decode()
    assert "gd_bc_backward" in set(_capi.SYMBOLS)
    assert re.search(r"\bint gd_bc_backward\(", open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read())
    rule = open(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "bc_grad_rule.hpp")).read()
    assert "bounds included" in rule.replace("BOTH ", "") and "1e-8" in rule
