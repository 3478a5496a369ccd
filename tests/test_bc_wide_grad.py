"""The device BC backward at network_dim 128 without a GPU: the differentiable restatement at the state dict's width
(bc_wide_grad_reference.py) pinned to the 64-wide restatement, to the float64 forward (bc_reference.py) and to the reference
module's own `gmm_loss(...)[0].backward()` at network_dim 128 (tests/golden/bc_wide_grad_wide_min.npz); the margins of every
wide case; the wrong backward rules shown caught (`quarter_scale` among them: the copy-paste mistake of the kernels);
`gd_bc_backward_dim`'s declaration, binding and refusals; `TrainableBCPolicyDim`'s surface and refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from gpudrive_lab_amd import bc_train as BT

from . import bc_cases as BC
from . import bc_grad_reference as GR
from . import bc_wide_cases as WC
from . import bc_wide_grad_reference as WGR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 32  # the bound of the GPU tests: error <= K E_p


# ---- the pins

def test_wide_restatement_on_a_64_wide_state_dict_is_the_64_wide_restatement():
    B, A, R = 3, 64, 1
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R)
    w = GR.grad_weights(B, "seeded")
    want, nll, _ = GR.gradients(sd, obs, pm, rm, expert, w, A)
    got, got_nll, _ = WGR.gradients(sd, obs, pm, rm, expert, w, A)
    assert np.abs(got_nll - nll).max() <= 1e-12 * (1 + np.abs(nll).max())
    assert list(got) == list(want)
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * max(np.abs(want[k]).max(), 1e-300), k


@pytest.mark.parametrize("name", list(WC.CASES))
def test_wide_nll_is_the_float64_forwards_and_the_margins_hold(name):
    """Seed 1 keeps both head margins above bc_grad_reference.MARGIN on every wide case (the smallest: relu 0.0028 at
    wide_sweep, clamp 0.027 at wide_chunks), so no clamp and no ReLU can flip between float32 and float64."""
    c, f = WGR.case(name), WC.case(name)
    assert np.array_equal(c["obs"], f["obs"]) and np.array_equal(c["pm"], f["pm"])  # the same inputs as the forward's cases
    assert np.abs(c["nll"] - f["ref"]["nll"]).max() <= 1e-12 * (1 + np.abs(c["nll"]).max())
    assert c["margins"]["clamp"] > GR.MARGIN and c["margins"]["relu"] > GR.MARGIN, c["margins"]


def test_wide_restatement_equals_the_reference_modules_backward():
    _restatement_equals_the_reference_modules_backward("wide_min")


def test_wide_restatement_equals_the_reference_modules_backward_at_the_largest_model():
    """wide_top: 288 tensors, head depth 4, 16 components, num_stack 8, (4, 4) layers."""
    _restatement_equals_the_reference_modules_backward("wide_top")


def _restatement_equals_the_reference_modules_backward(case):
    """tests/test_bc_grad.py's comparison and tolerances at network_dim 128 (loss.mean() in float64: weights 1 / B)."""
    g = np.load(os.path.join(GOLDEN, "bc_wide_grad_%s.npz" % case))
    sd, obs, pm, rm, expert, _, A, cfg = WGR.case_inputs(case)
    B = len(obs)
    g64, nll, _ = WGR.gradients(sd, obs, pm, rm, expert, np.full(B, 1.0 / B), A, cfg)
    names = [str(n) for n in g["names"]]
    assert names == list(g64) == list(WC.shapes(WC.lookup(case)[2], cfg))
    assert abs(float(g["loss"]) - nll.mean()) <= 1e-12 * abs(float(g["loss"]))
    for i, (name, grad) in enumerate(g64.items()):
        flat = grad.reshape(-1)
        norm = float(g["norms"][i])
        if name.endswith("k_proj.bias"):  # zero in exact arithmetic: rounding residue, held against the layer's q_proj bias
            q = float(g["norms"][names.index(name.replace("k_proj", "q_proj"))])
            if q > 0:
                assert norm <= 1e-12 * q and np.sqrt((flat * flat).sum()) <= 1e-12 * q, name
            continue
        if norm == 0:  # ego_ro_attn's q side on sample a alone would be; with three samples nothing else is
            assert (flat == 0).all(), name
            continue
        assert abs(np.sqrt((flat * flat).sum()) - norm) <= 1e-12 * norm, name
        assert abs(flat.sum() - float(g["sums"][i])) <= 1e-12 * np.abs(flat).sum(), name
        pos = g["positions"][i]
        assert pos.max() < flat.size
        assert np.abs(flat[pos] - g["values"][i]).max() <= 1e-12 * np.abs(flat).max(), name


# ---- wrong backward rules are caught

@pytest.mark.parametrize("wrong,name", [("quarter_scale", "wide_min"), ("quarter_scale", "wide_sweep"), ("normed_residual", "wide_min"),
                                        ("tanh_gelu", "wide_min"), ("tanh_gelu", "wide_sweep"), ("soft_clamp", "wide_sweep"),
                                        ("additive_mask", "wide_min")])
def test_a_wrong_backward_rule_is_caught_at_128(wrong, name):
    """Each wrong rule moves some parameter gradient by more than K E_p, so the GPU comparison (error <= K E_p) cannot pass
    with it.  soft_clamp needs a covariance pushed outside the clamp (wide_min has C = 1 and none); additive_mask needs a row
    with every key of a segment masked (wide_min's sample a)."""
    c = WGR.case(name)
    bad, nll, _ = WGR.gradients(c["sd"], c["obs"], c["pm"], c["rm"], c["expert"], c["w"], c["A"], c["cfg"], wrong=wrong)
    if wrong in ("quarter_scale", "tanh_gelu", "soft_clamp", "additive_mask"):  # these leave the forward's values alone
        assert np.abs(nll - c["nll"]).max() <= 1e-12 * (1 + np.abs(c["nll"]).max())
    ratio = {k: float(np.abs(bad[k] - c["g64"][k]).max()) / c["E"][k] for k in bad if c["E"][k] > 0}
    print("BCWIDE WRONG %s %s worst %.3g" % (wrong, name, max(ratio.values())))
    assert max(ratio.values()) > K, (wrong, name, max(ratio.values()))
    if wrong == "quarter_scale":  # every q_proj carries it
        assert ratio["fusion_attn.0.0.module.attention.q_proj.weight"] > K


# ---- the C entry

def test_backward_dim_is_declared_exported_and_bound():
    assert "gd_bc_backward_dim" in set(_capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert re.search(r"\bint gd_bc_backward_dim\(const gd_bc_policy_dim \*p, const gd_bc_grad \*g,", header)
    L = _capi.lib()
    assert len(L.gd_bc_backward_dim.argtypes) == len(L.gd_bc_backward.argtypes) == 11
    assert L.gd_bc_backward_dim.argtypes[1:] == L.gd_bc_backward.argtypes[1:]


def _structs(dim, A=64, R=5, num_layer=(4, 3), hl=2, C_=6, chunk=8):
    pd, g = _capi.GdBCPolicyDim(), _capi.GdBCGrad()
    p = pd.base
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers, p.head_layers, p.n_components = A, R, *num_layer, hl, C_
    p.clip_value, p.chunk_rows, p.blob, p.scratch = -20.0, chunk, 4096, 4096
    p.blob_floats = int(BP.pack_index(R, num_layer, hl, C_, network_dim=dim).size)
    p.scratch_floats = BP.scratch_floats(A, chunk, dim)
    pd.network_dim, pd.reserved = dim, 0
    g.scratch, g.partials, g.num_partials = 4096, 4096, 4
    g.grad_floats = BT.grad_floats(R, num_layer, hl, C_, network_dim=dim)
    g.scratch_floats = BT.grad_scratch_floats(A, chunk, num_layer, p.blob_floats, network_dim=dim)
    return pd, g


def test_backward_dim_refuses_before_the_device():
    """The checker answers from the structs alone; every pointer is junk and is never read.  With everything in order up to
    a field, the NEXT check is the one that speaks: that is how the sizes computed here are shown equal to the C side's."""
    L = _capi.lib()

    def call(pd, g, n=4, grad=4096):
        rc = L.gd_bc_backward_dim(C.byref(pd), C.byref(g), 4096, 4096, 4096, n, 4096, 4096, None, grad, None)
        return rc, L.gd_last_error().decode()

    for dim in (64, 128):
        pd, g = _structs(dim)
        rc, why = call(pd, g, grad=4100)  # everything else passes: the last check of all speaks
        assert rc == _capi.GD_ERR_INVALID and why.startswith("gd_bc_backward_dim: ") and "16-byte aligned" in why, why
        for obj, field, bad, word in ((g, "grad_floats", g.grad_floats + 1, "grad_floats"), (g, "grad_floats", g.grad_floats - 1, "grad_floats"),
                                      (g, "scratch_floats", g.scratch_floats - 1, "grad scratch_floats"),
                                      (g, "num_partials", 0, "num_partials"), (g, "reserved", 1, "reserved must be 0"),
                                      (pd.base, "blob_floats", pd.base.blob_floats - 1, "blob_floats"),
                                      (pd.base, "scratch_floats", pd.base.scratch_floats - 1, "scratch_floats is below"),
                                      (pd, "network_dim", 96, "network_dim must be 64 or 128"), (pd, "network_dim", 0, "network_dim"),
                                      (pd, "reserved", 1, "reserved must be 0")):
            keep = getattr(obj, field)
            setattr(obj, field, bad)
            rc, why = call(pd, g)
            assert rc == _capi.GD_ERR_INVALID and word in why, (dim, field, why)
            setattr(obj, field, keep)
        assert call(pd, g, n=0)[0] == _capi.GD_ERR_INVALID
    # the struct is looked at first: a bad network_dim speaks before a bad base
    pd, g = _structs(128)
    pd.network_dim, pd.base.max_agents = 96, 96
    assert "network_dim must be 64 or 128" in call(pd, g)[1]
    # the gradient's sizes for 64 at 128, and the other way round
    pd, g = _structs(128)
    g64 = _structs(64)[1]
    g.grad_floats = g64.grad_floats
    assert "grad_floats is not the parameters' count at network_dim 128" in call(pd, g)[1]
    pd, g = _structs(128)
    g.scratch_floats = BT.grad_scratch_floats(64, 8, (4, 3), pd.base.blob_floats)  # (the 64-wide formula on the 128-wide blob)
    assert "grad scratch_floats is below" in call(pd, g)[1] and "128 *" in call(pd, g)[1]
    pd, g = _structs(64)
    g.grad_floats = _structs(128)[1].grad_floats
    assert "grad_floats is not the parameters' count for these" in call(pd, g)[1]
    assert L.gd_bc_backward_dim(None, C.byref(g), 4096, 4096, 4096, 4, 4096, 4096, None, 4096, None) == _capi.GD_ERR_INVALID
    assert "null argument" in L.gd_last_error().decode()
    # gd_bc_backward itself still answers for 64 only, under its own name
    p64 = _structs(64)[0].base
    g128 = _structs(128)[1]
    assert L.gd_bc_backward(C.byref(p64), C.byref(g128), 4096, 4096, 4096, 4, 4096, 4096, None, 4096, None) == _capi.GD_ERR_INVALID
    assert L.gd_last_error().decode().startswith("gd_bc_backward: grad_floats is not the parameters' count for these")


def test_grad_floats_at_128():
    for name, (B, A, R, cfg) in WC.CASES.items():
        G = BT.grad_floats(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], network_dim=128)
        assert G == sum(int(np.prod(s)) for s in WC.shapes(R, cfg).values()), name
    assert BT.grad_floats(5, (4, 3), 2, 6, network_dim=128) == 1399274  # the sweep's model
    assert BT.grad_floats(5, (3, 2), 2, 6) == BT.grad_floats(5, (3, 2), 2, 6, network_dim=64)
    assert BT.grad_scratch_floats(64, 8, (3, 2), 1000) == BT.grad_scratch_floats(64, 8, (3, 2), 1000, network_dim=64)
    assert BT.grad_scratch_floats(64, 2, (1, 1), 128, network_dim=128) == 128 + 2 * 264 * (128 * 7 + 16)


# ---- the module's surface without a device

def test_trainable_dim_surface_and_refusals():
    from gpudrive_lab_amd import TrainableBCPolicy, TrainableBCPolicyDim
    B, A, R, cfg = WC.CASES["wide_min"]
    wide, narrow = BC.state_dict(R, cfg, network_dim=128), BC.state_dict(R, cfg)
    ok = dict(max_agents=A, num_stack=R, num_head=4, **cfg)
    assert issubclass(TrainableBCPolicyDim, TrainableBCPolicy)
    assert TrainableBCPolicy.NETWORK_DIMS == (64,) and TrainableBCPolicyDim.NETWORK_DIMS == (64, 128)
    tbp = TrainableBCPolicyDim(wide, network_dim=128, partials=2, chunk_rows=2, **ok)
    want = WC.shapes(R, cfg)
    assert tbp.network_dim == 128
    assert [(k, tuple(p.shape)) for k, p in tbp.named_parameters()] == list(want.items())
    assert list(tbp.state_dict()) == list(want)
    assert all(torch.equal(v, wide[k]) and v.data_ptr() != wide[k].data_ptr() for k, v in tbp.state_dict().items())
    BP.check_bc_args(tbp.state_dict(), network_dim=128, network_dims=BP.DeviceBCPolicy.NETWORK_DIMS, **ok)  # load_state_dict's own check
    G = BT.grad_floats(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], network_dim=128)
    assert G == sum(p.numel() for p in tbp.parameters())
    assert tbp.nbytes(17) - tbp.nbytes(3) == 14 * 12
    assert tbp.nbytes(1) > 4 * (2 * G + 3 * G + BP.scratch_floats(A, 2, 128))
    n64 = TrainableBCPolicyDim(narrow, partials=2, chunk_rows=2, **ok)
    assert n64.network_dim == 64 and not n64._wide
    assert n64.nbytes(1) == TrainableBCPolicy(narrow, partials=2, chunk_rows=2, **ok).nbytes(1) < tbp.nbytes(1)
    with pytest.raises(ValueError, match="TrainableBCPolicy: network_dim must be 64 or 128"):
        TrainableBCPolicyDim(wide, network_dim=96, **ok)
    with pytest.raises(ValueError, match="shape"):
        TrainableBCPolicyDim(narrow, network_dim=128, **ok)
    with pytest.raises(ValueError, match="shape"):
        TrainableBCPolicyDim(wide, **ok)
    with pytest.raises(ValueError, match="TrainableBCPolicy: network_dim must be 64"):
        TrainableBCPolicy(wide, network_dim=128, **ok)
    with pytest.raises(ValueError, match="head_dim"):
        TrainableBCPolicyDim(wide, network_dim=128, head_dim=128, **ok)
    obs, pm, rm, expert, _, _, _ = BC.inputs(2, A, R)
    with pytest.raises(ValueError, match="no host path"):
        tbp(*[torch.from_numpy(a) for a in (obs, pm, rm, expert)])
