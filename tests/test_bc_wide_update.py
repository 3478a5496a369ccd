"""The device BC update at network_dim 128 without a GPU: `gd_bc_adamw_dim` and `gd_bc_update_dim`'s declarations, bindings and
refusals (junk pointers: every call stops at a check, nothing is launched); `blob_of(network_dim=128)` as the inverse of the
128-wide layout; the rule's host program (csrc/bc_opt_rule.hpp) against torch in float64 at the sizes the reference sweep's
model brings (G = 1,399,274 parameters in T = 252 tensors, the largest of 24,576 floats); `DeviceBCDim`'s surface and host-side
refusals.  The kernels are tested in test_gpu_bc_wide_update.py.

The yardstick and the bound of the rule's test are tests/test_bc_update.py's (C_ADAMW = 2 times the error of float32 torch
against float64, floored at 2^-23 max |float64|): nothing in the rule depends on the width."""
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
from . import bc_update_reference as UR
from . import bc_wide_cases as WC
from . import bc_wide_update_reference as WUR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ADAMW = 2  # tests/test_bc_update.py's
OK = WUR.OK
INVALID = _capi.GD_ERR_INVALID


# ---- declarations and bindings

def test_both_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "int gd_bc_adamw_dim(const gd_bc_opt *opt, int32_t network_dim, const float *grad, void *stream);" in header
    assert re.search(r"\bint gd_bc_update_dim\(const gd_bc_policy_dim \*p, const gd_bc_grad \*g, const gd_bc_opt \*opt,", header)
    assert {"gd_bc_adamw_dim", "gd_bc_update_dim"} <= set(_capi.SYMBOLS)
    L = _capi.lib()
    assert L.gd_bc_update_dim.argtypes[0]._type_ is _capi.GdBCPolicyDim and L.gd_bc_update.argtypes[0]._type_ is _capi.GdBCPolicy
    assert len(L.gd_bc_update_dim.argtypes) == len(L.gd_bc_update.argtypes) == 9
    assert L.gd_bc_update_dim.argtypes[1:] == L.gd_bc_update.argtypes[1:]
    assert L.gd_bc_adamw_dim.argtypes == [L.gd_bc_adamw.argtypes[0], C.c_int32] + L.gd_bc_adamw.argtypes[1:]
    # gd_bc_opt did not change: the width travels beside it
    assert C.sizeof(_capi.GdBCOpt) == 4 * 4 + 2 * 8 + 2 * 8 + 8 * 4 + 18 * 8 and _capi.GdBCOpt.tensor_end.offset == 80
    assert C.sizeof(_capi.GdBCPolicyDim) == C.sizeof(_capi.GdBCPolicy) + 8


# ---- the refusals, with junk pointers

def _update_dim(pd, g, o, n=3, obs=OK, pm=OK, rm=OK, expert=OK):
    L = _capi.lib()
    ref = lambda s: None if s is None else C.byref(s)  # noqa: E731
    rc = L.gd_bc_update_dim(ref(pd), ref(g), ref(o), obs, pm, rm, n, expert, None)
    return rc, L.gd_last_error().decode()


def _adamw_dim(o, dim, grad=OK):
    L = _capi.lib()
    rc = L.gd_bc_adamw_dim(None if o is None else C.byref(o), dim, grad, None)
    return rc, L.gd_last_error().decode()


# gd_bc_update_dim's refusals at 128 IN ORDER: (where, field, value, the words of the refusal).  where: a struct ("pd", its
# "base", "g", "o"; field None: the struct itself is NULL) or "arg", a keyword of the call.  The first three are the _dim
# struct's, the rest gd_bc_update's own in its order: the NULL structs, the row scratch, the forward's checks, the rows', the
# backward's, the optimiser's, then what ties the structs together
ORDER = [
    ("pd", None, None, "null argument"),
    ("pd", "network_dim", 96, "network_dim must be 64 or 128"),
    ("pd", "reserved", 1, "reserved must be 0"),
    ("g", None, None, "null argument"),
    ("o", "actions", None, "null argument (expert_actions, or opt's actions, nll, grad_nll or grad)"),
    ("arg", "pm", None, "null argument"),
    ("base", "max_agents", 96, "max_agents must be 64 or 128"),
    ("base", "num_stack", 9, "num_stack must be in [1, 8]"),
    ("base", "fusion_layers", 5, "fusion_layers and branch_layers must be in [1, 4]"),
    ("base", "head_layers", 5, "head_layers must be in [0, 4]"),
    ("base", "n_components", 17, "n_components must be in [1, 16]"),
    ("base", "chunk_rows", 0, "chunk_rows must be in [1, 4096]"),
    ("arg", "n", 0, "n must be in [1, 2^20]"),
    ("base", "scratch", None, "blob and scratch are required"),
    ("base", "blob_floats", 5, "blob_floats is not the layout's size at network_dim 128"),
    ("base", "scratch_floats", 5, "scratch_floats is below chunk_rows * 3 * (max_agents + 200) * 128"),
    ("arg", "obs", OK + 2, "float and int32 buffers must be 4-byte aligned"),
    ("o", "stats", None, "stats and stats_sum are required"),
    ("o", "stats_sum", OK + 2, "float buffers must be 4-byte aligned"),
    ("g", "num_partials", 0, "num_partials must be in [1, 4096]"),
    ("g", "reserved", 1, "reserved must be 0"),
    ("g", "partials", None, "scratch and partials are required"),
    ("g", "grad_floats", 5, "grad_floats is not the parameters' count at network_dim 128"),
    ("g", "scratch_floats", 5, "grad scratch_floats is below blob_floats rounded up to 64 + chunk_rows * (max_agents + 200) * (128 *"),
    ("o", "grad", OK + 4, "grad scratch must be 256-byte aligned, partials and grad 16-byte aligned"),
    ("o", "num_stack", 0, "num_stack must be in [1, 8]"),
    ("o", "branch_layers", 0, "fusion_layers and branch_layers must be in [1, 4]"),
    ("o", "reserved", 1, "reserved must be 0"),
    ("o", "grad_floats", 5, "grad_floats is not the parameters' count at network_dim 128"),
    ("o", "blob_floats", 5, "blob_floats is not the layout's size at network_dim 128"),
    ("o", "num_tensors", 251, "num_tensors is not the state dict's tensor count"),
    ("o", "beta1", 1.0, "betas must be in [0, 1)"),
    ("o", "eps", 0.0, "eps and max_grad_norm must be positive"),
    ("o", "weight_decay", float("inf"), "weight_decay must be finite and not negative"),
    ("o", "blob_of", None, "tensor_end, lr, step, beta_pow, params, exp_avg, exp_avg_sq, blob, blob_of"),
    ("o", "beta_pow", OK + 4, "beta_pow and scal must be 8-byte aligned"),
    ("o", "max_rows", 0, "max_rows must be in [1, 2^20]"),
    ("o", "max_rows", 2, "n is above max_rows"),
    ("o", "blob", OK + 64, "the policy's blob must be opt's"),
]


def _broken(*breakers):
    pd, g, o = WUR.structs(128)
    s, kw, null = dict(pd=pd, base=pd.base, g=g, o=o), {}, set()
    for where, field, value, _ in breakers:
        if where == "arg":
            kw[field] = value
        elif field is None:
            null.add(where)
        else:
            setattr(s[where], field, value)
    return _update_dim(*(None if k in null else s[k] for k in ("pd", "g", "o")), **kw)


def test_update_dim_refuses_in_gd_bc_updates_order_at_128():
    """Each breaker alone gives its words under the entry's own name; together with any LATER breaker the earlier one still
    speaks -- that is the order.  (A later breaker of the same field would undo the earlier one and is skipped.)"""
    assert len(ORDER) >= 36
    for i, b in enumerate(ORDER):
        rc, why = _broken(b)
        assert rc == INVALID and why.startswith("gd_bc_update_dim: " + b[3]), (i, b[3], why)
    for i, b in enumerate(ORDER):
        for j in range(i + 1, len(ORDER)):
            if ORDER[j][:2] == b[:2]:
                continue
            rc, why = _broken(b, ORDER[j])
            assert rc == INVALID and why.startswith("gd_bc_update_dim: " + b[3]), (i, j, b[3], why)
    # p, g of one configuration, opt of another, each consistent in itself
    pd, g, _ = WUR.structs(128, "wide_min")
    rc, why = _update_dim(pd, g, WUR.structs(128, "wide_sweep")[2])
    assert rc == INVALID and why == "gd_bc_update_dim: the configurations and sizes of the policy, the backward and opt differ"
    # a null opt, and the other nulls of the call
    pd, g, o = WUR.structs(128)
    assert _update_dim(pd, g, None)[1] == "gd_bc_update_dim: null argument"
    assert _update_dim(pd, g, o, expert=None)[1].startswith("gd_bc_update_dim: null argument (expert_actions")
    for name in ("nll", "grad_nll", "grad"):
        assert _update_dim(*WUR.structs(128, **{name: None}))[1].startswith("gd_bc_update_dim: null argument (expert_actions")
    # the struct is looked at first: a bad network_dim speaks before a NULL beside it
    pd.network_dim = 96
    assert _update_dim(pd, None, None)[1] == "gd_bc_update_dim: network_dim must be 64 or 128"


def test_the_sizes_of_one_width_are_refused_at_the_other():
    L = _capi.lib()
    for dim, other, words in ((128, 64, " at network_dim 128 for these"), (64, 128, " for these")):
        pd, g, o = WUR.structs(dim)
        _, g2, o2 = WUR.structs(other)
        assert g.grad_floats != g2.grad_floats and o.blob_floats != o2.blob_floats
        # everything in order at this width: the last check of all speaks
        rc, why = _update_dim(pd, g, o, obs=OK + 2)
        assert rc == INVALID and "4-byte aligned" in why, why
        rc, why = _adamw_dim(o, dim, grad=OK + 2)
        assert rc == INVALID and why.startswith("gd_bc_adamw_dim: beta_pow and scal must be 8-byte aligned, the other"), why
        # gd_bc_adamw_dim: the optimiser's sizes of the other width
        rc, why = _adamw_dim(o2, dim)
        assert rc == INVALID and why.startswith("gd_bc_adamw_dim: grad_floats is not the parameters' count" + words), why
        o3 = WUR.structs(dim, blob_floats=o2.blob_floats)[2]
        rc, why = _adamw_dim(o3, dim)
        assert rc == INVALID and why.startswith("gd_bc_adamw_dim: blob_floats is not the layout's size" + words), why
        # gd_bc_update_dim: the policy's blob, the backward's gradient, the optimiser's two sizes
        pd.base.blob_floats = o2.blob_floats
        assert _update_dim(pd, g, o)[1].startswith("gd_bc_update_dim: blob_floats is not the layout's size" + words)
        pd, g, o = WUR.structs(dim)
        g.grad_floats = g2.grad_floats
        assert _update_dim(pd, g, o)[1].startswith("gd_bc_update_dim: grad_floats is not the parameters' count" + words)
        for field in ("grad_floats", "blob_floats"):
            pd, g, o = WUR.structs(dim, **{field: getattr(o2, field)})
            assert _update_dim(pd, g, o)[1].startswith("gd_bc_update_dim: %s is not the " % field), field
    for dim in (96, 0, -128, 256):
        rc, why = _adamw_dim(WUR.structs(128)[2], dim)
        assert rc == INVALID and why == "gd_bc_adamw_dim: network_dim must be 64 or 128", (dim, why)
    # the width is looked at first
    assert _adamw_dim(None, 96)[1] == "gd_bc_adamw_dim: network_dim must be 64 or 128"
    assert _adamw_dim(None, 128)[1] == "gd_bc_adamw_dim: null argument"
    assert _adamw_dim(WUR.structs(128)[2], 128, grad=None)[1] == "gd_bc_adamw_dim: null argument"
    for kw, words in ((dict(num_stack=9), "num_stack"), (dict(reserved=1), "reserved must be 0"), (dict(num_tensors=288), "num_tensors"),
                      (dict(beta2=-0.1), "betas"), (dict(max_grad_norm=0.0), "max_grad_norm"), (dict(weight_decay=-0.01), "weight_decay"),
                      (dict(scal=None), "are required"), (dict(scal=OK + 4), "aligned")):
        rc, why = _adamw_dim(WUR.structs(128, **kw)[2], 128)
        assert rc == INVALID and why.startswith("gd_bc_adamw_dim: ") and words in why, (kw, why)
    # gd_bc_adamw and gd_bc_update answer as before: 64 only, under their own names, with their own words
    pd, g, o = WUR.structs(128)
    assert L.gd_bc_adamw(C.byref(o), OK, None) == INVALID
    assert L.gd_last_error().decode() == ("gd_bc_adamw: grad_floats is not the parameters' count for these layer counts, num_stack "
                                          "and n_components")
    assert L.gd_bc_update(C.byref(pd.base), C.byref(g), C.byref(o), OK, OK, OK, 3, OK, None) == INVALID
    assert L.gd_last_error().decode() == ("gd_bc_update: blob_floats is not the layout's size for these layer counts, num_stack and "
                                          "n_components")
    pd, g, o = WUR.structs(64)
    assert L.gd_bc_update(C.byref(pd.base), C.byref(g), C.byref(o), OK + 2, OK, OK, 3, OK, None) == INVALID
    assert L.gd_last_error().decode() == "gd_bc_update: float and int32 buffers must be 4-byte aligned"
    assert L.gd_bc_adamw(C.byref(o), OK + 2, None) == INVALID and L.gd_last_error().decode().startswith("gd_bc_adamw: beta_pow and scal")
    assert L.gd_bc_update(None, None, None, None, None, None, 1, None, None) == INVALID
    assert L.gd_last_error().decode() == "gd_bc_update: null argument"
    assert L.gd_bc_adamw(None, None, None) == INVALID and L.gd_last_error().decode() == "gd_bc_adamw: null argument"


# ---- the layout

@pytest.mark.parametrize("name", ["wide_min", "wide_sweep", "wide_a128"])
def test_blob_of_inverts_the_wide_layout(name):
    from gpudrive_lab_amd.bc_opt import blob_of, tensor_end
    _, _, R, cfg = WC.CASES[name]
    lay = WUR.layout_args(R, cfg)
    index, inv = BP.pack_index(*lay, network_dim=128), blob_of(*lay, network_dim=128)
    G = BT.grad_floats(*lay, network_dim=128)
    assert inv.dtype == np.int32 and inv.shape == (G,)
    assert np.array_equal(index[inv], np.arange(G)), "pack_index[blob_of] is the identity"
    place = np.zeros(len(index), bool)
    place[inv] = True
    assert place.sum() == G, "one to one"
    assert np.array_equal(place, index != G), "onto the places that are no padding"
    assert (index[~place] == G).all() and (~place).sum() == len(index) - G
    end = tensor_end(WC.shapes(R, cfg))
    names, end2, G2 = WUR.layout(name)
    assert end.dtype == np.int32 and np.array_equal(end, end2) and end[-1] == G == G2 and (np.diff(end) > 0).all()
    assert len(end) == len(names) == 48 + 16 * (cfg["num_layer"][0] + 2 * cfg["num_layer"][1]) + 36 + 2 * (cfg["head_num_layers"] + 2)
    # another width's inverse is another map
    assert blob_of(*lay).shape[0] == BT.grad_floats(*lay) < G
    if name == "wide_sweep":
        assert G == WUR.SWEEP_G and len(end) == WUR.SWEEP_T
        sizes = np.diff(np.concatenate([[0], end]))
        assert sizes.max() == sizes[names.index(WUR.LARGEST)] == 64 * 384 == 96 * 256, "a k_bc_sq lane owns 96 elements"


def test_no_accepted_layer_count_has_more_tensors_than_the_step_kernel_holds():
    most = 0
    for f in range(1, 5):
        for b in range(1, 5):
            for hl in range(0, 5):
                T = len(BP.expected_shapes(1, (f, b), hl, 1, network_dim=128))
                assert T == 48 + 16 * (f + 2 * b) + 36 + 2 * (hl + 2) == len(BP.expected_shapes(1, (f, b), hl, 1))
                most = max(most, T)
    assert most == 288  # bc_opt_rule::MAX_TENSORS
    rule = open(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "bc_opt_rule.hpp")).read()
    assert "constexpr int MAX_TENSORS = 288;" in rule


def test_blob_of_refuses_a_wide_layout_that_is_no_permutation(monkeypatch):
    from gpudrive_lab_amd import bc_opt
    _, _, R, cfg = WC.CASES["wide_min"]
    lay = WUR.layout_args(R, cfg)
    index = BP.pack_index(*lay, network_dim=128)
    twice = index.copy()
    twice[np.flatnonzero(index == 7)[0]] = 8       # parameter 7 has no place, parameter 8 two
    seen = []
    monkeypatch.setattr(bc_opt.BP, "pack_index", lambda *a, **kw: (seen.append(kw), twice)[1])
    with pytest.raises(ValueError, match="exactly one place"):
        bc_opt.blob_of(*lay, network_dim=128)
    assert seen == [dict(network_dim=128)]


# ---- the rule at this size

def test_the_adamw_rule_against_float64_at_the_sweeps_layout():
    """tests/test_bc_update.py's test of the rule on the sweep's 128-wide layout: 1.4 M parameters in 252 tensors, the largest
    tensor (24,576 floats: 96 elements per partial sum) planted as the tensor of the largest norm, one whole tensor of zeros."""
    names, end, G = WUR.layout("wide_sweep")
    assert G == WUR.SWEEP_G and len(end) == WUR.SWEEP_T
    grads, zt, largest = WUR.planted_gradients("wide_sweep")
    norms = [float(np.linalg.norm(g.astype(np.float64))) for g in grads]
    assert norms[0] > 20 + 1 and norms[1] < 20 - 1 and norms[2] > 20 + 1
    zeros = slice(int(end[zt - 1]), int(end[zt]))
    assert (grads[0][zeros] == 0).all() and zeros.stop - zeros.start == 4096
    for g in grads:   # the condition on the inputs: no float32 rounding can change which tensor is the largest
        n64 = UR.tensor_norms64(g, end)
        top = np.sort(n64)[-2:]
        assert int(np.argmax(n64)) == largest and top[1] - top[0] > 1e-3 * top[1], top
    p0 = np.random.default_rng(5).normal(0.0, 0.1, G).astype(np.float32)
    z = np.zeros(G, np.float32)
    host = UR.run_adamw_host(p0, z, z, grads, end, **UR.ADAMW)
    r64 = UR.adamw_reference(p0, grads, end, torch.float64, **UR.ADAMW)
    r32 = UR.adamw_reference(p0, grads, end, torch.float32, **UR.ADAMW)
    worst = 0.0
    for s in range(3):
        what = "step %d" % (s + 1)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            err, E = UR.error_floor(host[s][k], r64[s][k], r32[s][k])
            ratio = UR.ratio_of(err, E)
            worst = max(worst, ratio)
            print("BCWIDEOPT RATIO adamw %s %s err %.3e E %.3e ratio %.2f" % (what, k, err, E, ratio))
            assert err <= C_ADAMW * E, (what, k, "error %.3g above %d E = %.3g" % (err, C_ADAMW, C_ADAMW * E))
        n64 = UR.tensor_norms64(grads[s], end)
        assert (np.abs(host[s]["tensor_norms"] - n64) <= 2.0 ** -22 * n64).all(), what
        assert abs(float(host[s]["total"]) - r64[s]["total"]) <= 2.0 ** -22 * r64[s]["total"], what
        assert abs(float(host[s]["total"]) - norms[s]) <= 2.0 ** -22 * norms[s], what
        assert abs(float(host[s]["max_grad_norm"]) - r64[s]["max_grad_norm"]) <= 2.0 ** -21 * r64[s]["max_grad_norm"], what
        assert host[s]["max_grad_tensor"] == largest == r64[s]["max_grad_tensor"], what
        assert host[s]["step"] == s + 1
        assert host[s]["beta_pow"][0] == pytest.approx(0.9 ** (s + 1), rel=1e-15)
        assert host[s]["beta_pow"][1] == pytest.approx(0.999 ** (s + 1), rel=1e-15)
    print("BCWIDEOPT WORST adamw %.2f" % worst)
    assert host[0]["tensor_norms"][zt] == 0
    decay = np.float32(1.0 - float(np.float32(UR.ADAMW["lr"])) * float(np.float32(UR.ADAMW["weight_decay"])))
    assert np.array_equal(host[0]["params"][zeros], p0[zeros] * decay)
    assert (host[0]["exp_avg"][zeros] == 0).all() and (host[0]["exp_avg_sq"][zeros] == 0).all()


# ---- DeviceBCDim's surface without a device

def test_device_bc_dim_surface_and_refusals(monkeypatch):
    import gpudrive_lab_amd
    from gpudrive_lab_amd.bc_opt import DeviceBC, DeviceBCDim
    assert gpudrive_lab_amd.DeviceBCDim is DeviceBCDim and issubclass(DeviceBCDim, DeviceBC)
    assert DeviceBC.NETWORK_DIMS == (64,) and DeviceBCDim.NETWORK_DIMS == (64, 128)
    assert "partials" in DeviceBCDim.__doc__ and "partials" in DeviceBC.nbytes.__doc__ and "716 MB" in DeviceBC.nbytes.__doc__
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library is not needed for a refusal"))
    _, A, R, cfg = WC.CASES["wide_min"]
    wide, narrow = BC.state_dict(R, cfg, network_dim=128), BC.state_dict(R, cfg)
    ok = dict(max_agents=A, num_stack=R, num_head=4, batch_size=4, **cfg)
    for kw, words in ((dict(network_dim=96), "DeviceBC: network_dim must be 64 or 128"), (dict(head_dim=128), "DeviceBC: head_dim"),
                      (dict(dropout=0.1), "DeviceBC: dropout"), (dict(max_agents=100), "DeviceBC: max_agents"),
                      (dict(batch_size=0), "DeviceBC: batch_size"), (dict(betas=(1.0, 0.999)), "DeviceBC: betas"),
                      (dict(eps=0.0), "DeviceBC: eps"), (dict(weight_decay=-0.01), "DeviceBC: weight_decay"),
                      (dict(partials=4097), "DeviceBC: partials"), (dict(amsgrad=True), "DeviceBC: unknown argument")):
        with pytest.raises(ValueError, match=re.escape(words)):
            DeviceBCDim(wide, **dict(dict(ok, network_dim=128), **kw))
    with pytest.raises(ValueError, match="shape"):
        DeviceBCDim(narrow, network_dim=128, **ok)
    with pytest.raises(ValueError, match="shape"):
        DeviceBCDim(wide, **ok)
    with pytest.raises(ValueError, match="DeviceBC: network_dim must be 64 "):
        DeviceBC(wide, network_dim=128, **ok)
    for bad in ({k: v for k, v in wide.items() if k != "head.head.bias"}, dict(wide, extra=torch.zeros(1))):
        with pytest.raises(ValueError, match="key"):
            DeviceBCDim(bad, network_dim=128, **ok)
    # a wide state dict passes every host check and stops at the device's
    for sd, kw in ((wide, dict(network_dim=128)), (narrow, {}), (narrow, dict(network_dim=64))):
        with pytest.raises(ValueError, match="GPU"):
            DeviceBCDim(sd, device="cpu", **ok, **kw)
