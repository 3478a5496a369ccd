"""CPU suite of the training-mode dropout of the device policy: the C interface and its argument checks, the host-side
refusals of the three classes, and the masked stand-in module against `nn.Dropout` -- which pins that the reference module's
dropout sits at exactly the four sites the kernels mask.  The kernels themselves are tested in test_gpu_policy_dropout.py and
test_gpu_ppo_dropout.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from gpudrive_lab_amd import _capi
from tests import dropout_reference as DREF
from tests import policy_cases as PC
from tests.conftest import ROOT

NEW = ("gd_policy_forward_dropout", "gd_policy_evaluate_dropout", "gd_policy_backward_dropout", "gd_ppo_update_dropout")


def test_the_header_declares_the_struct_and_the_entry_points_and_null_is_refused():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "typedef struct gd_dropout {" in header and "csrc/dropout_rule.hpp" in header
    for line in ("    uint64_t seed;", "    const uint64_t *call;", "    uint64_t *used;", "    uint32_t threshold;", "    float scale;"):
        assert line in header, line
    assert "int gd_policy_forward_dropout(const gd_policy *p, const gd_dropout *d, const float *obs, " in header
    assert "int gd_policy_evaluate_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_dropout *d, " in header
    assert "int gd_policy_backward_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_dropout *d, " in header
    assert "int gd_ppo_update_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, const gd_dropout *d, " in header
    assert set(NEW) <= set(_capi.SYMBOLS)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    D = _capi.GdDropout
    assert C.sizeof(D) == 32
    assert [getattr(D, n).offset for n in ("seed", "call", "used", "threshold", "scale")] == [0, 8, 16, 24, 28]
    L = _capi.lib()
    assert [len(getattr(L, n).argtypes) for n in NEW] == [11, 9, 10, 11]
    for name in NEW:
        fn = getattr(L, name)
        assert fn(*[0 if t is C.c_int32 else None for t in fn.argtypes]) == _capi.GD_ERR_INVALID
        assert name[:-len("_dropout")].encode() in L.gd_last_error()


def test_the_entry_points_check_the_dropout_struct_without_a_device():
    """Nothing is launched: every call below stops at a check."""
    from gpudrive_lab_amd.policy import grad_floats, pack_index
    L = _capi.lib()
    ok = 0x1000

    def structs():
        p, g = _capi.GdPolicy(), _capi.GdPolicyGrad()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = 3, 64, 6, 7
        p.blob, p.blob_floats, p.features, p.logits = ok, len(pack_index(6, 7)), ok, ok
        g.features = g.logits = g.winners = g.params = g.rowstat = g.partials = ok
        g.grad_floats, g.num_partials = grad_floats(6, 7), 4
        return p, g

    def drop(**kw):
        d = _capi.GdDropout()
        d.seed, d.call, d.used, d.threshold, d.scale = 1, ok, ok + 8, 655, 1.0 / 0.99
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def calls(d):
        p, g = structs()
        yield "gd_policy_forward_dropout", L.gd_policy_forward_dropout(C.byref(p), C.byref(d), ok, ok, 0, ok, ok, ok, ok, None, None)
        yield "gd_policy_evaluate_dropout", L.gd_policy_evaluate_dropout(C.byref(p), C.byref(g), C.byref(d), ok, ok, ok, ok, ok, None)
        yield "gd_policy_backward_dropout", L.gd_policy_backward_dropout(C.byref(p), C.byref(g), C.byref(d), ok, ok, ok, ok, ok, ok, None)

    for kw, word in ((dict(call=None), b"call and used"), (dict(used=None), b"call and used"), (dict(call=ok + 4), b"8-byte"),
                     (dict(used=ok + 4), b"8-byte"), (dict(threshold=0), b"threshold"), (dict(threshold=65536), b"threshold"),
                     (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale")):
        gen = calls(drop(**kw))
        for name, rc in gen:
            msg = L.gd_last_error()
            assert rc == _capi.GD_ERR_INVALID and word in msg and name.encode() in msg, (kw, name, msg)
    # the existing checks come first, under the new name
    p, g = structs()
    d = drop()
    assert L.gd_policy_forward_dropout(C.byref(p), C.byref(d), ok, ok, 0, ok + 4, ok, ok, ok, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_policy_forward_dropout" in L.gd_last_error() and b"8-byte aligned" in L.gd_last_error()
    p.max_agents = 100
    assert L.gd_policy_evaluate_dropout(C.byref(p), C.byref(g), C.byref(d), ok, ok, ok, ok, ok, None) == _capi.GD_ERR_INVALID
    assert b"max_agents" in L.gd_last_error()
    # gd_ppo_update_dropout: ppo's own checks, under the new name
    p, g = structs()
    o = _capi.GdPPO()
    assert L.gd_ppo_update_dropout(C.byref(p), C.byref(g), C.byref(o), C.byref(d), ok, ok, ok, ok, ok, ok, None) == _capi.GD_ERR_INVALID
    assert b"gd_ppo_update_dropout" in L.gd_last_error()


def test_the_classes_refuse_on_the_host(monkeypatch):
    from gpudrive_lab_amd.policy import DevicePolicy, TrainablePolicy
    from gpudrive_lab_amd.ppo import DevicePPO
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library is not needed for a refusal"))
    sd = PC.state_dict(1, 6, 7)
    kw = dict(max_agents=64, ego_width=6)
    for bad in (0.01, "rule", object(), True):
        with pytest.raises(ValueError, match="dropout_rule"):
            DevicePolicy.from_state_dict(sd, dropout_rule=bad, **kw)
        with pytest.raises(ValueError, match="dropout_rule"):
            TrainablePolicy.from_state_dict(sd, dropout_rule=bad, **kw)
        with pytest.raises(ValueError, match="dropout_rule"):
            DevicePPO(sd, minibatch_size=4, dropout_rule=bad, **kw)
    # the numeric keyword keeps refusing, and now points at the new argument
    with pytest.raises(ValueError, match="dropout_rule=DropoutRule"):
        TrainablePolicy.from_state_dict(sd, dropout=0.01, **kw)
    with pytest.raises(ValueError, match="dropout_rule=DropoutRule"):
        DevicePPO(sd, minibatch_size=4, dropout=0.01, **kw)
    # a host module without a rule has the train / eval switch of any module
    tp = TrainablePolicy.from_state_dict(sd, **kw)
    assert tp.dropout_rule is None and tp.training and not tp.eval().training


@pytest.mark.parametrize("a,ew,na", [(64, 6, 7), (64, 9, 91)])
def test_the_masked_stand_in_is_the_module_with_dropout_at_the_four_sites(a, ew, na):
    """`StandIn` (the reference module's layers) in train mode with nn.Dropout(0.5): the masks torch drew are read off the four
    Dropout layers by hooks and handed to the masked stand-in, which must then return the same outputs -- kept * 1 / (1 - p),
    dropped 0, at these four places and nowhere else.  In eval mode both are the unmasked module."""
    n, p = 3, 0.5
    sd = PC.state_dict(5, ew, na)
    obs = torch.from_numpy(PC.observations(6, n, a, ew)).double()
    net = PC.StandIn(a, ew, na, dropout=p).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    drops = [m for m in net.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) == 4 and [m for m in (net.ego_embed[3], net.partner_embed[3], net.road_map_embed[3], net.shared_embed[1])] == drops
    seen = {}

    def hook(name):
        def fn(mod, inp, out):
            x = inp[0]
            assert (x != 0).all()                       # so that a zero output is a dropped element
            keep = out != 0
            assert torch.equal(out, torch.where(keep, x * (1.0 / (1.0 - p)), torch.zeros_like(x)))
            seen[name] = keep.numpy()
        return fn

    for name, mod in zip(DREF.SITES, drops):
        mod.register_forward_hook(hook(name))
    net.train()
    torch.manual_seed(11)
    with torch.no_grad():
        want_l, want_v = net(obs)
    assert seen["ego"].shape == (n, 64) and seen["partner"].shape == (n, a - 1, 64) and seen["road"].shape == (n, 200, 64) \
        and seen["shared"].shape == (n, 128)
    assert all(0.3 < 1 - k.mean() < 0.7 for k in seen.values())
    got_l, got_v = DREF.forward(sd, obs.numpy(), a, ew, torch.float64, seen, 1.0 / (1.0 - p))
    assert np.array_equal(got_l, want_l.numpy()) and np.array_equal(got_v, want_v.numpy()[:, 0])
    # eval mode: the masks are ignored, and the module is the unmasked one
    masked = DREF.masked_stand_in(sd, a, ew, torch.float64, seen, 1.0 / (1.0 - p)).eval()
    with torch.no_grad():
        e_l, e_v = masked(obs)
    w_l, w_v = PC.stand_in_forward(sd, obs.numpy(), a, ew, torch.float64)
    assert np.array_equal(e_l.numpy(), w_l) and np.array_equal(e_v.numpy()[:, 0], w_v)
    assert not np.array_equal(got_l, w_l)
    # all-kept masks with scale 1 are the unmasked module too
    k_l, k_v = DREF.forward(sd, obs.numpy(), a, ew, torch.float64, DREF.all_kept(n, a), 1.0)
    assert np.array_equal(k_l, w_l) and np.array_equal(k_v, w_v)
