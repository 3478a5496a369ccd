"""CPU suite of the device PPO update: the C interface and its argument checks, `blob_of`, the host-side refusals of
`DevicePPO`, and the rule's header (csrc/ppo_rule.hpp) run on the host against torch in float64.  The kernels themselves are
tested in test_gpu_ppo_update.py.

The yardstick is the project's: E of a quantity is the error of the same lines in torch float32 on the CPU against float64,
floored at 2^-23 max |float64|; the host program must stay within C E.  C_LOSS and C_ADAM are the next power of two at or
above twice the largest ratio measured over all cases below (DESIGN.md section 5 tabulates them):
  loss  largest ratio 1.28 (policy_loss, M = 1025, norm_adv on)                        -> C_LOSS = 4
  adam  largest ratio 0.74 (the parameters after the third step)                       -> C_ADAM = 2"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import policy_cases as PC
from tests import ppo_update_reference as UR
from tests.conftest import ROOT

C_LOSS = 4
C_ADAM = 2
SHAPES = ((6, 91), (9, 7), (6, 31))


# ---- the C interface

def test_the_header_declares_the_entry_points_and_null_is_refused():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "int gd_ppo_loss(const gd_ppo *ppo, " in header and "int gd_ppo_adam(const gd_ppo *ppo, " in header
    assert "int gd_ppo_update(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, " in header
    assert "typedef struct gd_ppo {" in header and "csrc/ppo_rule.hpp" in header
    assert os.path.exists(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "ppo_rule.hpp"))
    names = {"gd_ppo_loss", "gd_ppo_adam", "gd_ppo_update"}
    assert names <= set(_capi.SYMBOLS)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_ppo_loss.argtypes) == 12 and len(L.gd_ppo_adam.argtypes) == 3 and len(L.gd_ppo_update.argtypes) == 10
    assert C.sizeof(_capi.GdPPO) == 12 * 4 + 2 * 8 + 2 * 8 + 18 * 8 and _capi.GdPPO.beta1.offset == 48
    assert len(_capi.PPO_STATS) == 7 and _capi.PPO_STATS[:6] == UR.STATS and _capi.PPO_STATS[6] == "grad_norm"
    assert L.gd_ppo_loss(*[None] * 12) == _capi.GD_ERR_INVALID and b"gd_ppo_loss" in L.gd_last_error()
    assert L.gd_ppo_adam(None, None, None) == _capi.GD_ERR_INVALID and b"gd_ppo_adam" in L.gd_last_error()
    assert L.gd_ppo_update(*[None] * 10) == _capi.GD_ERR_INVALID and b"gd_ppo_update" in L.gd_last_error()


def _structs(m=3, ew=6, na=7, **kw):
    from gpudrive_lab_amd.policy import grad_floats, pack_index
    ok = 0x1000
    p, g, o = _capi.GdPolicy(), _capi.GdPolicyGrad(), _capi.GdPPO()
    p.num_rows, p.max_agents, p.ego_width, p.n_actions = m, 64, ew, na
    p.blob, p.blob_floats = ok, len(pack_index(ew, na))
    g.features = g.logits = g.winners = g.params = g.rowstat = g.partials = ok
    g.grad_floats, g.num_partials = grad_floats(ew, na), 4
    o.num_rows, o.ego_width, o.n_actions, o.norm_adv, o.clip_vloss = m, ew, na, 1, 0
    o.clip_coef, o.vf_clip_coef, o.ent_coef, o.vf_coef, o.max_grad_norm, o.eps, o.stats_scale = 0.2, 0.2, 1e-4, 0.3, 0.5, 1e-5, 1.0
    o.beta1, o.beta2 = 0.9, 0.999
    o.grad_floats, o.blob_floats = grad_floats(ew, na), len(pack_index(ew, na))
    for name, _ in _capi.GdPPO._fields_[16:]:
        setattr(o, name, ok)
    for k, v in kw.items():
        for s in (p, g, o):
            if k in dict(s._fields_) and (k not in ("num_rows", "ego_width", "n_actions") or s is o):
                setattr(s, k, v)
    return p, g, o


def test_the_entry_points_check_their_arguments_without_a_device():
    """Nothing is launched: every call below stops at a check (the last one of each group at a pointer's alignment, which is
    checked after everything else)."""
    L = _capi.lib()
    ok = 0x1000
    rows = [ok] * 10

    def loss(o, args=rows):
        return L.gd_ppo_loss(C.byref(o), *args, None), L.gd_last_error()

    for kw, msg in ((dict(num_rows=0), b"num_rows"), (dict(num_rows=(1 << 20) + 1), b"num_rows"), (dict(num_rows=1), b"norm_adv"),
                    (dict(stats=None), b"stats"), (dict(stats_sum=None), b"stats"), (dict(stats=ok + 2), b"aligned")):
        rc, err = loss(_structs(**kw)[2])
        assert rc == _capi.GD_ERR_INVALID and msg in err, (kw, err)
    for i in range(10):
        rc, err = loss(_structs()[2], [None if j == i else ok for j in range(10)])
        assert rc == _capi.GD_ERR_INVALID and b"null" in err
        rc, err = loss(_structs()[2], [ok + 2 if j == i else ok for j in range(10)])
        assert rc == _capi.GD_ERR_INVALID and b"aligned" in err
    o = _structs(num_rows=1, norm_adv=0)[2]
    rc, err = loss(o, [ok + 1] + rows[1:])
    assert rc == _capi.GD_ERR_INVALID and b"aligned" in err, "one row without norm_adv passes every check before alignment"

    def adam(o, grad=ok):
        return L.gd_ppo_adam(C.byref(o), grad, None), L.gd_last_error()

    bad = [(dict(ego_width=7), b"ego_width"), (dict(n_actions=0), b"n_actions"), (dict(n_actions=1025), b"n_actions"),
           (dict(grad_floats=5), b"grad_floats"), (dict(blob_floats=5), b"blob_floats"), (dict(beta1=1.0), b"betas"),
           (dict(beta2=-0.1), b"betas"), (dict(beta1=float("nan")), b"betas"), (dict(eps=0.0), b"eps"),
           (dict(max_grad_norm=0.0), b"max_grad_norm"), (dict(beta_pow=ok + 4), b"aligned"), (dict(blob_of=ok + 2), b"aligned")]
    bad += [({name: None}, b"required") for name in ("lr", "step", "beta_pow", "params", "exp_avg", "exp_avg_sq", "blob",
                                                      "blob_of", "stats", "stats_sum", "scal")]
    for kw, msg in bad:
        rc, err = adam(_structs(**kw)[2])
        assert rc == _capi.GD_ERR_INVALID and msg in err, (kw, err)
    rc, err = adam(_structs()[2], None)
    assert rc == _capi.GD_ERR_INVALID and b"null" in err
    rc, err = adam(_structs()[2], ok + 2)
    assert rc == _capi.GD_ERR_INVALID and b"aligned" in err

    def update(p, g, o, args=(ok,) * 6):
        return L.gd_ppo_update(C.byref(p), C.byref(g), C.byref(o), *args, None), L.gd_last_error()

    for kw in bad:
        rc, err = update(*_structs(**kw[0]))
        assert rc == _capi.GD_ERR_INVALID and b"gd_ppo_update" in err, (kw, err)
    for name in ("newlogprob", "entropy", "newvalue", "d_logprob", "d_entropy", "d_value", "grad"):
        rc, err = update(*_structs(**{name: None}))
        assert rc == _capi.GD_ERR_INVALID and b"null" in err, (name, err)
    for kw, msg in ((dict(num_rows=4), b"differ"), (dict(n_actions=8, grad_floats=_structs(na=8)[2].grad_floats,
                                                         blob_floats=_structs(na=8)[2].blob_floats), b"differ"),
                    (dict(blob=ok + 64), b"must be ppo's"), (dict(num_partials=0), b"num_partials")):
        p, g, o = _structs()
        for k, v in kw.items():
            setattr(g if k == "num_partials" else o, k, v)
        rc, err = update(p, g, o)
        assert rc == _capi.GD_ERR_INVALID and msg in err, (kw, err)
    for i in range(6):
        rc, err = update(*_structs(), [None if j == i else ok for j in range(6)])
        assert rc == _capi.GD_ERR_INVALID and b"null" in err


def test_blob_of_inverts_pack_index():
    from gpudrive_lab_amd.policy import grad_floats, pack_index
    from gpudrive_lab_amd.ppo import blob_of
    for ew, na in SHAPES + ((9, 1024),) + tuple((6 if i % 2 == 0 else 9, na) for i, na in enumerate(PC.EDGE_ACTIONS)):
        index, inv, G = pack_index(ew, na), blob_of(ew, na), grad_floats(ew, na)
        assert inv.dtype == np.int32 and inv.shape == (G,)
        assert (np.bincount(index, minlength=G + 1)[:G] == 1).all()
        assert np.array_equal(index[inv], np.arange(G)) and len(set(inv.tolist())) == G
        assert (index == G).sum() == len(index) - G
    assert (pack_index(6, 31) == grad_floats(6, 31)).sum() == 64


# ---- the host-side refusals

def test_the_constructor_refuses_on_the_host(monkeypatch):
    from gpudrive_lab_amd.ppo import DevicePPO
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library is not needed for a refusal"))
    sd = PC.state_dict(1, 6, 7)
    base = dict(max_agents=64, ego_width=6, minibatch_size=16)
    for kw in (dict(target_kl=0.01), dict(dropout=0.01), dict(dropout=True), dict(minibatch_size=1), dict(minibatch_size=0),
               dict(minibatch_size=(1 << 20) + 1), dict(minibatch_size=16.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
               dict(betas=(0.9,)), dict(betas=0.9), dict(betas=(0.9, float("nan"))), dict(eps=0.0), dict(eps=-1e-5),
               dict(max_grad_norm=0.0), dict(learning_rate=0.0), dict(learning_rate=-1.0), dict(learning_rate=None),
               dict(clip_coef=float("inf")), dict(partials=0), dict(partials=1025), dict(max_agents=100), dict(ego_width=7),
               dict(act_func="gelu"), dict(vbd_in_obs=True), dict(device="cpu"), dict(device="no such device")):
        with pytest.raises(ValueError):
            DevicePPO(sd, **dict(base, **kw))
    for bad in ({k: v for k, v in sd.items() if k != "critic.bias"}, dict(sd, extra=torch.zeros(1)),
                dict(sd, **{"actor.bias": sd["actor.bias"].double()}),
                dict(sd, **{"actor.weight": torch.zeros(1025, 128), "actor.bias": torch.zeros(1025)})):
        with pytest.raises(ValueError):
            DevicePPO(bad, **base)
    # one row is refused only with norm_adv: without it the arguments pass, and the refusal is the device's
    with pytest.raises(ValueError, match="GPU"):
        DevicePPO(sd, **dict(base, minibatch_size=1, norm_adv=False, device="cpu"))


def test_update_and_train_refuse_on_the_host():
    from gpudrive_lab_amd.ppo import check_train_args, check_update_args
    from gpudrive_lab_amd.rollout import DeviceRollout
    M, D, dev = 16, 11, torch.device("cpu")  # (the checks compare devices; they touch none)
    f = torch.float32

    def args(**kw):
        a = dict(obs=torch.zeros(M, D), actions=torch.zeros(M, dtype=torch.int64), logprobs=torch.zeros(M), values=torch.zeros(M),
                 advantages=torch.zeros(M), returns=torch.zeros(M))
        a.update(kw)
        return list(a.values())

    assert len(check_update_args(M, D, dev, *args())) == 6
    views = args(obs=torch.zeros(8, 2, D), actions=torch.zeros(8, 2, dtype=torch.int64), logprobs=torch.zeros(8, 2))
    assert len(check_update_args(M, D, dev, *views)) == 6
    for kw in (dict(obs=torch.zeros(M, D + 1)), dict(obs=torch.zeros(M + 1, D)), dict(obs=torch.zeros(M, D, dtype=torch.float64)),
               dict(obs=torch.zeros(D, M).t()), dict(obs=torch.zeros(4, 2, D)), dict(actions=torch.zeros(M, dtype=torch.int32)),
               dict(actions=torch.zeros(4, 4, dtype=torch.int64)), dict(logprobs=torch.zeros(M + 1)), dict(values=torch.zeros(M, 1)),
               dict(advantages=torch.zeros(M, dtype=torch.float16)), dict(returns=None), dict(returns=np.zeros(M, np.float32))):
        with pytest.raises(ValueError):
            check_update_args(M, D, dev, *args(**kw))
    with pytest.raises(ValueError):
        check_update_args(M, D, torch.device("cuda", 0), *args())     # tensors on another device
    with pytest.raises(ValueError):
        check_update_args(M, D, dev, *args()[:5])

    ro = object.__new__(DeviceRollout)
    ro.minibatch_size, ro.obs_width, ro.device, ro.action_shape = M, D, dev, ()
    check_train_args(ro, M, D, dev, 2)
    for kw in (dict(minibatch_size=8), dict(obs_width=D + 3), dict(device=torch.device("cuda", 0)), dict(action_shape=(3,))):
        other = object.__new__(DeviceRollout)
        other.__dict__.update(ro.__dict__, **kw)
        with pytest.raises(ValueError):
            check_train_args(other, M, D, dev, 2)
    for epochs in (0, -1, 2.0, None):
        with pytest.raises(ValueError):
            check_train_args(ro, M, D, dev, epochs)
    with pytest.raises(ValueError):
        check_train_args("a rollout", M, D, dev, 2)


# ---- the rule on the host

@pytest.mark.parametrize("m", UR.ROWS)
def test_the_loss_rule_against_float64(m):
    x = UR.loss_inputs(m)
    UR.assert_gaps(x, "M = %d" % m)
    nlp, _, _, old_lp, _, adv, _ = x
    one = np.flatnonzero(nlp == old_lp)
    assert len(one) >= 1 and (one % 5 == 1).all(), "rows with ratio exactly 1"
    ratio = np.exp(nlp.astype(np.float64) - old_lp)
    if m >= 70:
        assert (ratio < 0.8).any() and (ratio > 1.2).any() and ((ratio > 0.8) & (ratio < 1.2) & (ratio != 1)).any()
    worst = 0.0
    for norm_adv, clip_vloss in UR.FLAGS:
        what = "M = %d norm_adv %s clip_vloss %s" % (m, norm_adv, clip_vloss)
        r64 = UR.loss_reference(x, torch.float64, norm_adv, clip_vloss)
        r32 = UR.loss_reference(x, torch.float32, norm_adv, clip_vloss)
        got = UR.run_loss_host(x, norm_adv, clip_vloss)
        pairs = [(n, got[k], r64[k], r32[k]) for k, n in enumerate(("d_logprob", "d_entropy", "d_value"))]
        pairs += [(n, got[3][k], r64[3][k], r32[3][k]) for k, n in enumerate(UR.STATS)]
        for name, g, w64, w32 in pairs:
            assert np.isfinite(g).all(), (what, name)
            err, E = UR.error_floor(g, w64, w32)
            worst = max(worst, UR.ratio_of(err, E))
            assert err <= C_LOSS * E, (what, name, "error %.3g above %d E = %.3g" % (err, C_LOSS, C_LOSS * E))
        # ratio == 1: the unclipped branch, d_logprob = -adv' / M (ratio is exactly 1.0f, so float32 adds nothing)
        a = adv.astype(np.float64)
        a = (a - a.mean()) / (a.std(ddof=1) + 1e-8) if norm_adv else a
        assert np.abs(got[0][one] - (-a[one] / m)).max() <= 2.0 ** -21 * max(1.0, np.abs(a).max()) / m, what
        assert (r64[0][one] != 0).all(), (what, "the float64 reference agrees that those rows are not clipped")
        # d_entropy is the constant -ent_coef / M
        assert (got[1] == got[1][0]).all() and abs(got[1][0] + 0.01 / m) <= 2.0 ** -22 * 0.01 / m, what
    print("ppo loss rule M=%d: largest error / E %.2f" % (m, worst))


def test_the_adam_rule_against_float64():
    from gpudrive_lab_amd.policy import grad_floats
    G = grad_floats(6, 31)
    assert G % 256, "the last partial sums are shorter"
    p0 = np.random.default_rng(5).normal(0.0, 0.1, G).astype(np.float32)
    grads = UR.adam_gradients(G)
    norms = [float(np.linalg.norm(g.astype(np.float64))) for g in grads]
    assert norms[0] > 0.5 and norms[1] < 0.5 - 1e-3 and norms[2] > 0.5
    mags = np.abs(np.concatenate(grads))
    mags = mags[mags > 0]
    assert mags.min() < 2e-8 and mags.max() > 0.5 and (mags < 1e-6).any() and (mags > 1e-4).any(), "either side of eps"
    zeros = UR.zero_block(G)
    assert (grads[0][zeros] == 0).all()
    host = UR.run_adam_host(p0, np.zeros(G, np.float32), np.zeros(G, np.float32), grads, **UR.ADAM)
    r64 = UR.adam_reference(p0, grads, torch.float64, **UR.ADAM)
    r32 = UR.adam_reference(p0, grads, torch.float32, **UR.ADAM)
    worst = 0.0
    for s in range(3):
        for i, k in enumerate(("params", "exp_avg", "exp_avg_sq")):
            err, E = UR.error_floor(host[s][k], r64[s][i], r32[s][i])
            worst = max(worst, UR.ratio_of(err, E))
            assert err <= C_ADAM * E, ("step %d" % (s + 1), k, "error %.3g above %d E = %.3g" % (err, C_ADAM, C_ADAM * E))
        assert abs(float(host[s]["total"]) - r64[s][3]) <= 2.0 ** -22 * r64[s][3], ("step %d" % (s + 1), "grad_norm")
        assert abs(float(host[s]["total"]) - norms[s]) <= 2.0 ** -22 * norms[s]
        assert host[s]["step"] == s + 1
        assert host[s]["beta_pow"][0] == pytest.approx(0.9 ** (s + 1), rel=1e-15)
        assert host[s]["beta_pow"][1] == pytest.approx(0.999 ** (s + 1), rel=1e-15)
    print("ppo adam rule: largest error / E %.2f" % worst)
    # exact zeros of the first gradient move nothing on the first step
    assert np.array_equal(host[0]["params"][zeros], p0[zeros])
    assert (host[0]["exp_avg"][zeros] == 0).all() and (host[0]["exp_avg_sq"][zeros] == 0).all()
    # below max_grad_norm the coefficient is exactly 1: the second step from the first step's state, gradient unscaled
    m1, v1 = host[0]["exp_avg"].astype(np.float32), host[0]["exp_avg_sq"].astype(np.float32)
    g = grads[1]
    omb1, b2, omb2 = np.float32(1.0 - 0.9), np.float32(0.999), np.float32(1.0 - 0.999)
    assert np.array_equal(host[1]["exp_avg"], m1 + (g - m1) * omb1)
    assert np.array_equal(host[1]["exp_avg_sq"], v1 * b2 + omb2 * (g * g))
    # the state carries over: steps two and three from the first step's state give the same bits
    again = UR.run_adam_host(host[0]["params"], host[0]["exp_avg"], host[0]["exp_avg_sq"], grads[1:], step=1,
                             beta_pow=host[0]["beta_pow"], **UR.ADAM)
    for s in (0, 1):
        for k in ("params", "exp_avg", "exp_avg_sq", "beta_pow"):
            assert np.array_equal(again[s][k], host[s + 1][k])
        assert again[s]["step"] == s + 2 and again[s]["total"] == host[s + 1]["total"]
