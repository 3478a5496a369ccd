"""CPU suite of the device policy backward: the C interface and its argument checks, the host-side refusals of
`TrainablePolicy`, the head gradient rule's header run on the host, the float64 reference against plain autograd, and
`nbytes`.  The kernels themselves are tested in test_gpu_policy_grad.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import policy_cases as PC
from tests import policy_grad_reference as GR
from tests.conftest import ROOT


def _sd(ew=6, na=7):
    return PC.state_dict(1, ew, na)


# ---- the C interface

def test_the_header_declares_the_entry_points_and_null_is_refused():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "int gd_policy_evaluate(const gd_policy *p, const gd_policy_grad *g, " in header
    assert "int gd_policy_backward(const gd_policy *p, const gd_policy_grad *g, " in header
    assert "typedef struct gd_policy_grad {" in header and "csrc/policy_grad_rule.hpp" in header
    assert "gpudrive/integrations/puffer/ppo.py:261-332" in header and "clamped" in header
    assert "gd_policy_evaluate" in _capi.SYMBOLS and "gd_policy_backward" in _capi.SYMBOLS
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert {"gd_policy_evaluate", "gd_policy_backward"} <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_policy_evaluate.argtypes) == 8 and len(L.gd_policy_backward.argtypes) == 9
    assert C.sizeof(_capi.GdPolicyGrad) == 6 * 8 + 8 + 4 + 4 and C.sizeof(_capi.GdPolicy) == 16 + 4 * 8
    assert L.gd_policy_evaluate(None, None, None, None, None, None, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_policy_evaluate" in L.gd_last_error()
    assert L.gd_policy_backward(None, None, None, None, None, None, None, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_policy_backward" in L.gd_last_error()


def test_the_entry_points_check_their_arguments_without_a_device():
    """Nothing is launched: every call below stops at a check."""
    from gpudrive_lab_amd.policy import grad_floats, pack_index
    L = _capi.lib()
    ok = 0x1000

    def structs(**kw):
        p, g = _capi.GdPolicy(), _capi.GdPolicyGrad()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = 3, 64, 6, 7
        p.blob, p.blob_floats = ok, len(pack_index(6, 7))
        g.features = g.logits = g.winners = g.params = g.rowstat = g.partials = ok
        g.grad_floats, g.num_partials = grad_floats(6, 7), 4
        for k, v in kw.items():
            setattr(g if hasattr(g, k) else p, k, v)  # (features and logits: those of gd_policy_grad)
        return C.byref(p), C.byref(g)

    def evaluate(args=(ok,) * 5, **kw):
        rc = L.gd_policy_evaluate(*structs(**kw), *args, None)
        return rc, L.gd_last_error()

    def backward(args=(ok,) * 6, **kw):
        rc = L.gd_policy_backward(*structs(**kw), *args, None)
        return rc, L.gd_last_error()

    # with everything in order but a misaligned `actions`, both get as far as the alignment check
    for call, args in ((evaluate, (ok, ok + 4, ok, ok, ok)), (backward, (ok, ok + 4, ok, ok, ok, ok))):
        rc, msg = call(args)
        assert rc == _capi.GD_ERR_INVALID and b"8-byte aligned" in msg, msg
        for kw, word in ((dict(max_agents=100), b"max_agents"), (dict(ego_width=7), b"ego_width"), (dict(n_actions=0), b"n_actions"),
                         (dict(n_actions=1025), b"n_actions"), (dict(num_rows=0), b"num_rows"), (dict(features=None), b"features"),
                         (dict(logits=None), b"logits"), (dict(winners=None), b"winners"), (dict(features=ok + 4), b"16-byte")):
            rc, msg = call(args, **kw)
            assert rc == _capi.GD_ERR_INVALID and word in msg and b"gd_policy_" in msg, (kw, msg)
    for i in range(5):
        rc, msg = evaluate(tuple(None if j == i else ok for j in range(5)))
        assert rc == _capi.GD_ERR_INVALID and b"gd_policy_evaluate: null" in msg
    for i in range(6):
        rc, msg = backward(tuple(None if j == i else ok for j in range(6)))
        assert rc == _capi.GD_ERR_INVALID and b"gd_policy_backward: null" in msg
    for kw, word in ((dict(blob=None), b"blob"), (dict(blob_floats=5), b"blob_floats"), (dict(blob=ok + 4), b"16-byte")):
        rc, msg = evaluate(**kw)
        assert rc == _capi.GD_ERR_INVALID and word in msg, (kw, msg)
    for kw, word in ((dict(params=None), b"params"), (dict(rowstat=None), b"rowstat"), (dict(partials=None), b"partials"),
                     (dict(num_partials=0), b"num_partials"), (dict(num_partials=1025), b"num_partials"),
                     (dict(grad_floats=grad_floats(6, 7) + 1), b"grad_floats"), (dict(partials=ok + 2), b"aligned")):
        rc, msg = backward(**kw)
        assert rc == _capi.GD_ERR_INVALID and word in msg and b"gd_policy_backward" in msg, (kw, msg)


def test_the_library_counts_the_parameters_as_the_state_dict_does():
    from gpudrive_lab_amd.policy import expected_shapes, grad_floats
    L = _capi.lib()
    for ew, na in ((6, 91), (9, 7), (6, 1), (9, 1024), (9, 8), (6, 31), (9, 32), (6, 33)):
        assert grad_floats(ew, na) == sum(v.numel() for v in PC.state_dict(2, ew, na).values())
        assert list(expected_shapes(ew, na)) == list(PC.state_dict(2, ew, na))
        p, g = _capi.GdPolicy(), _capi.GdPolicyGrad()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = 3, 64, ew, na
        g.features = g.logits = g.winners = g.params = g.rowstat = g.partials = 0x1000
        g.grad_floats, g.num_partials = grad_floats(ew, na), 1
        args = (0x1000, 0x1004, 0x1000, 0x1000, 0x1000, 0x1000, None)
        assert L.gd_policy_backward(C.byref(p), C.byref(g), *args) == _capi.GD_ERR_INVALID and b"8-byte aligned" in L.gd_last_error()
        g.grad_floats -= 1
        assert L.gd_policy_backward(C.byref(p), C.byref(g), *args) == _capi.GD_ERR_INVALID and b"grad_floats" in L.gd_last_error()


# ---- the module's host side

def test_the_constructor_and_forward_refuse_on_the_host(monkeypatch):
    from gpudrive_lab_amd.policy import TrainablePolicy
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library is not needed for a refusal"))
    sd = _sd()
    for kw in (dict(dropout=0.01), dict(dropout=True), dict(dropout=None), dict(partials=0), dict(partials=1025), dict(partials=2.0),
               dict(max_agents=100), dict(ego_width=7), dict(act_func="gelu"), dict(vbd_in_obs=True), dict(device="no such device")):
        with pytest.raises(ValueError):
            TrainablePolicy.from_state_dict(sd, **dict(dict(max_agents=64, ego_width=6), **kw))
    for bad in ({k: v for k, v in sd.items() if k != "critic.bias"}, dict(sd, extra=torch.zeros(1)),
                dict(sd, **{"actor.bias": sd["actor.bias"].double()}), dict(sd, **{"ego_embed.0.weight": torch.zeros(64, 9)}),
                dict(sd, **{"actor.weight": torch.zeros(1025, 128), "actor.bias": torch.zeros(1025)})):
        with pytest.raises(ValueError):
            TrainablePolicy.from_state_dict(bad, max_agents=64, ego_width=6)
    tp = TrainablePolicy.from_state_dict(sd, max_agents=64, ego_width=6)
    assert tp.partials == 256 and tp.n_actions == 7
    w = tp.obs_width
    obs, act = torch.zeros(3, w), torch.zeros(3, dtype=torch.int64)
    for o, a in ((obs[:, :-1], act), (obs.double(), act), (obs.requires_grad_(False).clone().requires_grad_(True), act), (obs, None),
                 (obs, act[:2]), (obs, act.int()), (obs, act), (torch.zeros(0, w), act[:0]), (obs.numpy(), act)):
        with pytest.raises(ValueError):  # (the last but two: a host tensor -- there is no host path)
            tp(o, a)


def test_the_module_has_the_reference_modules_state_dict():
    from gpudrive_lab_amd.policy import TrainablePolicy
    sd = _sd(9, 91)
    tp = TrainablePolicy.from_state_dict(sd, max_agents=128, ego_width=9)
    got = tp.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert [k for k, _ in tp.named_parameters()] == list(sd) and all(p.requires_grad for p in tp.parameters())
    net = PC.StandIn(128, 9, 91)
    net.load_state_dict(got)                      # strict: the names and shapes are the stand-in's
    other = PC.state_dict(2, 9, 91)
    net.load_state_dict(other)
    tp.load_state_dict(net.state_dict())
    assert all(torch.equal(tp.state_dict()[k], other[k]) for k in other)
    assert tp.train() is tp and tp.eval() is tp
    sd["actor.bias"][0] = 5.0                     # the module owns copies
    assert tp.state_dict()["actor.bias"][0] != 5.0


def test_nbytes_is_its_formula():
    from gpudrive_lab_amd.policy import TrainablePolicy, grad_floats, pack_index
    for ew, na, P in ((6, 91, None), (9, 7, 3)):
        tp = TrainablePolicy.from_state_dict(_sd(ew, na), max_agents=64, ego_width=ew, partials=P)
        G, P = grad_floats(ew, na), P or 256
        per_row = tp.nbytes(2) - tp.nbytes(1)
        assert per_row == 4 * (192 + na + 3 + 3 + 8) + 128 and per_row <= 4 * (192 + 128 + na) + 128
        assert tp.nbytes(1000) - tp.nbytes(1) == 999 * per_row
        assert tp.nbytes(0) == 4 * ((G + 1) + len(pack_index(ew, na)) + (P + 2) * G) + 512 * 64


# ---- the head gradient rule

def _rule_cases():
    rng = np.random.default_rng(6)
    for na in (91, 7, 1, 1024) + tuple(k for k in PC.EDGE_ACTIONS if k not in (1, 1024)):
        logits = rng.normal(0.0, 2.0, (40, na)).astype(np.float32)
        logits[0] = 0.0
        yield "seeded", na, logits
    logits = rng.normal(0.0, 2.0, (40, 91)).astype(np.float32)
    logits[:, 3] += 120.0   # case (v): every other expf underflows
    yield "lifted", 91, logits


@pytest.mark.parametrize("name,na,logits", list(_rule_cases()), ids=lambda v: str(v) if isinstance(v, (int, str)) else "")
def test_rule_header_on_the_host_equals_the_float64_rule(name, na, logits):
    rng = np.random.default_rng(na)
    n = len(logits)
    actions = rng.integers(0, na, n)
    actions[::3] = logits[::3].argmax(-1)
    for dlp, dent in ((rng.normal(0, 1, n), rng.normal(0, 1, n)), (rng.normal(0, 1, n), np.zeros(n)), (np.zeros(n), rng.normal(0, 1, n))):
        dlp, dent = dlp.astype(np.float32), dent.astype(np.float32)
        got = GR.run_rule_host(logits, actions, dlp, dent)
        want = GR.rule64(logits, actions, dlp, dent)
        assert np.isfinite(got).all()
        assert (np.abs(got - want) <= (na + 8) * 2.0 ** -24 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()
    zero = GR.run_rule_host(logits, actions, np.zeros(n), np.zeros(n))
    assert (zero == 0.0).all()
    # the rule against autograd of the formulas it differentiates
    l = torch.tensor(logits.astype(np.float64), requires_grad=True)
    q = torch.log_softmax(l, -1)
    (torch.tensor(dlp.astype(np.float64)) * q.gather(1, torch.tensor(actions)[:, None])[:, 0]
     + torch.tensor(dent.astype(np.float64)) * -(q.exp() * q).sum(-1)).sum().backward()
    assert np.abs(l.grad.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_rule_host_program_under_the_sanitizers_at_the_edge_action_counts():
    """The same program as a stand-alone executable built with -fsanitize=address,undefined: it must exit cleanly and give the
    plain build's bits; at one action every dlogit is zero."""
    rng = np.random.default_rng(8)
    for na in PC.EDGE_ACTIONS:
        n = 5
        logits = rng.normal(0.0, 2.0, (n, na)).astype(np.float32)
        actions = rng.integers(0, na, n)
        dlp, dent = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
        plain = GR.run_rule_host(logits, actions, dlp, dent)
        san = GR.run_rule_host(logits, actions, dlp, dent, sanitize=True)
        assert np.array_equal(plain.view(np.int32), san.view(np.int32)), na
        if na == 1:
            assert (plain == 0.0).all()


# ---- the reference

@pytest.mark.parametrize("max_agents,ego_width,n_actions", [(64, 6, 91), (128, 9, 7)])
def test_gather_at_the_argmax_equals_plain_max_autograd(max_agents, ego_width, n_actions):
    n = 3
    sd = _sd(ego_width, n_actions)
    obs = PC.observations(4, n, max_agents, ego_width)
    rng = np.random.default_rng(3)
    actions = rng.integers(0, n_actions, n)
    ups = [rng.normal(0, 1, n) for _ in range(3)]
    net = GR.stand_in(sd, max_agents, ego_width, torch.float64)
    lp, ent, val, pe, re = GR.evaluate(net, obs, actions)
    (torch.tensor(ups[0]) * lp + torch.tensor(ups[1]) * ent + torch.tensor(ups[2]) * val).sum().backward()
    plain = {k: p.grad.numpy() for k, p in net.named_parameters()}
    winners = np.concatenate([pe.argmax(1).numpy(), re.argmax(1).numpy()], 1)
    at = GR.gradients(sd, obs, max_agents, ego_width, actions, ups, winners, torch.float64)
    assert list(at) == list(sd)
    for k in plain:
        assert np.array_equal(at[k], plain[k]), k
    # and the forward is the forward reference's
    from tests import policy_reference as REF
    l64, v64, _ = REF.forward(sd, obs, max_agents, ego_width)
    _, wlp, went = REF.action_rule(l64, deterministic=True)
    lp2, ent2, val2, _, _ = GR.evaluate(net, obs, l64.argmax(-1))
    assert np.abs(lp2.detach().numpy() - wlp).max() < 1e-12 and np.abs(ent2.detach().numpy() - went).max() < 1e-12
    assert np.abs(val2.detach().numpy() - v64).max() < 1e-12


def test_the_yardstick_is_not_degenerate():
    """E_p / max |g_p| of the float32 computation lies between 5e-8 and 6e-7 for every tensor on four of the seeded shapes
    (over all 24, with these seeds, it runs from the floor 2^-23 = 1.2e-7 to 9.4e-7: the sums over 70 rows are the longer)."""
    for n, a, ew, na in ((1, 64, 6, 91), (3, 64, 6, 7), (3, 128, 9, 7), (70, 64, 6, 7)):
        sd = PC.state_dict(10 + na + ew, ew, na)
        obs = PC.observations(20 + n + a, n, a, ew)
        net = GR.stand_in(sd, a, ew, torch.float64)
        actions = np.random.default_rng(n).integers(0, na, n)
        lp, ent, val, pe, re = GR.evaluate(net, obs, actions)
        winners = np.concatenate([pe.argmax(1).numpy(), re.argmax(1).numpy()], 1)
        ups = GR.ppo_upstream(n + a, lp.detach().numpy(), ent.detach().numpy(), val.detach().numpy())
        g64 = GR.gradients(sd, obs, a, ew, actions, ups, winners, torch.float64)
        g32 = GR.gradients(sd, obs, a, ew, actions, ups, winners, torch.float32)
        for k, e in GR.yardstick(g64, g32).items():
            rel = e / np.abs(g64[k]).max()
            assert 5e-8 <= rel <= 6e-7, (n, a, ew, na, k, rel)


def test_the_constructed_cases_are_what_they_claim():
    from tests import policy_reference as REF
    a, ew, na, n = 64, 6, 7, 3
    sd, obs = _sd(ew, na), PC.observations(4, n, a, ew)
    p0, r0 = ew, ew + 6 * (a - 1)
    pad = GR.all_padding_partners(obs, a, ew)
    assert (pad[:, p0:r0] == 0).all() and np.array_equal(pad[:, r0:], obs[:, r0:]) and np.array_equal(pad[:, :p0], obs[:, :p0])
    cp, low = GR.copied_winner(sd, obs, a, ew)
    for i in range(n):
        for s, (name, rows) in enumerate((("partner_embed", cp[i, p0:r0].reshape(a - 1, 6)), ("road_map_embed", cp[i, r0:].reshape(200, 13)))):
            emb = REF._embed(sd, name, rows.astype(np.float64))[:, 0]
            assert emb.argmax() == low[i, s] < len(rows) - 1 and np.array_equal(rows[-1], rows[low[i, s]])
            first = GR.first_identical_row(rows)
            assert first[-1] == first[low[i, s]] <= low[i, s]
    lifted = GR.lifted_actor_bias(sd)
    l64, _, _ = REF.forward(lifted, obs, a, ew)
    assert (np.exp((l64 - l64.max(-1, keepdims=True)).astype(np.float32))[:, np.arange(na) != 3] == 0).all()
    lp, ent, val = np.zeros(8), np.ones(8), np.zeros(8)
    ups = GR.ppo_upstream(1, lp, ent, val)
    assert (ups[0] == 0).any() and (ups[0] != 0).any(), "some rows clip and some do not"
    assert np.allclose(ups[1], -0.01 / 8) and all(len(u) == 1 for u in GR.ppo_upstream(1, lp[:1], ent[:1], val[:1]))
