"""GPU suite: training-mode dropout of the device policy (gpudrive_lab_amd.dropout.DropoutRule; gd_policy_forward_dropout,
gd_policy_evaluate_dropout, gd_policy_backward_dropout) against the host program of csrc/dropout_rule.hpp and the masked
float64 stand-in (tests/dropout_reference.py).

1. The masks made visible by constructed weights, bit for bit against the host program, at all four sites.
2. Forward and evaluate against the masked float64 stand-in fed the host program's masks.  The yardstick E is the same masked
   computation in torch float32 on the CPU against float64, floored at 2^-23 max |.|; the bound stays the unmasked forward's
   8 E: the mask adds one multiply by `scale` to the kernel and to the yardstick alike (a dropped element is exact in both).
3. Consistency: seek, equal (seed, call), the counter, d = NULL and dropout_rule=None, eval().
4. Backward against float64 autograd of the masked stand-in, gathered at the kernel's own winners, by the yardstick E_p of
   test_gpu_policy_grad.py.  The bound is set as there: the next power of two at or above twice the largest ratio measured
   over all cases (5.97, actor.bias, last_entity_wins, n = 3, p = 0.5), which is 16 -- below the unmasked backward's 32.
The largest ratios measured are tabulated in DESIGN.md section 5 (forward: 2.08, so the bound stays 8)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import dropout_reference as DREF
from tests import policy_cases as PC
from tests import policy_grad_reference as GR
from tests.test_gpu_policy import Carver, _no_sync
from tests.test_gpu_policy_grad import Raw

pytestmark = pytest.mark.gpu

A = 64
FWD_BOUND = 8    # the largest ratio measured over all cases is 2.08 (n = 3, (6, 7), p = 0.01)
BWD_BOUND = 16   # the largest ratio measured over all cases is 5.97; see the module docstring
SHAPES = [(n, ew, na) for n in (1, 3, 70) for ew, na in ((6, 7), (9, 91))]


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.uint8 if a.dtype.itemsize == 1 else np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rule(p, seed=42):
    from gpudrive_lab_amd.dropout import DropoutRule
    return DropoutRule(p, seed)


class RawDrop(Raw):
    """`Raw` of test_gpu_policy_grad.py on the *_dropout entry points: canary guards around every buffer, `used` included."""

    def __init__(self, n, a, ew, na, partials, rule):
        super().__init__(n, a, ew, na, partials)
        self.rule = rule
        self.used = self.fwd.carve("used", (1,), torch.int64)

    def evaluate(self, obs, actions, what, drop=True):
        self.fwd.refill()
        self.obs, self.actions = obs, actions
        p, g = self._structs()
        d = self.rule.struct(self.used)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _no_sync(lambda: _capi.check(self.L.gd_policy_evaluate_dropout(C.byref(p), C.byref(g), C.byref(d) if drop else None,
                                                                       obs.data_ptr(), actions.data_ptr(),
                                                                       *(o.data_ptr() for o in self.out), stream)))
        if drop:
            self.fwd.assert_guards_and_written(what + " evaluate")
        return [o.cpu().numpy().copy() for o in self.out] + [self.logits.cpu().numpy().copy(), self.winners.cpu().numpy().copy()]

    def backward(self, ups, what, drop=True):
        self.bwd.refill()
        dd = [torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda() for u in ups]
        p, g = self._structs()
        d = self.rule.struct(self.used)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _no_sync(lambda: _capi.check(self.L.gd_policy_backward_dropout(C.byref(p), C.byref(g), C.byref(d) if drop else None,
                                                                       self.obs.data_ptr(), self.actions.data_ptr(),
                                                                       *(t.data_ptr() for t in dd), self.grad.data_ptr(), stream)))
        self.bwd.assert_guards_and_written(what + " backward")
        flat, out, o = self.grad.cpu().numpy().copy(), {}, 0
        for k, shape in self.shapes.items():
            size = int(np.prod(shape))
            out[k] = flat[o:o + size].reshape(shape)
            o += size
        return out


# ---- 1. the masks made visible

def test_the_shared_mask_is_the_host_programs_bit_for_bit():
    from gpudrive_lab_amd.policy import DevicePolicy
    n, ew, na = 70, 6, 128
    sd = PC.state_dict(1, ew, na)
    sd["shared_embed.0.weight"].zero_(), sd["shared_embed.0.bias"].fill_(1.0)
    sd["actor.weight"].copy_(torch.eye(128)), sd["actor.bias"].zero_()
    rule = _rule(0.5)
    pol = DevicePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, dropout_rule=rule)
    obs = torch.from_numpy(PC.observations(2, n, A, ew)).cuda()
    logits = torch.empty((n, na), device="cuda")
    rule.seek(9)
    pol(obs, deterministic=True, logits_out=logits)
    keep = DREF.host_mask(rule.seed, 9, rule.threshold, 3, n, 1, 128)[:, 0]
    want = np.where(keep, np.float32(rule.scale), np.float32(0.0)).astype(np.float32)
    assert rule.scale == 2.0 and 0.4 < keep.mean() < 0.6
    assert _same(logits, want), "logits are {0, scale} in the host program's pattern"


@pytest.mark.parametrize("ew", [6, 9])
def test_the_ego_and_set_masks_are_the_host_programs(ew):
    n, na = 3, 7
    sd = PC.state_dict(1, ew, na)
    for name in PC.EMBEDDERS:
        sd[name + ".4.weight"].copy_(torch.eye(64)), sd[name + ".4.bias"].zero_()
    obs = torch.from_numpy(PC.observations(2, n, A, ew)).cuda()
    actions = torch.zeros(n, dtype=torch.int64, device="cuda")
    rule = _rule(0.5, seed=3)
    raw = RawDrop(n, A, ew, na, 1, rule)
    for sign in (1.0, -1.0):
        for name in PC.EMBEDDERS[1:]:
            sd[name + ".1.weight"].zero_(), sd[name + ".1.bias"].fill_(sign)
        raw.load(sd)
        rule.seek(4)
        _, _, _, _, winners = raw.evaluate(obs, actions, "constructed %+g" % sign)
        keep = DREF.host_masks(rule.seed, 4, rule.threshold, n, A)
        feats = raw.features.cpu().numpy()
        # ego: second layer = identity, so the saved ego features are the masked tanh outputs
        assert ((feats[:, :64] == 0) == ~keep["ego"]).all() and (np.signbit(feats[:, :64][~keep["ego"]]) == 0).all()
        for s, site in enumerate(("partner", "road")):
            k = keep[site]                                         # [n, entities, 64]
            w = winners[:, 64 * s:64 * s + 64].astype(np.int64)
            target = k if sign > 0 else ~k                         # +1: the first kept entity wins; -1: the first dropped one (0 > tanh(-1) scale)
            assert target.any(1).all()
            assert np.array_equal(w, target.argmax(1)), (site, sign)
            pooled = feats[:, 64 + 64 * s:128 + 64 * s]
            want = np.float32(np.tanh(np.float32(1.0))) * np.float32(rule.scale) if sign > 0 else np.float32(0.0)
            assert np.abs(pooled - want).max() <= 2.0 ** -20, (site, sign)   # (OCML's tanhf against libm's)


# ---- 2. forward and evaluate against the masked float64 stand-in

@pytest.mark.parametrize("p", [0.01, 0.5])
@pytest.mark.parametrize("n,ew,na", SHAPES, ids=lambda v: str(v))
def test_forward_and_evaluate_against_the_masked_float64_stand_in(n, ew, na, p):
    _forward_case(n, ew, na, p)


def _forward_case(n, ew, na, p):
    from gpudrive_lab_amd.policy import DevicePolicy
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs_h = PC.observations(20 + n + A, n, A, ew)
    obs = torch.from_numpy(obs_h).cuda()
    rule = _rule(p, seed=1234567890123)
    pol = DevicePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, dropout_rule=rule)
    raw = RawDrop(n, A, ew, na, 7, rule)
    raw.load(sd)
    carver = Carver()
    out = (carver.carve("actions", (n,), torch.int64),) + tuple(carver.carve(k, (n,), torch.float32) for k in ("logprob", "entropy", "value"))
    logits = carver.carve("logits", (n, na), torch.float32)
    call = 2 ** 32 + 5   # (the high word of the counter too)
    what = "n=%d ego=%d actions=%d p=%g" % (n, ew, na, p)
    rule.seek(call)
    pol(obs, torch.from_numpy(PC.uniforms(n, n)).cuda(), out=out, logits_out=logits)
    carver.assert_guards_and_written(what)
    keep = DREF.host_masks(rule.seed, call, rule.threshold, n, A)
    l64, v64, E = DREF.forward_yardstick(sd, obs_h, A, ew, keep, rule.scale)
    err = max(np.abs(logits.cpu().numpy() - l64).max(), np.abs(out[3].cpu().numpy() - v64).max())
    print("policy dropout forward %s: E %.3g, kernel error %.3g, ratio %.2f" % (what, E, err, err / E))
    assert err <= FWD_BOUND * E, (what, "error %.3g above %d E = %.3g" % (err, FWD_BOUND, FWD_BOUND * E))
    # the masks matter: the unmasked reference is far away
    if p == 0.5:
        u_l, _ = PC.stand_in_forward(sd, obs_h, A, ew, torch.float64)
        assert np.abs(u_l - l64).max() > 100 * FWD_BOUND * E
    # evaluate at the same index: the same logits, logprob, entropy and value, bit for bit, and winners on the masked outputs
    rule.seek(call)
    lp, ent, val, e_logits, winners = raw.evaluate(obs, out[0], what)
    assert _same(e_logits, logits) and _same(lp, out[1]) and _same(ent, out[2]) and _same(val, out[3])
    assert int(raw.used.item()) == call and rule.call == call + 1
    net = DREF.masked_stand_in(sd, A, ew, torch.float64, keep, rule.scale)
    with torch.no_grad():
        _, _, _, pe, re = GR.evaluate(net, obs_h, out[0].cpu().numpy())
    for s, emb in enumerate((pe.numpy(), re.numpy())):
        w = winners[:, 64 * s:64 * s + 64].astype(np.int64)
        assert (w < emb.shape[1]).all()
        at = np.take_along_axis(emb, w[:, None, :], 1)[:, 0]
        assert (at >= emb.max(1) - FWD_BOUND * E).all(), (what, "a winner below the masked maximum")


# ---- 3. consistency

def test_the_counter_the_null_struct_and_eval_mode():
    from gpudrive_lab_amd.policy import DevicePolicy, TrainablePolicy
    n, ew, na = 70, 9, 91
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs = torch.from_numpy(PC.observations(5, n, A, ew)).cuda()
    u = torch.from_numpy(PC.uniforms(6, n)).cuda()
    rule = _rule(0.5, seed=2 ** 63 + 11)
    pol = DevicePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, dropout_rule=rule)
    plain = DevicePolicy.from_state_dict(sd, max_agents=A, ego_width=ew)
    assert pol.training and rule.call == 0 and rule.nbytes == 16

    def run(policy, **kw):
        logits = torch.empty((n, na), device="cuda")
        return [t.clone() for t in policy(obs, u, logits_out=logits, **kw)] + [logits]

    first = run(pol)
    assert rule.call == 1
    second = run(pol)
    assert rule.call == 2 and not _same(first[4], second[4]), "the next call draws other masks"
    rule.seek(0)
    again = _no_sync(lambda: run(pol))
    assert all(_same(a, b) for a, b in zip(first, again)), "equal (seed, call) gives equal bits"
    other = DevicePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, dropout_rule=_rule(0.5, seed=2 ** 63 + 12))
    assert not _same(run(other)[4], first[4]), "another seed draws other masks"
    rule.seek(0)
    det = run(pol, deterministic=True)
    assert _same(det[4], first[4]) and rule.call == 1, "deterministic=True does not switch the masks off"
    # eval(): the unmasked path, and the counter stands still
    base = run(plain)
    assert pol.eval() is pol and all(_same(a, b) for a, b in zip(run(pol), base)) and rule.call == 1
    assert pol.train() is pol and not _same(run(pol)[4], base[4]) and rule.call == 2
    # d = NULL on the new entry points is the existing function
    raw = RawDrop(n, A, ew, na, 7, rule)
    raw.load(sd)
    old = Raw(n, A, ew, na, 7)
    old.load(sd)
    ups = [np.random.default_rng(k).normal(0, 1.0 / n, n).astype(np.float32) for k in range(3)]
    got = raw.evaluate(obs, first[0], "d = NULL", drop=False)
    want = old.evaluate(obs, first[0], "existing")
    assert all(_same(a, b) for a, b in zip(got, want)) and _same(got[3], base[4]) and rule.call == 2
    g_new, g_old = raw.backward(ups, "d = NULL", drop=False), old.backward(ups, "existing")
    assert all(_same(g_new[k], g_old[k]) for k in g_old)
    L = _capi.lib()
    p = _capi.GdPolicy()
    p.num_rows, p.max_agents, p.ego_width, p.n_actions = n, A, ew, na
    p.blob, p.blob_floats, p.features, p.logits = plain.blob.data_ptr(), plain.blob.numel(), raw.features.data_ptr(), raw.logits.data_ptr()
    outs = [torch.empty(n, dtype=torch.int64, device="cuda")] + [torch.empty(n, device="cuda") for _ in range(3)]
    _capi.check(L.gd_policy_forward_dropout(C.byref(p), None, obs.data_ptr(), u.data_ptr(), 0, *(t.data_ptr() for t in outs), None,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert all(_same(a, b) for a, b in zip(outs, base[:4]))
    # the module: eval() with a rule, and no rule, are the unmasked path bit for bit
    tp = TrainablePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, device="cuda", dropout_rule=rule, partials=7)
    tp0 = TrainablePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, device="cuda", partials=7)
    t_ups = [torch.from_numpy(x).cuda() for x in ups]

    def grads(mod):
        mod.zero_grad(set_to_none=True)
        _, lp, ent, val = mod(obs, first[0])
        torch.autograd.backward([lp, ent, val], t_ups)
        return [lp.detach(), ent.detach(), val.detach()] + [q.grad.clone() for q in mod.parameters()]

    want = grads(tp0)
    tp.eval()
    assert all(_same(a, b) for a, b in zip(grads(tp), want)) and rule.call == 2
    tp.train()
    masked = grads(tp)
    assert rule.call == 3 and not _same(masked[0], want[0])
    # the module in train mode is the raw calls at the same index
    rule.seek(2)
    lp, ent, val, _, _ = raw.evaluate(obs, first[0], "raw")
    g_raw = raw.backward(ups, "raw")
    assert _same(lp, masked[0]) and _same(ent, masked[1]) and _same(val, masked[2])
    assert all(_same(g_raw[k], g) for k, g in zip(raw.shapes, masked[3:]))


def test_two_forwards_then_the_first_ones_backward_use_the_first_ones_masks():
    from gpudrive_lab_amd.policy import TrainablePolicy
    n, ew, na = 3, 6, 7
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs = torch.from_numpy(PC.observations(5, n, A, ew)).cuda()
    actions = torch.from_numpy(np.random.default_rng(1).integers(0, na, n)).cuda()
    ups = [torch.randn(n, device="cuda") for _ in range(3)]
    rule = _rule(0.5, seed=77)
    tp = TrainablePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, device="cuda", dropout_rule=rule, partials=7)
    rule.seek(10)
    _, lp, ent, val = tp(obs, actions)
    torch.autograd.backward([lp, ent, val], ups)
    alone = [q.grad.clone() for q in tp.parameters()]
    tp.zero_grad(set_to_none=True)
    rule.seek(10)
    _, lp, ent, val = tp(obs, actions)
    _, lp2, ent2, val2 = tp(obs, actions)      # index 11, between the first forward and its backward
    assert not _same(lp, lp2) and rule.call == 12
    _no_sync(lambda: torch.autograd.backward([lp, ent, val], ups))
    assert all(_same(q.grad, g) for q, g in zip(tp.parameters(), alone))
    tp.zero_grad(set_to_none=True)
    torch.autograd.backward([lp2, ent2, val2], ups)
    assert not all(_same(q.grad, g) for q, g in zip(tp.parameters(), alone))


# ---- 4. backward

def _compare(what, sd, obs, ew, actions, ups, winners, got, keep, scale):
    g64 = DREF.gradients(sd, obs, A, ew, actions, ups, winners, torch.float64, keep, scale)
    g32 = DREF.gradients(sd, obs, A, ew, actions, ups, winners, torch.float32, keep, scale)
    E = GR.yardstick(g64, g32)
    worst, at = 0.0, None
    for k in g64:
        assert np.isfinite(got[k]).all(), (what, k)
        err = float(np.abs(got[k] - g64[k]).max())
        ratio = err / E[k] if E[k] > 0 else (0.0 if err == 0 else np.inf)
        if ratio >= worst:
            worst, at = ratio, k
    print("policy dropout backward %s: largest error / E_p %.2f at %s" % (what, worst, at))
    for k in g64:
        err = float(np.abs(got[k] - g64[k]).max())
        assert err <= BWD_BOUND * E[k], (what, k, "error %.3g above %d E_p = %.3g" % (err, BWD_BOUND, BWD_BOUND * E[k]))
    return g64


@pytest.mark.parametrize("p", [0.01, 0.5])
@pytest.mark.parametrize("n,ew,na", SHAPES, ids=lambda v: str(v))
def test_backward_against_float64_autograd_of_the_masked_stand_in(n, ew, na, p):
    _backward_case(n, ew, na, p)


# the action counts where the tiling of the heads changes (tests/policy_cases.py EDGE_SHAPES): the value alone in a second tile,
# 33 tiles, and a softmax of one number (its actor gradients are exactly zero in float64, E_p is zero and so is the bound)
EDGE = [(33, 9, 32), (3, 6, 1024), (33, 6, 1)]


@pytest.mark.parametrize("n,ew,na", EDGE, ids=lambda v: str(v))
def test_forward_evaluate_and_backward_at_the_action_counts_where_the_tiling_changes(n, ew, na):
    assert na in PC.EDGE_ACTIONS
    _forward_case(n, ew, na, 0.5)
    _backward_case(n, ew, na, 0.5)


def _backward_case(n, ew, na, p):
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs0 = PC.observations(20 + n + A, n, A, ew)
    rule = _rule(p, seed=99)
    raw = RawDrop(n, A, ew, na, 7, rule)
    raw.load(sd)
    cases = (("seeded", obs0), ("last_entity_wins", PC.last_entity_wins(sd, obs0, A, ew)),
             ("all_padding_partners", GR.all_padding_partners(obs0, A, ew)))
    for ci, (name, obs_h) in enumerate(cases):
        what = "%s n=%d ego=%d actions=%d p=%g" % (name, n, ew, na, p)
        obs = torch.from_numpy(obs_h).cuda()
        actions_h = np.random.default_rng(n + ci).integers(0, na, n)
        actions = torch.from_numpy(actions_h).cuda()
        call = 100 + ci
        rule.seek(call)
        lp, ent, val, _, winners = raw.evaluate(obs, actions, what)
        keep = DREF.host_masks(rule.seed, call, rule.threshold, n, A)
        ups = GR.ppo_upstream(100 + n + ci, lp, ent, val)
        rule.seek(7)                                   # the backward reads `used`, not the counter
        got = raw.backward(ups, what)
        assert rule.call == 7 and int(raw.used.item()) == call
        _compare(what, sd, obs_h, ew, actions_h, ups, winners, got, keep, rule.scale)
        assert (winners[:, :64] < A - 1).all() and (winners[:, 64:] < 200).all(), what


@pytest.mark.parametrize("P", [1, 7, 256])
def test_backward_for_every_partials(P):
    n, ew, na = 70, 6, 91
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs_h = PC.observations(20 + n + A, n, A, ew)
    obs = torch.from_numpy(obs_h).cuda()
    actions_h = np.random.default_rng(1).integers(0, na, n)
    actions = torch.from_numpy(actions_h).cuda()
    rule = _rule(0.5, seed=5)
    raw = RawDrop(n, A, ew, na, P, rule)
    raw.load(sd)
    what = "partials=%d" % P
    rule.seek(3)
    lp, ent, val, _, winners = raw.evaluate(obs, actions, what)
    keep = DREF.host_masks(rule.seed, 3, rule.threshold, n, A)
    ups = GR.ppo_upstream(5, lp, ent, val)
    got = raw.backward(ups, what)
    _compare(what, sd, obs_h, ew, actions_h, ups, winners, got, keep, rule.scale)
    again = raw.backward(ups, what)
    assert all(_same(again[k], got[k]) for k in got), "two calls differ"


def test_a_dropped_winner_contributes_exactly_zero():
    n, ew, na = 1, 6, 7
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs_h = PC.observations(21, n, A, ew)
    obs = torch.from_numpy(obs_h).cuda()
    actions_h = np.array([3])
    actions = torch.from_numpy(actions_h).cuda()
    ups = [np.array([v], dtype=np.float32) for v in (0.7, -0.3, 1.1)]
    # (a) p = 0.5: row j of dW2 is dpool_j times the winner's masked tanh outputs -- exactly 0.0 where the winner's feature is dropped
    rule = _rule(0.5, seed=8)
    raw = RawDrop(n, A, ew, na, 1, rule)
    raw.load(sd)
    rule.seek(1)
    lp, ent, val, _, winners = raw.evaluate(obs, actions, "p = 0.5")
    keep = DREF.host_masks(rule.seed, 1, rule.threshold, n, A)
    got = raw.backward(ups, "p = 0.5")
    _compare("dropped winner, p = 0.5", sd, obs_h, ew, actions_h, ups, winners, got, keep, rule.scale)
    for s, (site, name) in enumerate((("partner", "partner_embed"), ("road", "road_map_embed"))):
        w = winners[0, 64 * s:64 * s + 64].astype(np.int64)
        k = keep[site][0][w]                               # [pooled feature j, first-layer feature f] at j's winner
        g = got[name + ".4.weight"]
        assert (~k).any() and (g[~k] == 0.0).all() and (g[k] != 0.0).mean() > 0.9, site
    g = got["ego_embed.4.weight"]
    assert (g[:, ~keep["ego"][0]] == 0.0).all() and (g[:, keep["ego"][0]] != 0.0).mean() > 0.9
    dropped_h = ~keep["shared"][0]
    assert (got["shared_embed.0.weight"][dropped_h] == 0.0).all() and (got["shared_embed.0.bias"][dropped_h] == 0.0).all()
    assert (got["actor.weight"][:, dropped_h] == 0.0).all() and (got["critic.weight"][:, dropped_h] == 0.0).all()
    # (b) the largest threshold, 65535, and a seed at which the host program drops EVERY element of this row: nothing passes a
    # mask, so everything below the heads' biases gets a gradient of exactly 0.0 and the logits are the actor's bias
    from gpudrive_lab_amd.dropout import DropoutRule
    rule = DropoutRule(0.99999, 0)
    assert rule.threshold == 65535
    for seed in range(64):
        keep = DREF.host_masks(seed, 0, 65535, n, A)
        if not any(k.any() for k in keep.values()):
            break
    else:
        raise AssertionError("no seed drops every element")
    rule.seed = seed
    raw = RawDrop(n, A, ew, na, 1, rule)
    raw.load(sd)
    lp, ent, val, logits, winners = raw.evaluate(obs, actions, "all dropped")
    assert _same(logits[0], sd["actor.bias"]) and _same(val, sd["critic.bias"]) and (winners == 0).all()
    got = raw.backward(ups, "all dropped")
    for k, g in got.items():
        if k in ("actor.bias", "critic.bias"):
            assert (g != 0.0).any(), k
        else:
            assert (g == 0.0).all(), (k, "a gradient passed a dropped element")
    _compare("all dropped", sd, obs_h, ew, actions_h, ups, winners, got, keep, rule.scale)
