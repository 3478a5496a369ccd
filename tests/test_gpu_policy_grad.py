"""GPU suite: the device policy backward (gpudrive_lab_amd.policy.TrainablePolicy; gd_policy_evaluate, gd_policy_backward)
against torch autograd in float64 on the CPU (tests/policy_grad_reference.py) on the seeded and constructed cases.

Forward: the logits of gd_policy_evaluate equal gd_policy_forward's bit for bit, and evaluating the actions the forward
sampled returns its logprob, entropy and value bit for bit.

Gradients: judged AT THE KERNEL'S OWN WINNERS (the reference gathers the pooled features there), so that a float32 near-tie
cannot flip a whole gradient row; the winners are judged separately.  The yardstick E_p of a parameter tensor is the maximum
absolute error of the same computation in torch float32 on the CPU against float64, floored at 2^-23 max |g64_p|
(test_policy_grad.py shows E_p / max |g_p| between 5e-8 and 6e-7); the kernel's error must be <= C E_p.  C = BOUND below is
the next power of two at or above twice the largest ratio measured over all cases (DESIGN.md section 5 tabulates them); an
indexing or masking error is >= 1e-2 relative, four orders of magnitude above.

Upstream gradients: the reference's own loss (ppo.py:282-324, clip 0.2, value clip on, norm_adv on) differentiated in float64
at the kernel's logprob, entropy and value, with old logprobs perturbed so that some rows clip and some do not; for N = 1,
where adv.std() is undefined, seeded gradients of size 1 / N."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import policy_cases as PC
from tests import policy_grad_reference as GR
from tests import policy_reference as REF
from tests.test_gpu_policy import Carver, _no_sync

pytestmark = pytest.mark.gpu

BOUND = 32  # C: the largest ratio measured over all cases is 12.7 (actor.bias, negative_pool, n = 3); see the module docstring


class Raw:
    """The two C entry points on buffers carved from canary-filled memory (guards either side, every word checked as
    written after every call)."""

    def __init__(self, n, a, ew, na, partials):
        from gpudrive_lab_amd.policy import expected_shapes, grad_floats, pack_index
        self.n, self.a, self.ew, self.na, self.P = n, a, ew, na, partials
        self.shapes = expected_shapes(ew, na)
        self.G = grad_floats(ew, na)
        self.index = torch.from_numpy(pack_index(ew, na)).cuda()
        f = torch.float32
        self.fwd, self.bwd = Carver(), Carver()
        c = self.fwd
        self.features, self.logits = c.carve("features", (n, 192), f), c.carve("logits", (n, na), f)
        self.winners = c.carve("winners", (n, 32), torch.int32).view(torch.uint8)
        self.out = [c.carve(name, (n,), f) for name in ("logprob", "entropy", "value")]
        c = self.bwd
        self.rowstat, self.partials = c.carve("rowstat", (n, 8), f), c.carve("partials", (partials, self.G), f)
        self.grad = c.carve("grad", (self.G,), f)
        self.L = _capi.lib()

    def load(self, sd):
        self.flat = torch.cat([sd[k].reshape(-1) for k in self.shapes] + [torch.zeros(1)]).cuda()
        self.blob = self.flat[self.index].contiguous()

    def _structs(self):
        p, g = _capi.GdPolicy(), _capi.GdPolicyGrad()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = self.n, self.a, self.ew, self.na
        p.blob, p.blob_floats = self.blob.data_ptr(), self.blob.numel()
        g.features, g.logits, g.winners = self.features.data_ptr(), self.logits.data_ptr(), self.winners.data_ptr()
        g.params, g.rowstat, g.partials = self.flat.data_ptr(), self.rowstat.data_ptr(), self.partials.data_ptr()
        g.grad_floats, g.num_partials = self.G, self.P
        return p, g

    def evaluate(self, obs, actions, what):
        """(logprob, entropy, value, logits, winners) on the host."""
        self.fwd.refill()
        self.obs, self.actions = obs, actions
        p, g = self._structs()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _no_sync(lambda: _capi.check(self.L.gd_policy_evaluate(C.byref(p), C.byref(g), obs.data_ptr(), actions.data_ptr(),
                                                               *(o.data_ptr() for o in self.out), stream)))
        self.fwd.assert_guards_and_written(what + " evaluate")
        return [o.cpu().numpy().copy() for o in self.out] + [self.logits.cpu().numpy().copy(), self.winners.cpu().numpy().copy()]

    def backward(self, ups, what):
        """The gradients as a dict of float32 numpy arrays under the state dict's names (views of the flat buffer)."""
        self.bwd.refill()
        d = [torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda() for u in ups]
        p, g = self._structs()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _no_sync(lambda: _capi.check(self.L.gd_policy_backward(C.byref(p), C.byref(g), self.obs.data_ptr(), self.actions.data_ptr(),
                                                               *(t.data_ptr() for t in d), self.grad.data_ptr(), stream)))
        self.bwd.assert_guards_and_written(what + " backward")
        flat, out, o = self.grad.cpu().numpy().copy(), {}, 0
        for k, shape in self.shapes.items():
            size = int(np.prod(shape))
            out[k] = flat[o:o + size].reshape(shape)
            o += size
        assert o == self.G
        return out


def _compare(what, sd, obs, a, ew, actions, ups, winners, got, ratios=None):
    """The kernel's gradients `got` against float64 at the kernel's winners, by the yardstick.  Returns the largest ratio."""
    g64 = GR.gradients(sd, obs, a, ew, actions, ups, winners, torch.float64)
    g32 = GR.gradients(sd, obs, a, ew, actions, ups, winners, torch.float32)
    E = GR.yardstick(g64, g32)
    worst, at = 0.0, None
    for k in g64:
        assert np.isfinite(got[k]).all(), (what, k, "not finite")
        err = float(np.abs(got[k] - g64[k]).max())
        ratio = err / E[k] if E[k] > 0 else (0.0 if err == 0 else np.inf)
        if ratio >= worst:
            worst, at = ratio, k
    print("policy backward %s: largest error / E_p %.2f at %s" % (what, worst, at))
    if ratios is not None:
        ratios.append(worst)
    for k in g64:
        err = float(np.abs(got[k] - g64[k]).max())
        assert err <= BOUND * E[k], (what, k, "error %.3g above %d E_p = %.3g" % (err, BOUND, BOUND * E[k]))
    return worst


def _check_winners(what, sd, obs, a, ew, winners, E_fwd):
    """Every winner attains the float64 maximum within 8 E_fwd, and no lower index holds a bit-identical input row."""
    n, a1 = obs.shape[0], a - 1
    p0, r0 = ew, ew + 6 * a1
    for s, (name, lo, hi, cnt, k) in enumerate((("partner_embed", p0, r0, a1, 6), ("road_map_embed", r0, obs.shape[1], 200, 13))):
        w = winners[:, 64 * s:64 * s + 64].astype(np.int64)
        assert (w < cnt).all(), (what, name, "a winner outside the set")
        for i in range(n):
            rows = obs[i, lo:hi].reshape(cnt, k)
            emb = REF._embed(sd, name, rows.astype(np.float64))
            assert (emb[w[i], np.arange(64)] >= emb.max(0) - 8 * E_fwd).all(), (what, name, i, "a winner below the maximum")
            first = GR.first_identical_row(rows)
            assert (first[w[i]] == w[i]).all(), (what, name, i, "a lower index holds the same row")


def _cases(sd, obs, a, ew):
    yield "seeded", sd, obs
    yield "negative_pool", PC.negative_pool_state(sd), obs               # (i)
    yield "last_entity_wins", sd, PC.last_entity_wins(sd, obs, a, ew)    # (ii)
    yield "all_padding_partners", sd, GR.all_padding_partners(obs, a, ew)  # (iii)
    yield "copied_winner", sd, GR.copied_winner(sd, obs, a, ew)          # (iv)
    if sd["actor.bias"].shape[0] > 3:  # (v) lifts action 3
        yield "lifted_actor_bias", GR.lifted_actor_bias(sd), obs


def _backward_case(n, a, ew, na, P=7):
    """Returns the largest error / E_p over the case's comparisons."""
    from gpudrive_lab_amd.policy import DevicePolicy
    sd0 = PC.state_dict(10 + na + ew, ew, na)
    obs0 = PC.observations(20 + n + a, n, a, ew)
    ratios = []
    raw = Raw(n, a, ew, na, P)
    pol = DevicePolicy.from_state_dict(sd0, max_agents=a, ego_width=ew)
    logits_f = torch.empty((n, na), device="cuda")
    for ci, (name, sd, obs) in enumerate(_cases(sd0, obs0, a, ew)):
        what = "%s n=%d A=%d ego=%d actions=%d" % (name, n, a, ew, na)
        low = None
        if name == "copied_winner":
            obs, low = obs
        t_l, t_v = PC.stand_in_forward(sd, obs, a, ew, torch.float32)
        w_l, w_v, _ = REF.forward(sd, obs, a, ew)
        E_fwd = max(np.abs(t_l - w_l).max(), np.abs(t_v - w_v).max())
        pol.load_state_dict({k: v.cuda() for k, v in sd.items()})
        raw.load(sd)
        d_obs = torch.from_numpy(obs).cuda()
        # 1. forward identity: the logits, and the sampled actions' logprob, entropy and value, bit for bit
        actions, lp_f, ent_f, val_f = pol(d_obs, torch.from_numpy(PC.uniforms(n + ci, n)).cuda(), logits_out=logits_f)
        lp, ent, val, logits, winners = raw.evaluate(d_obs, actions, what)
        for nm, g, w in (("logits", logits, logits_f), ("logprob", lp, lp_f), ("entropy", ent, ent_f), ("value", val, val_f)):
            assert np.array_equal(g.view(np.int32), w.cpu().numpy().view(np.int32)), (what, nm, "differs from gd_policy_forward")
        if name == "lifted_actor_bias":
            # every sampled action is the lifted one; evaluate other actions too, so that the taken action's term counts
            assert (actions.cpu().numpy() == 3).all()
            mixed = np.where(np.arange(n) % 2 == 0, 3, np.random.default_rng(n).integers(0, na, n))
            actions = torch.from_numpy(mixed).cuda()
            lp, ent, val, logits2, winners = raw.evaluate(d_obs, actions, what)
            assert np.array_equal(logits2, logits)
            assert all(np.isfinite(x).all() for x in (lp, ent, val, logits))
        h_actions = actions.cpu().numpy()
        # 3. winners
        _check_winners(what, sd, obs, a, ew, winners, E_fwd)
        if name == "last_entity_wins":
            assert (winners[:, 0] == a - 2).all() and (winners[:, 64] == 199).all(), what
        if name == "all_padding_partners":
            assert (winners[:, :64] == 0).all(), what
        if low is not None:
            assert (winners[:, 0] == low[:, 0]).all() and (winners[:, 64] == low[:, 1]).all(), (what, "the lower index wins")
        # 2. gradients
        ups = GR.ppo_upstream(100 + n + ci, lp, ent, val)
        if n > 3:
            assert (ups[0] == 0).any() and (ups[0] != 0).any(), (what, "some rows clip and some do not")
        got = raw.backward(ups, what)
        _compare(what, sd, obs, a, ew, h_actions, ups, winners, got, ratios)
        if na == 1:
            # a softmax of one number: logprob and entropy are constants, so the float64 reference's actor gradients are
            # exactly zero, the yardstick E_p is zero there, and the kernel's must be zero as values
            assert (got["actor.weight"] == 0.0).all() and (got["actor.bias"] == 0.0).all(), (what, "one action")
            assert np.abs(got["critic.weight"]).max() > 0 and np.abs(got["shared_embed.0.weight"]).max() > 0, what
        if name != "seeded":
            continue
        # (vi) no gradient into logprob and entropy: the actor's gradients are exactly zero, the rest within the bound
        zero = np.zeros(n, dtype=np.float32)
        got6 = raw.backward([zero, zero, ups[2]], what + " (vi)")
        assert (got6["actor.weight"] == 0.0).all() and (got6["actor.bias"] == 0.0).all(), what + " (vi)"
        _compare(what + " (vi)", sd, obs, a, ew, h_actions, [zero, zero, ups[2]], winners, got6, ratios)
        # (vii) rows whose three upstream gradients are zero change no bit: two such rows appended, the same partials (with
        # the rows p, p + P, .. summed in order, the appended rows come last in every workgroup and add zeros)
        more = Raw(n + 2, a, ew, na, P)
        more.load(sd)
        obs2 = torch.cat([d_obs, d_obs[:1], d_obs[-1:]]).contiguous()
        act2 = torch.cat([actions, actions[:1], actions[-1:]]).contiguous()
        more.evaluate(obs2, act2, what + " (vii)")
        got7 = more.backward([np.concatenate([u, [0.0, 0.0]]) for u in ups], what + " (vii)")
        for k in got:
            assert np.array_equal(got7[k].view(np.int32), got[k].view(np.int32)), (what, k, "rows without gradient changed bits")
    return max(ratios)


@pytest.mark.parametrize("n,a,ew,na", PC.SHAPES, ids=lambda v: str(v))
def test_evaluate_and_backward_against_the_float64_reference(n, a, ew, na):
    _backward_case(n, a, ew, na)


@pytest.mark.parametrize("P", [1, 7])
@pytest.mark.parametrize("n,a,ew,na", PC.EDGE_SHAPES, ids=lambda v: str(v))
def test_evaluate_and_backward_at_the_action_counts_where_the_tiling_changes(n, a, ew, na, P):
    """[Wa; Wc] is walked eight rows at a time with no remainder loop: 8, 32 and 1024 put the critic's row first in a group,
    31 last, 33 second, 1 second of the only group; 1024 uses s_dl to its last index."""
    worst = _backward_case(n, a, ew, na, P)
    print("POLICY_EDGE backward n=%d A=%d ego=%d actions=%d partials=%d: largest error / E_p %.2f (bound %d)"
          % (n, a, ew, na, P, worst, BOUND), flush=True)


@pytest.mark.parametrize("a,ew,na", [(64, 6, 91), (128, 9, 7)])
def test_the_reduction_is_deterministic_for_every_partials(a, ew, na):
    n = 70
    sd = PC.state_dict(10 + na + ew, ew, na)
    obs = PC.observations(20 + n + a, n, a, ew)
    d_obs = torch.from_numpy(obs).cuda()
    actions = torch.from_numpy(np.random.default_rng(1).integers(0, na, n)).cuda()
    seen = {}
    for P in (1, 2, 7, 256, 1024):  # 256 is TrainablePolicy's default
        what = "partials=%d A=%d ego=%d actions=%d" % (P, a, ew, na)
        raw = Raw(n, a, ew, na, P)
        raw.load(sd)
        lp, ent, val, _, winners = raw.evaluate(d_obs, actions, what)
        ups = GR.ppo_upstream(5, lp, ent, val)
        got = raw.backward(ups, what)
        _compare(what, sd, obs, a, ew, actions.cpu().numpy(), ups, winners, got)
        again = raw.backward(ups, what)
        for k in got:
            assert np.array_equal(again[k].view(np.int32), got[k].view(np.int32)), (what, k, "two calls differ")
        seen[P] = got
    assert any(not np.array_equal(seen[1][k], seen[7][k]) for k in seen[1]), "the order of summation follows partials"


def _module(a, ew, na, **kw):
    from gpudrive_lab_amd.policy import TrainablePolicy
    sd = PC.state_dict(10 + na + ew, ew, na)
    return sd, TrainablePolicy.from_state_dict(sd, max_agents=a, ego_width=ew, device="cuda", **kw)


def test_the_module_allocates_what_nbytes_says_and_never_synchronises():
    n, a, ew, na = 70, 64, 6, 91
    sd, tp = _module(a, ew, na)
    obs = torch.from_numpy(PC.observations(3, n, a, ew)).cuda()
    actions = torch.from_numpy(np.random.default_rng(2).integers(0, na, n)).cuda()
    ups = [torch.randn(n, device="cuda") / n for _ in range(3)]
    _, lp, ent, val = tp(obs, actions)                      # (the first call loads the library and the kernels)
    torch.autograd.backward([lp, ent, val], ups)
    tp.zero_grad(set_to_none=True)
    del lp, ent, val
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()

    def once():
        _, lp, ent, val = tp(obs, actions)
        torch.autograd.backward([lp, ent, val], ups)

    _no_sync(once)
    rise = torch.cuda.max_memory_allocated() - before
    print("policy backward n=%d: peak rise %d bytes, nbytes %d" % (n, rise, tp.nbytes(n)))
    assert 0 < rise <= tp.nbytes(n)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tp.parameters())


def test_the_module_surface():
    from gpudrive_lab_amd.policy import DevicePolicy
    n, a, ew, na = 3, 64, 9, 7
    sd, tp = _module(a, ew, na, partials=7)
    obs_h = PC.observations(3, n, a, ew)
    obs = torch.from_numpy(obs_h).cuda()
    # the state dict round-trips with the stand-in, and feeds DevicePolicy
    net = PC.StandIn(a, ew, na, dropout=0.0)
    net.load_state_dict({k: v.cpu() for k, v in tp.state_dict().items()})
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    pol = DevicePolicy.from_state_dict(sd, max_agents=a, ego_width=ew)
    pol.load_state_dict(tp.state_dict())
    actions, lp_f, ent_f, val_f = pol(obs, torch.from_numpy(PC.uniforms(1, n)).cuda())
    ret, lp, ent, val = tp(obs, actions)
    assert ret is actions and lp.requires_grad and ent.requires_grad and val.requires_grad
    assert torch.equal(lp, lp_f) and torch.equal(ent, ent_f) and torch.equal(val, val_f)  # the first-epoch ratio is exactly 1
    with pytest.raises(ValueError):
        tp(obs.clone().requires_grad_(True), actions)
    # two forwards before one backward both work, and .grad accumulates over two backwards
    other = torch.from_numpy(np.random.default_rng(4).integers(0, na, n)).cuda()
    _, lp2, ent2, val2 = tp(obs, other)
    ups = [torch.from_numpy(u).cuda() for u in GR.ppo_upstream(9, lp.detach().cpu().numpy(), ent.detach().cpu().numpy(),
                                                               val.detach().cpu().numpy())]
    torch.autograd.backward([lp, ent, val], ups)
    first = {k: p.grad.clone() for k, p in tp.named_parameters()}
    torch.autograd.backward([lp2, ent2, val2], ups)
    tp.zero_grad(set_to_none=True)
    torch.autograd.backward(list(tp(obs, other)[1:]), ups)
    second = {k: p.grad.clone() for k, p in tp.named_parameters()}
    tp.zero_grad(set_to_none=True)
    torch.autograd.backward(list(tp(obs, actions)[1:]), ups)
    torch.autograd.backward(list(tp(obs, other)[1:]), ups)
    for k, p in tp.named_parameters():
        assert tuple(p.grad.shape) == tuple(sd[k].shape)
        assert torch.equal(p.grad, first[k] + second[k]), (k, ".grad is the sum of the two backwards")
    with pytest.raises(RuntimeError):  # once differentiable, and the graph is freed
        torch.autograd.backward([lp, ent, val], ups)
    # an optimiser step between forward and backward is torch's error
    opt = torch.optim.SGD(tp.parameters(), lr=0.1)
    _, lp, ent, val = tp(obs, actions)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.backward([lp, ent, val], ups)


def test_one_sgd_step_moves_the_parameters_as_the_float64_reference_does():
    n, a, ew, na, lr = 70, 64, 6, 91, 0.05
    sd, tp = _module(a, ew, na, partials=7)
    obs_h = PC.observations(3, n, a, ew)
    obs = torch.from_numpy(obs_h).cuda()
    actions_h = np.random.default_rng(2).integers(0, na, n)
    actions = torch.from_numpy(actions_h).cuda()
    _, lp, ent, val = tp(obs, actions)
    old = [torch.from_numpy(t).cuda() for t in GR.minibatch(11, lp.detach().cpu().numpy(), val.detach().cpu().numpy())]
    loss = GR.ppo_loss(lp, ent, val, *old)                  # the reference's loss, in torch on the device, float32
    winners = lp.grad_fn.kept[3].cpu().numpy()               # this call's saved winners
    opt = torch.optim.SGD(tp.parameters(), lr=lr)
    opt.zero_grad()
    loss.backward()
    opt.step()
    # float64: the same loss through the stand-in at the same winners
    net = GR.stand_in(sd, a, ew, torch.float64)
    lp64, ent64, val64, _, _ = GR.evaluate(net, obs_h, actions_h, winners)
    GR.ppo_loss(lp64, ent64, val64, *(t.cpu().double() for t in old)).backward()
    net32 = GR.stand_in(sd, a, ew, torch.float32)
    lp32, ent32, val32, _, _ = GR.evaluate(net32, obs_h, actions_h, winners)
    GR.ppo_loss(lp32, ent32, val32, *(t.cpu() for t in old)).backward()
    g64 = {k: p.grad.numpy() for k, p in net.named_parameters()}
    E = GR.yardstick(g64, {k: p.grad.double().numpy() for k, p in net32.named_parameters()})
    for k, p in tp.named_parameters():
        want = sd[k].double().numpy() - lr * g64[k]
        err = np.abs(p.detach().cpu().double().numpy() - want).max()
        # the gradient's bound times the learning rate, plus the rounding of the float32 parameter itself
        assert err <= lr * BOUND * E[k] + 2.0 ** -24 * np.abs(want).max(), (k, err, lr * BOUND * E[k])
        assert np.abs(want - sd[k].double().numpy()).max() > 100 * lr * BOUND * E[k], (k, "the step is visible")
