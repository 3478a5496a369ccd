"""GPU suite: the device PPO update (gpudrive_lab_amd.ppo.DevicePPO; gd_ppo_loss, gd_ppo_adam, gd_ppo_update) against torch
in float64 on the CPU (tests/ppo_update_reference.py) and against the rule's host program.

The yardstick is the project's: E of a quantity is the error of the same lines in torch float32 on the CPU against float64,
floored at 2^-23 max |float64|; the kernel's error must be <= C E, C the next power of two at or above twice the largest
ratio measured on the MI355X against the float64 reference (DESIGN.md section 5 tabulates them):
  C_DEV = 4   gd_ppo_loss: largest ratio 1.28 (policy_loss, M = 1025, norm_adv on; 0.52, 1.00, 0.80, 0.95 at M = 2, 3, 70, 257)
  C_E2E = 4   one whole update, the parameters after it: largest ratio 1.23 (shared_embed.0.weight)
The optimiser step has no transcendental, and sqrt and division are correctly rounded on both sides: it is held to the host
program bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import policy_cases as PC
from tests import policy_grad_reference as GR
from tests import ppo_update_reference as UR
from tests.test_gpu_policy import Carver, _no_sync
from tests.test_ppo_update import C_ADAM

pytestmark = pytest.mark.gpu

C_DEV = 4
C_E2E = 4
A = 64
SHAPES = ((6, 91), (9, 7), (6, 31))
# the action counts where the tiling of the heads changes (tests/policy_cases.py EDGE_SHAPES)
EDGE_SHAPES = ((6, 1), (9, 8), (6, 32), (9, 33), (6, 1024))
EDGE_UPDATES = ((33, 6, 1), (33, 9, 32), (3, 6, 1024))  # (n, ego_width, n_actions) of one whole update


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.uint8 if a.dtype.itemsize == 1 else np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- gd_ppo_loss

@pytest.mark.parametrize("m", UR.ROWS)
def test_the_loss_kernel_against_the_float64_reference(m):
    L = _capi.lib()
    x = UR.loss_inputs(m)
    UR.assert_gaps(x, "M = %d" % m)
    dev = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in x]
    nlp, ent, nv, old_lp, old_v, adv, ret = dev
    c = Carver()
    f = torch.float32
    out = [c.carve(n, (m,), f) for n in ("d_logprob", "d_entropy", "d_value")]
    stats, stats_sum = c.carve("stats", (6,), f), c.carve("stats_sum", (6,), f)  # (stats[6] is the optimiser step's)
    worst = 0.0
    for norm_adv, clip_vloss in UR.FLAGS:
        what = "M = %d norm_adv %s clip_vloss %s" % (m, norm_adv, clip_vloss)
        o = _capi.GdPPO()
        o.num_rows, o.norm_adv, o.clip_vloss = m, int(norm_adv), int(clip_vloss)
        o.clip_coef, o.vf_clip_coef, o.ent_coef, o.vf_coef = (UR.HYPER[k] for k in ("clip_coef", "vf_clip_coef", "ent_coef", "vf_coef"))
        o.stats_scale = 0.5
        o.stats, o.stats_sum = stats.data_ptr(), stats_sum.data_ptr()

        def call():
            _capi.check(L.gd_ppo_loss(C.byref(o), nlp.data_ptr(), ent.data_ptr(), nv.data_ptr(), old_lp.data_ptr(),
                                      old_v.data_ptr(), adv.data_ptr(), ret.data_ptr(), *(t.data_ptr() for t in out), _stream()))

        c.refill()
        stats_sum.zero_()
        _no_sync(call)
        c.assert_guards_and_written(what)
        got = [t.cpu().numpy().copy() for t in out] + [stats.cpu().numpy().copy()]
        r64 = UR.loss_reference(x, torch.float64, norm_adv, clip_vloss)
        r32 = UR.loss_reference(x, torch.float32, norm_adv, clip_vloss)
        pairs = [(n, got[k], r64[k], r32[k]) for k, n in enumerate(("d_logprob", "d_entropy", "d_value"))]
        pairs += [(n, got[3][k], r64[3][k], r32[3][k]) for k, n in enumerate(UR.STATS)]
        for name, g, w64, w32 in pairs:
            assert np.isfinite(g).all(), (what, name)
            err, E = UR.error_floor(g, w64, w32)
            ratio = UR.ratio_of(err, E)
            if ratio > worst:
                worst = ratio
                print("ppo loss kernel %s: error / E %.2f at %s" % (what, ratio, name))
        for name, g, w64, w32 in pairs:
            err, E = UR.error_floor(g, w64, w32)
            assert err <= C_DEV * E, (what, name, "error %.3g above %d E = %.3g" % (err, C_DEV, C_DEV * E))
        one = np.flatnonzero(x[0] == x[3])
        assert len(one) and (r64[0][one] != 0).all() and (got[0][one] != 0).all(), (what, "ratio == 1 is the unclipped branch")
        # a second call: the same bits, and stats_sum is the order-fixed float32 sum (0 + 0.5 s) + 0.5 s
        once = stats_sum.cpu().numpy().copy()
        half = np.float32(0.5) * got[3]
        assert _same(once, np.float32(0.0) + half), what
        _no_sync(call)
        c.assert_guards_and_written(what + " (second call)")
        for name, t, g in zip(("d_logprob", "d_entropy", "d_value", "stats"), out + [stats], got):
            assert _same(t, g), (what, name, "two calls differ")
        assert _same(stats_sum, (np.float32(0.0) + half) + half), what
    print("ppo loss kernel M=%d: largest error / E %.2f" % (m, worst))


# ---- gd_ppo_adam

@pytest.mark.parametrize("ew,na", SHAPES + EDGE_SHAPES, ids=lambda v: str(v))
def test_the_optimiser_step_is_the_host_programs_bit_for_bit(ew, na):
    from gpudrive_lab_amd.policy import grad_floats, pack_index
    from gpudrive_lab_amd.ppo import blob_of
    L = _capi.lib()
    G, index = grad_floats(ew, na), pack_index(ew, na)
    sd = PC.state_dict(10 + na + ew, ew, na)
    flat0 = np.concatenate([sd[k].numpy().reshape(-1) for k in sd] + [np.zeros(1, np.float32)])
    grads = UR.adam_gradients(G, seed=na)
    host = UR.run_adam_host(flat0[:G], np.zeros(G, np.float32), np.zeros(G, np.float32), grads, **UR.ADAM)
    c = Carver()
    f = torch.float32
    params, m, v = c.carve("params", (G + 1,), f), c.carve("exp_avg", (G,), f), c.carve("exp_avg_sq", (G,), f)
    blob, stats, stats_sum = c.carve("blob", (len(index),), f), c.carve("stats", (7,), f), c.carve("stats_sum", (7,), f)
    scal, step, lr = c.carve("scal", (4,), f), c.carve("step", (1,), torch.int32), c.carve("lr", (1,), f)
    beta_pow = c.carve("beta_pow", (2,), torch.int64).view(torch.float64)
    params.copy_(torch.from_numpy(flat0))
    blob.copy_(torch.from_numpy(flat0[index]))
    for t in (m, v, stats, stats_sum, scal, step):
        t.zero_()
    lr.fill_(UR.ADAM["lr"])
    beta_pow.fill_(1.0)
    inverse = torch.from_numpy(blob_of(ew, na)).cuda()
    o = _capi.GdPPO()
    o.ego_width, o.n_actions, o.grad_floats, o.blob_floats = ew, na, G, len(index)
    o.max_grad_norm, o.eps, o.stats_scale = UR.ADAM["max_norm"], UR.ADAM["eps"], 1.0
    o.beta1, o.beta2 = UR.ADAM["betas"]
    o.lr, o.step, o.beta_pow = lr.data_ptr(), step.data_ptr(), beta_pow.data_ptr()
    o.params, o.exp_avg, o.exp_avg_sq, o.blob, o.blob_of = (t.data_ptr() for t in (params, m, v, blob, inverse))
    o.stats, o.stats_sum, o.scal = stats.data_ptr(), stats_sum.data_ptr(), scal.data_ptr()
    total_sum = np.float32(0.0)
    for s, g in enumerate(grads):
        what = "ego=%d actions=%d step %d" % (ew, na, s + 1)
        d_g = torch.from_numpy(g).cuda()
        _no_sync(lambda: _capi.check(L.gd_ppo_adam(C.byref(o), d_g.data_ptr(), _stream())))
        c.assert_guards_and_written(what)
        h = host[s]
        flat = params.cpu().numpy()
        assert _same(flat[:G], h["params"]), (what, "params")
        assert flat[G] == 0.0 and _bits(flat)[G] == 0, (what, "the trailing zero stays zero")
        assert _same(m, h["exp_avg"]) and _same(v, h["exp_avg_sq"]), (what, "the moments")
        assert int(step.item()) == h["step"] == s + 1 and _same(beta_pow, h["beta_pow"]), (what, "step and the running products")
        assert _same(stats[6], h["total"]), (what, "grad_norm")
        assert (stats[:6] == 0).all(), (what, "the loss's statistics are not the optimiser step's")
        total_sum = total_sum + h["total"]
        assert _same(stats_sum[6], total_sum), what
        assert _same(blob, flat[index]), (what, "blob == flat[pack_index]")
        assert (blob.cpu().numpy()[index == G] == 0).all(), (what, "the padding entries")
    z = UR.zero_block(G)
    assert (grads[0][z] == 0).all() and _same(host[0]["params"][z], flat0[:G][z])


# ---- gd_ppo_update and DevicePPO

HYPER = dict(UR.HYPER, learning_rate=UR.ADAM["lr"], betas=UR.ADAM["betas"], eps=UR.ADAM["eps"], max_grad_norm=UR.ADAM["max_norm"])


def _ppo(n, ew, na, **kw):
    from gpudrive_lab_amd.ppo import DevicePPO
    sd = PC.state_dict(10 + na + ew, ew, na)
    return sd, DevicePPO(sd, max_agents=A, ego_width=ew, minibatch_size=n, partials=7, **dict(HYPER, **kw))


def _sampled(ppo, n, ew, seed=3):
    """Seeded observations, and the actions, logprobs and values `ppo.policy` samples on them (device tensors)."""
    obs = torch.from_numpy(PC.observations(seed, n, A, ew)).cuda()
    actions, logprob, _, value = ppo.policy(obs, torch.from_numpy(PC.uniforms(seed + 1, n)).cuda())
    return obs, actions, logprob, value


def _state(ppo):
    return dict(flat=ppo.flat, exp_avg=ppo.exp_avg, exp_avg_sq=ppo.exp_avg_sq, blob=ppo.policy.blob, stats=ppo.stats,
                stats_sum=ppo.stats_sum, step=ppo._step, beta_pow=ppo._beta_pow, grad=ppo.grad, winners=ppo.winners,
                **{"row%d" % i: t for i, t in enumerate(ppo._rows)})


def test_one_call_is_the_four_calls_and_allocates_nothing():
    n, ew, na = 70, 6, 91
    L = _capi.lib()
    _, one = _ppo(n, ew, na, clip_vloss=True)
    _, four = _ppo(n, ew, na, clip_vloss=True)
    obs, actions, lp, val = _sampled(one, n, ew)
    old_lp, adv, ret, old_v = (torch.from_numpy(t).cuda() for t in GR.minibatch(11, lp.cpu().numpy(), val.cpu().numpy()))
    one.update(obs, actions, old_lp, old_v, adv, ret)  # (the first call loads the kernels)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    _no_sync(lambda: one.update(obs, actions, old_lp, old_v, adv, ret))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before

    p, g, o = four._p, four._g, four._o
    r = four._rows

    def separately():
        _capi.check(L.gd_policy_evaluate(C.byref(p), C.byref(g), obs.data_ptr(), actions.data_ptr(), r[0].data_ptr(), r[1].data_ptr(),
                                         r[2].data_ptr(), _stream()))
        _capi.check(L.gd_ppo_loss(C.byref(o), r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), old_lp.data_ptr(), old_v.data_ptr(),
                                  adv.data_ptr(), ret.data_ptr(), r[3].data_ptr(), r[4].data_ptr(), r[5].data_ptr(), _stream()))
        _capi.check(L.gd_policy_backward(C.byref(p), C.byref(g), obs.data_ptr(), actions.data_ptr(), r[3].data_ptr(), r[4].data_ptr(),
                                         r[5].data_ptr(), four.grad.data_ptr(), _stream()))
        _capi.check(L.gd_ppo_adam(C.byref(o), four.grad.data_ptr(), _stream()))

    for _ in range(2):
        _no_sync(separately)
    got, want = _state(one), _state(four)
    for k in got:
        assert _same(got[k], want[k]), (k, "gd_ppo_update differs from the four calls")
    assert int(one._step.item()) == 2 and np.isfinite(one.flat.cpu().numpy()).all()
    G, P, B = one.G, 7, one.policy.blob.numel()
    floats = (G + 1) + 2 * G + G + P * G + n * (192 + na + 8 + 6) + 1 + 7 + 7 + 4  # flat, moments, grad, partials, rows, scalars
    assert one.nbytes == 4 * floats + 4 * G + n * 128 + 4 + 2 * 8 + (4 * B + 8 * B + 4), "blob_of, winners, step, beta_pow; the policy"


def test_the_first_epochs_ratio_is_exactly_one():
    n, ew, na = 70, 9, 7
    _, ppo = _ppo(n, ew, na)
    obs, actions, lp, val = _sampled(ppo, n, ew)
    adv = torch.from_numpy(np.random.default_rng(1).normal(0, 1, n).astype(np.float32)).cuda()
    _no_sync(lambda: ppo.update(obs, actions, lp, val, adv, (val + adv).contiguous()))
    stats = dict(zip(_capi.PPO_STATS, ppo.stats.cpu().numpy().tolist()))
    assert stats["old_approx_kl"] == 0.0 and stats["approx_kl"] == 0.0 and stats["clipfrac"] == 0.0, stats
    assert stats["grad_norm"] > 0 and np.isfinite(list(stats.values())).all()
    assert _same(ppo._rows[0], lp) and _same(ppo._rows[2], val), "evaluating the sampled actions returns their logprob and value"


def _updated(n, ew, na):
    sd, ppo = _ppo(n, ew, na, clip_vloss=True)
    obs, actions, lp, val = _sampled(ppo, n, ew)
    old = GR.minibatch(11, lp.cpu().numpy(), val.cpu().numpy())  # (old_logprob, adv, ret, old_value)
    old_lp, adv, ret, old_v = (torch.from_numpy(t).cuda() for t in old)
    _no_sync(lambda: ppo.update(obs, actions, old_lp, old_v, adv, ret))
    return dict(n=n, ew=ew, na=na, sd=sd, ppo=ppo, obs=obs, actions=actions.cpu().numpy(), old=old,
                winners=ppo.winners.cpu().numpy().copy(), after={k: v.cpu().numpy() for k, v in ppo.state_dict().items()})


@pytest.fixture(scope="module")
def updated():
    """One update at n = 70, (6, 91), with `minibatch`'s perturbed old logprobs and values; everything on the host."""
    return _updated(70, 6, 91)


def _check_update(u, what="ppo update end to end"):
    obs_h = u["obs"].cpu().numpy()
    kw = dict(norm_adv=True, clip_vloss=True)
    p64, g64 = UR.pipeline(u["sd"], A, u["ew"], obs_h, u["actions"], u["winners"], u["old"], torch.float64, **kw)
    p32, _ = UR.pipeline(u["sd"], A, u["ew"], obs_h, u["actions"], u["winners"], u["old"], torch.float32, **kw)
    E = GR.yardstick(p64, p32)
    worst, at = 0.0, None
    for k in p64:
        assert np.isfinite(u["after"][k]).all(), k
        ratio = UR.ratio_of(float(np.abs(u["after"][k] - p64[k]).max()), E[k])
        if ratio > worst:
            worst, at = ratio, k
    print("%s: largest error / E %.2f at %s" % (what, worst, at))
    for k in p64:
        err = float(np.abs(u["after"][k] - p64[k]).max())
        assert err <= C_E2E * E[k], (k, "error %.3g above %d E = %.3g" % (err, C_E2E, C_E2E * E[k]))
        if np.any(g64[k] != 0):
            moved = float(np.abs(u["after"][k].astype(np.float64) - u["sd"][k].double().numpy()).max())
            assert moved > 100 * C_E2E * E[k], (k, "the step is visible", moved, E[k])
    return g64


def test_one_update_moves_the_parameters_as_the_float64_pipeline_does(updated):
    g64 = _check_update(updated)
    assert all(np.any(g64[k] != 0) for k in g64), "every tensor has a gradient here"


@pytest.mark.parametrize("n,ew,na", EDGE_UPDATES, ids=lambda v: str(v))
def test_one_update_at_the_action_counts_where_the_tiling_changes(n, ew, na):
    u = _updated(n, ew, na)
    g64 = _check_update(u, "POLICY_EDGE ppo update n=%d ego=%d actions=%d (bound %d)" % (n, ew, na, C_E2E))
    for k in g64:
        if na == 1 and k.startswith("actor."):
            # a softmax of one number has no gradient: float64 leaves the actor where it was, and so must the device, bit for bit
            assert not np.any(g64[k] != 0) and _same(u["after"][k], u["sd"][k].numpy()), k
        else:
            assert np.any(g64[k] != 0), (k, "the tensor has a gradient here")


def test_the_blob_stored_in_place_is_the_repack(updated):
    from gpudrive_lab_amd.policy import DevicePolicy, grad_floats, pack_index
    u = updated
    ppo, n, na = u["ppo"], u["n"], u["na"]
    fresh = DevicePolicy.from_state_dict(ppo.state_dict(), max_agents=A, ego_width=u["ew"])
    assert _same(ppo.policy.blob, fresh.blob)
    assert _same(ppo.policy.blob, ppo.flat.cpu().numpy()[pack_index(u["ew"], na)]) and float(ppo.flat[-1]) == 0.0
    uni = torch.from_numpy(PC.uniforms(8, n)).cuda()
    logits = [torch.empty((n, na), device="cuda") for _ in range(2)]
    a = ppo.policy(u["obs"], uni, logits_out=logits[0])
    b = fresh(u["obs"], uni, logits_out=logits[1])
    assert _same(logits[0], logits[1]) and all(_same(x, y) for x, y in zip(a, b))
    assert not _same(ppo.flat[:grad_floats(u["ew"], na)], np.concatenate([v.numpy().reshape(-1) for v in u["sd"].values()]))


def _rollout(ppo, ew, na, seed=0):
    """DeviceRollout(batch_size=32, minibatch_size=16, num_rows=8) filled from seeded tensors, sorted, with advantages."""
    from gpudrive_lab_amd.rollout import DeviceRollout
    ro = DeviceRollout(32, 16, 1, num_rows=8, obs_width=ppo.obs_width)
    rng = np.random.default_rng(seed)
    for t in range(4):
        obs = torch.from_numpy(PC.observations(seed + t, 8, A, ew)).cuda()
        actions, logprob, _, value = ppo.policy(obs, torch.from_numpy(PC.uniforms(seed + 10 + t, 8)).cuda())
        reward = torch.from_numpy(rng.normal(0, 1, 8).astype(np.float32)).cuda()
        done = torch.from_numpy(rng.random(8) < 0.2).cuda()
        ro.store(obs, value, actions, logprob, reward, done, torch.ones(8, dtype=torch.bool, device="cuda"))
    ro.sort_training_data()
    ro.compute_gae(0.99, 0.95)
    return ro


def test_train_is_the_loop_of_minibatch_and_update():
    ew, na = 9, 7
    _, loop = _ppo(16, ew, na)
    _, hand = _ppo(16, ew, na)
    ro = _rollout(loop, ew, na)
    before = loop.nbytes
    loop.train(ro, 1)       # (the first call allocates the minibatch buffers)
    hand_stats = []

    def by_hand(epochs):
        for _ in range(epochs):
            for mb in range(ro.num_minibatches):
                obs, actions, logprobs, _, values, advantages, returns = ro.minibatch(mb)
                hand.update(obs, actions, logprobs, values, advantages, returns)
                hand_stats.append(hand.stats.clone())

    by_hand(1)
    assert loop.nbytes == before + sum(int(np.prod(s)) * torch.empty((), dtype=dt).element_size() for s, dt in ro.batch_shapes())
    assert loop.losses()["grad_norm"] > 0 and loop.host_reads == 1
    del hand_stats[:]
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    _no_sync(lambda: loop.train(ro, 2))
    assert torch.cuda.memory_allocated() == allocated
    by_hand(2)
    got, want = _state(loop), _state(hand)
    for k in got:
        if k != "stats_sum":
            assert _same(got[k], want[k]), (k, "train differs from the loop written by hand")
    assert int(loop._step.item()) == 6 and len(hand_stats) == 4
    per = np.stack([s.cpu().numpy() for s in hand_stats])
    total = np.zeros(7, np.float32)
    for s in per:
        total = total + s          # the float32 running sum the kernels keep
    losses = loop.losses()
    assert loop.host_reads == 2 and list(losses) == list(_capi.PPO_STATS)
    for i, k in enumerate(_capi.PPO_STATS):
        assert losses[k] == float(total[i]) / 4, k
        assert abs(losses[k] - per[:, i].astype(np.float64).mean()) <= 2.0 ** -21 * np.abs(per[:, i]).max(), k
    assert (loop.stats_sum == 0).all() and all(v == 0.0 for v in loop.losses().values())
    loop.set_learning_rate(1e-4)
    assert float(loop._lr) == float(np.float32(1e-4)) and loop.learning_rate == 1e-4


def test_the_optimiser_state_round_trips_with_torch():
    from gpudrive_lab_amd.policy import TrainablePolicy
    n, ew, na = 16, 9, 7
    L = _capi.lib()
    _, ppo = _ppo(n, ew, na)
    obs, actions, lp, val = _sampled(ppo, n, ew)
    old_lp, adv, ret, old_v = (torch.from_numpy(t).cuda() for t in GR.minibatch(4, lp.cpu().numpy(), val.cpu().numpy()))
    for _ in range(2):
        ppo.update(obs, actions, old_lp, old_v, adv, ret)
    # loading its own state changes no bit
    keep = {k: v.clone() for k, v in _state(ppo).items()}
    lr = ppo._lr.clone()
    osd = ppo.optimizer_state_dict()
    ppo.load_optimizer_state_dict(osd)
    now = _state(ppo)
    assert all(_same(now[k], keep[k]) for k in keep) and _same(ppo._lr, lr)
    tensors = len(ppo._shapes)
    assert len(osd["state"]) == tensors == 24 and float(osd["state"][0]["step"]) == 2.0 and osd["param_groups"][0]["eps"] == 1e-5
    # one further step on a fed gradient: torch's Adam on the device from this state, and float64 / float32 on the CPU
    sd = {k: v.cpu() for k, v in ppo.state_dict().items()}
    fed = UR.adam_gradients(ppo.G, seed=1)[2]
    ad = UR.ADAM

    def torch_step(params, device):
        opt = torch.optim.Adam(params, lr=ad["lr"], betas=ad["betas"], eps=ad["eps"], foreach=False)
        opt.load_state_dict(copy.deepcopy(osd))  # (torch adopts the `step` tensors it is given and advances them in place)
        o = 0
        for p in params:
            # (a copy: clip_grad_norm_ scales .grad in place, and a float32 CPU tensor would share `fed`'s memory)
            p.grad = torch.tensor(fed[o:o + p.numel()]).to(device=device, dtype=p.dtype).view(p.shape)
            o += p.numel()
        torch.nn.utils.clip_grad_norm_(params, ad["max_norm"], foreach=False)
        opt.step()
        return opt

    tp = TrainablePolicy.from_state_dict(sd, max_agents=A, ego_width=ew, device="cuda")
    torch_step(list(tp.parameters()), "cuda")
    nets = {dt: GR.stand_in(sd, A, ew, dt) for dt in (torch.float64, torch.float32)}
    opts = {dt: torch_step(list(net.parameters()), "cpu") for dt, net in nets.items()}
    d_fed = torch.from_numpy(fed).cuda()
    _capi.check(L.gd_ppo_adam(C.byref(ppo._o), d_fed.data_ptr(), _stream()))
    mine = ppo.state_dict()
    p64 = {k: p.detach().numpy() for k, p in nets[torch.float64].named_parameters()}
    E = GR.yardstick(p64, {k: p.detach().double().numpy() for k, p in nets[torch.float32].named_parameters()})
    for k, p in tp.named_parameters():
        got = mine[k].cpu().double().numpy()
        assert np.abs(got - p64[k]).max() <= C_ADAM * E[k], (k, "against float64")
        assert np.abs(got - p.detach().cpu().double().numpy()).max() <= C_ADAM * E[k], (k, "against torch.optim.Adam on the device")
        assert np.abs(got - sd[k].double().numpy()).max() > 0, (k, "the step moved it")
    # and the state after that step is torch's, to float32 rounding of the moments
    after = ppo.optimizer_state_dict()
    st64 = opts[torch.float64].state_dict()["state"]
    for i in range(tensors):
        assert float(after["state"][i]["step"]) == 3.0 == float(st64[i]["step"])
        for name in ("exp_avg", "exp_avg_sq"):
            want = st64[i][name].numpy()
            assert np.abs(after["state"][i][name].cpu().double().numpy() - want).max() <= 2.0 ** -21 * np.abs(want).max(), (i, name)
