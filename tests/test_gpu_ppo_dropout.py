"""GPU suite: the device PPO update with training-mode dropout (gpudrive_lab_amd.ppo.DevicePPO(dropout_rule=...);
gd_ppo_update_dropout) against the float64 chain of tests/ppo_update_reference.py with the host program's masks injected
(tests/dropout_reference.py), by test_gpu_ppo_update.py's yardstick and its bound of 4: the masks add one multiply per masked
site to the kernels and to the yardstick alike."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import dropout_reference as DREF
from tests import policy_cases as PC
from tests import policy_grad_reference as GR
from tests import ppo_update_reference as UR
from tests.test_gpu_policy import _no_sync
from tests.test_gpu_ppo_update import A, C_E2E, HYPER, _same, _state, _stream

pytestmark = pytest.mark.gpu

N, EW, NA = 70, 6, 91


def _ppo(rule, **kw):
    from gpudrive_lab_amd.ppo import DevicePPO
    sd = PC.state_dict(10 + NA + EW, EW, NA)
    return sd, DevicePPO(sd, max_agents=A, ego_width=EW, minibatch_size=N, partials=7, dropout_rule=rule, **dict(HYPER, **kw))


def _rule(p, seed=31):
    from gpudrive_lab_amd.dropout import DropoutRule
    return DropoutRule(p, seed)


def _sampled(ppo, seed=3):
    obs = torch.from_numpy(PC.observations(seed, N, A, EW)).cuda()
    actions, logprob, _, value = ppo.policy(obs, torch.from_numpy(PC.uniforms(seed + 1, N)).cuda())
    return obs, actions, logprob, value


def _pipeline(sd, obs, actions, winners, old, dtype, keep, scale):
    """`ppo_update_reference.pipeline` (norm_adv, clip_vloss) with the masks injected into the stand-in."""
    net, lp, ent, val = DREF.evaluate(sd, obs, A, EW, actions, winners, dtype, keep, scale)
    old_lp, adv, ret, old_v = (torch.tensor(np.asarray(t)).to(dtype) for t in old)
    loss, _ = UR.ppo_loss(lp, ent, val, old_lp, adv, ret, old_v, norm_adv=True, clip_vloss=True, **UR.HYPER)
    ad = UR.ADAM
    opt = torch.optim.Adam(net.parameters(), lr=ad["lr"], betas=ad["betas"], eps=ad["eps"], foreach=False)
    opt.zero_grad()
    loss.backward()
    grads = {k: q.grad.double().numpy().copy() for k, q in net.named_parameters()}
    torch.nn.utils.clip_grad_norm_(net.parameters(), ad["max_norm"], foreach=False)
    opt.step()
    return {k: q.detach().double().numpy().copy() for k, q in net.named_parameters()}, grads


@pytest.mark.parametrize("p", [0.01, 0.5])
def test_one_update_moves_the_parameters_as_the_masked_float64_pipeline_does(p):
    rule = _rule(p)
    sd, ppo = _ppo(rule, clip_vloss=True)
    obs, actions, lp, val = _sampled(ppo)
    assert rule.call == 1, "the rollout forward consumed index 0"
    old = GR.minibatch(11, lp.cpu().numpy(), val.cpu().numpy())
    old_lp, adv, ret, old_v = (torch.from_numpy(t).cuda() for t in old)
    _no_sync(lambda: ppo.update(obs, actions, old_lp, old_v, adv, ret))
    assert rule.call == 2 and int(ppo._used.item()) == 1, "the update consumed index 1 and left it in `used`"
    keep = DREF.host_masks(rule.seed, 1, rule.threshold, N, A)
    obs_h, actions_h, winners = obs.cpu().numpy(), actions.cpu().numpy(), ppo.winners.cpu().numpy()
    after = {k: v.cpu().numpy() for k, v in ppo.state_dict().items()}
    p64, g64 = _pipeline(sd, obs_h, actions_h, winners, old, torch.float64, keep, rule.scale)
    p32, _ = _pipeline(sd, obs_h, actions_h, winners, old, torch.float32, keep, rule.scale)
    E = GR.yardstick(p64, p32)
    worst, at = 0.0, None
    for k in p64:
        assert np.isfinite(after[k]).all(), k
        ratio = UR.ratio_of(float(np.abs(after[k] - p64[k]).max()), E[k])
        if ratio > worst:
            worst, at = ratio, k
    print("ppo dropout update p=%g: largest error / E %.2f at %s (bound %d)" % (p, worst, at, C_E2E))
    for k in p64:
        err = float(np.abs(after[k] - p64[k]).max())
        assert err <= C_E2E * E[k], (k, "error %.3g above %d E = %.3g" % (err, C_E2E, C_E2E * E[k]))
        if np.any(g64[k] != 0):
            moved = float(np.abs(after[k].astype(np.float64) - sd[k].double().numpy()).max())
            assert moved > 100 * C_E2E * E[k], (k, "the step is visible", moved, E[k])
    # the rollout's mask (index 0) and the update's (index 1) differ, as in the reference: the first epoch's ratio is not 1
    stats = dict(zip(_capi.PPO_STATS, ppo.stats.cpu().numpy().tolist()))
    assert np.isfinite(list(stats.values())).all() and stats["grad_norm"] > 0
    if p == 0.5:
        _, fresh = _ppo(_rule(p), clip_vloss=True)
        obs, actions, lp, val = _sampled(fresh)
        adv = torch.from_numpy(np.random.default_rng(1).normal(0, 1, N).astype(np.float32)).cuda()
        fresh.update(obs, actions, lp, val, adv, (val + adv).contiguous())
        stats = dict(zip(_capi.PPO_STATS, fresh.stats.cpu().numpy().tolist()))
        assert stats["approx_kl"] != 0.0 and not _same(fresh._rows[0], lp), stats


def test_one_call_is_the_four_dropout_calls_and_allocates_nothing():
    L = _capi.lib()
    r_one, r_four = _rule(0.5), _rule(0.5)
    _, one = _ppo(r_one, clip_vloss=True)
    _, four = _ppo(r_four, clip_vloss=True)
    obs, actions, lp, val = _sampled(one)
    _sampled(four)
    old_lp, adv, ret, old_v = (torch.from_numpy(t).cuda() for t in GR.minibatch(11, lp.cpu().numpy(), val.cpu().numpy()))
    one.update(obs, actions, old_lp, old_v, adv, ret)  # (the first call loads the kernels)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    _no_sync(lambda: one.update(obs, actions, old_lp, old_v, adv, ret))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before
    p, g, o, d, r = four._p, four._g, four._o, four._d, four._rows

    def separately():
        _capi.check(L.gd_policy_evaluate_dropout(C.byref(p), C.byref(g), C.byref(d), obs.data_ptr(), actions.data_ptr(),
                                                 r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), _stream()))
        _capi.check(L.gd_ppo_loss(C.byref(o), r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), old_lp.data_ptr(), old_v.data_ptr(),
                                  adv.data_ptr(), ret.data_ptr(), r[3].data_ptr(), r[4].data_ptr(), r[5].data_ptr(), _stream()))
        _capi.check(L.gd_policy_backward_dropout(C.byref(p), C.byref(g), C.byref(d), obs.data_ptr(), actions.data_ptr(),
                                                 r[3].data_ptr(), r[4].data_ptr(), r[5].data_ptr(), four.grad.data_ptr(), _stream()))
        _capi.check(L.gd_ppo_adam(C.byref(o), four.grad.data_ptr(), _stream()))

    for _ in range(2):
        _no_sync(separately)
    got, want = _state(one), _state(four)
    for k in got:
        assert _same(got[k], want[k]), (k, "gd_ppo_update_dropout differs from the four calls")
    assert r_one.call == r_four.call == 3 and int(one._used.item()) == int(four._used.item()) == 2
    assert one.nbytes == _ppo(None)[1].nbytes + 8, "the update's `used` word; the counter is the rule's"
    # the policy the optimiser stored into is the re-pack, under the same masks
    from gpudrive_lab_amd.policy import DevicePolicy
    fresh = DevicePolicy.from_state_dict(one.state_dict(), max_agents=A, ego_width=EW, dropout_rule=r_one)
    uni = torch.from_numpy(PC.uniforms(8, N)).cuda()
    logits = [torch.empty((N, NA), device="cuda") for _ in range(2)]
    r_one.seek(40)
    a = one.policy(obs, uni, logits_out=logits[0])
    r_one.seek(40)
    b = fresh(obs, uni, logits_out=logits[1])
    assert _same(logits[0], logits[1]) and all(_same(x, y) for x, y in zip(a, b)) and r_one.call == 41
    r_one.seek(41)
    one.policy(obs, uni, logits_out=logits[1])
    assert not _same(logits[0], logits[1])
