"""GPU suite: the device policy forward (gpudrive_lab_amd.policy.DevicePolicy; gd_policy_forward) against the float64 numpy
reference (tests/policy_reference.py) on the seeded and constructed cases of tests/policy_cases.py.

Logits and value: the yardstick E of a case is the maximum absolute error of torch's own float32 CPU forward of the stand-in
module against the float64 reference on that case (logits and value together); the kernel's error must be <= 8 E.  The 8
covers another summation order over the 64-, 192- and 128-term dot products and OCML's tanh against libm's, and stays three
orders of magnitude below the >= 1e-2 of an indexing or masking error.  Actions, logprob and entropy are held to the rule
evaluated in float64 on the kernel's OWN logits: the deterministic action exactly, the sampled one to 1e-5 of the cumulative
softmax, logprob and entropy to (n_actions + 8) 2^-24 max(1, |x|) (an fp32 sum of n terms in [0, 1])."""
import contextlib

import numpy as np
import pytest
import torch

from tests import policy_cases as PC
from tests import policy_reference as REF
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

CANARY_BITS = 0x7FC0DEAD  # a NaN payload no kernel writes
GUARD = 64                # int32 words either side of every carved tensor


class Carver:
    """Tensors carved from canary-filled int32 buffers with GUARD words either side."""

    def __init__(self):
        self.whole = {}

    def carve(self, name, shape, dtype):
        words = int(np.prod(shape, dtype=np.int64)) * (2 if dtype == torch.int64 else 1)
        buf = torch.full((GUARD + words + GUARD,), CANARY_BITS, dtype=torch.int32, device="cuda")
        self.whole[name] = (buf, words)
        return buf[GUARD:GUARD + words].view(dtype).view(shape)

    def assert_guards_and_written(self, what):
        for name, (buf, words) in self.whole.items():
            h = buf.cpu().numpy()
            assert (h[:GUARD] == CANARY_BITS).all() and (h[GUARD + words:] == CANARY_BITS).all(), \
                "%s: bytes beside %s were written" % (what, name)
            if name != "actions":  # (an int64's high word is zero; its low word is checked as a value)
                assert (h[GUARD:GUARD + words] != CANARY_BITS).all(), "%s: %s was not written whole" % (what, name)

    def refill(self):
        for buf, _ in self.whole.values():
            buf.fill_(CANARY_BITS)


def _outputs(carver, n, na):
    f = torch.float32
    out = (carver.carve("actions", (n,), torch.int64), carver.carve("logprob", (n,), f), carver.carve("entropy", (n,), f),
           carver.carve("value", (n,), f))
    return out, carver.carve("logits", (n, na), f)


def _no_sync(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)


def _host(out):
    return [t.cpu().numpy().copy() for t in out]


def _bound(na, x):
    return (na + 8) * 2.0 ** -24 * np.maximum(1.0, np.abs(x))


def _check_rule(what, na, logits, u, det, actions, logprob, entropy):
    """actions / logprob / entropy against the float64 rule on the kernel's own logits."""
    n = len(logits)
    assert actions.dtype == np.int64 and (actions >= 0).all() and (actions < na).all(), what
    if det:
        assert np.array_equal(actions, logits.argmax(1)), what + ": not the first index of the maximum"
    else:
        c = REF.cumulative(logits)
        lo = np.where(actions > 0, c[np.arange(n), np.maximum(actions - 1, 0)], 0.0)
        hi = c[np.arange(n), actions]
        u64 = u.astype(np.float64)
        assert (lo - 1e-5 <= u64).all() and (u64 < hi + 1e-5).all(), what + ": the draw is not where u falls"
    l = logits.astype(np.float64)
    q = l - l.max(1, keepdims=True)
    q = q - np.log(np.exp(q).sum(1, keepdims=True))
    wlp, went = q[np.arange(n), actions], -(q * np.exp(q)).sum(1)
    assert (np.abs(logprob - wlp) <= _bound(na, wlp)).all(), (what, "logprob", np.abs(logprob - wlp).max())
    assert (np.abs(entropy - went) <= _bound(na, went)).all(), (what, "entropy", np.abs(entropy - went).max())


def _variants(sd, obs, a, ew):
    yield "seeded", sd, obs
    yield "negative_pool", PC.negative_pool_state(sd), obs              # (i)
    yield "last_entity_wins", sd, PC.last_entity_wins(sd, obs, a, ew)   # (ii)
    if sd["actor.bias"].shape[0] > 5:  # (iii) ties actions 3 and 5
        yield "tied_actor", PC.tied_actor_state(sd), obs


def _forward_case(n, a, ew, na, edge=False):
    """edge: a shape of PC.EDGE_SHAPES -- the value and the logits of the last tile are also judged on their own (same
    reference, same 8 E), so that a swapped or dropped last tile is named; with one action there is no second action to
    tie, and logprob and entropy are the host program's bits."""
    from gpudrive_lab_amd.policy import DevicePolicy
    sd0 = PC.state_dict(10 + na + ew, ew, na)
    obs0 = PC.observations(20 + n + a, n, a, ew)
    carver = Carver()
    out, logits_out = _outputs(carver, n, na)
    pol = None
    worst = 0.0
    for vi, (name, sd, obs) in enumerate(_variants(sd0, obs0, a, ew)):
        what = "%s n=%d A=%d ego=%d actions=%d" % (name, n, a, ew, na)
        want_l, want_v, _ = REF.forward(sd, obs, a, ew)
        t_l, t_v = PC.stand_in_forward(sd, obs, a, ew, torch.float32)
        E = max(np.abs(t_l - want_l).max(), np.abs(t_v - want_v).max())
        if pol is None:
            pol = DevicePolicy.from_state_dict(sd, max_agents=a, ego_width=ew)
        else:
            pol.load_state_dict({k: v.cuda() for k, v in sd.items()})  # new weights change the outputs to the new reference's
        d_obs = torch.from_numpy(obs).cuda()
        for ui, u in enumerate((PC.uniforms(n + vi, n), PC.edge_uniforms(n), None)):   # sampled, (iv), deterministic
            det = u is None
            d_u = None if det else torch.from_numpy(u).cuda()
            carver.refill()
            if ui == 0:
                pol(d_obs, d_u, out=out, logits_out=logits_out)  # (the first call of this N allocates the scratch)
            else:
                _no_sync(lambda: pol(d_obs, d_u, deterministic=det, out=out, logits_out=logits_out))
            carver.assert_guards_and_written(what)
            actions, logprob, entropy, value = _host(out)
            logits = logits_out.cpu().numpy().copy()
            err = max(np.abs(logits - want_l).max(), np.abs(value - want_v).max())
            if ui == 0:
                print("policy forward %s: E %.3g, kernel error %.3g, ratio %.2f" % (what, E, err, err / E))
            assert err <= 8 * E, (what, "error %.3g above 8 E = %.3g" % (err, 8 * E))
            worst = max(worst, err / E)
            if edge:
                _check_last_tile(what, na, logits, value, want_l, want_v, E)
                if na == 1:
                    _check_one_action(what, logits, u, det, actions, logprob, entropy)
            _check_rule(what + (" det" if det else " u%d" % ui), na, logits, u, det, actions, logprob, entropy)
            if name == "tied_actor" and det:
                assert (logits[:, 3] == logits[:, 5]).all() and (actions == 3).all(), what
            if ui == 1:
                assert (actions[u == 0] == 0).all(), what + ": u = 0 takes the first action"
    # without out=, fresh tensors carry the same values
    fresh = pol(d_obs, deterministic=True)
    for g, w in zip(_host(fresh), _host(out)):
        assert np.array_equal(g, w)
    return worst


def _check_last_tile(what, na, logits, value, want_l, want_v, E):
    """The value (output n_actions: alone in a tile of its own when n_actions is a multiple of 32) and the last 32-wide tile
    that holds logits, each against the float64 reference by the case's own yardstick."""
    assert E > 0, (what, "the float32 yardstick is degenerate")
    err_v = np.abs(value - want_v).max()
    assert err_v <= 8 * E, (what, "the value (output %d, tile %d): error %.3g above 8 E = %.3g" % (na, na // 32, err_v, 8 * E))
    lo = 32 * ((na - 1) // 32)
    err_l = np.abs(logits[:, lo:] - want_l[:, lo:]).max()
    assert err_l <= 8 * E, (what, "logits %d..%d (tile %d): error %.3g above 8 E = %.3g" % (lo, na - 1, lo // 32, err_l, 8 * E))


def _check_one_action(what, logits, u, det, actions, logprob, entropy):
    """A softmax of one number: expf(0) and logf(1) are exact on the device and on the host, so logprob and entropy are the
    host program's bits (a zero and a negative zero)."""
    n = len(logits)
    a, lp, ent = PC.run_rule_host(logits, np.zeros(n, np.float32) if det else u, det)
    assert np.array_equal(actions, a) and (actions == 0).all(), what
    assert np.array_equal(logprob.view(np.int32), lp.view(np.int32)), (what, "logprob is not the host program's bits", logprob)
    assert np.array_equal(entropy.view(np.int32), ent.view(np.int32)), (what, "entropy is not the host program's bits", entropy)


@pytest.mark.parametrize("n,a,ew,na", PC.SHAPES, ids=lambda v: str(v))
def test_forward_against_the_float64_reference(n, a, ew, na):
    _forward_case(n, a, ew, na)


@pytest.mark.parametrize("n,a,ew,na", PC.EDGE_SHAPES, ids=lambda v: str(v))
def test_forward_at_the_action_counts_where_the_tiling_changes(n, a, ew, na):
    worst = _forward_case(n, a, ew, na, edge=True)
    print("POLICY_EDGE forward n=%d A=%d ego=%d actions=%d: largest error / E %.2f (bound 8)" % (n, a, ew, na, worst))


def test_inputs_are_checked():
    from gpudrive_lab_amd.policy import DevicePolicy
    pol = DevicePolicy.from_state_dict(PC.state_dict(1, 6, 7), max_agents=64, ego_width=6)
    obs = torch.zeros((3, pol.obs_width), device="cuda")
    u = torch.zeros(3, device="cuda")
    bad = [((obs[:, :-1],), {}), ((obs.double(), u), {}), ((obs.t().contiguous().t(), u), {}), ((obs.cpu(), u.cpu()), {}),
           ((obs,), {}), ((obs, u[:2]), {}), ((obs, u.double()), {}), ((obs, u), dict(out=(u, u, u))),
           ((obs, u), dict(out=(u, u, u, u))), ((obs, u), dict(logits_out=torch.zeros((3, 8), device="cuda")))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            pol(*args, **kw)


@contextlib.contextmanager
def _side_stream():
    st = torch.cuda.Stream()  # the learner step is a captured graph: not on the legacy null stream
    with torch.cuda.stream(st):
        yield st


def test_in_the_learner_loop():
    """12 steps of DeviceLearnerEnv -> DevicePolicy -> DeviceRollout.store on the suite's small scenes with no host
    synchronisation; the stored logprobs, values and actions equal a second policy's recomputation from the stored
    observations, bit for bit."""
    from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table
    from gpudrive_lab_amd.policy import DevicePolicy
    from gpudrive_lab_amd.rollout import DeviceRollout
    from tests import parity as P
    params = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0,
                  dynamicsModel=0, isStaticAgentControlled=0, initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1,
                  roadObservationAlgorithm=1)
    sim = P.make_gpu_sim([TEST_JSON, SCENE_407, SCENE_4], max_agents=64, **params)
    try:
        with _side_stream():
            env = DeviceLearnerEnv(sim)
            n = env.num_agents
            obs = env.reset()
            na = action_table("classic").shape[0]
            sd = PC.state_dict(3, 6, na)
            assert n > 1 and int(obs.shape[1]) == PC.obs_width(64, 6)
            pol = DevicePolicy.from_state_dict(sd, max_agents=64, ego_width=6)
            steps = 12
            ro = DeviceRollout(steps * n, num_rows=n, obs_width=int(obs.shape[1]))
            gen = torch.Generator(device="cuda")
            gen.manual_seed(7)
            out = tuple(torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int64,) + (torch.float32,) * 3)
            obs, rewards, terminals, truncations, masks = env.step(torch.zeros(n, dtype=torch.int64, device="cuda"))
            pol(obs, torch.rand(n, device="cuda", generator=gen), out=out)  # (allocates the scratch of this N)
            us, live = [], []

            def loop():
                nonlocal obs, rewards, terminals, truncations, masks
                for _ in range(steps):
                    u = torch.rand(n, device="cuda", generator=gen)
                    actions, logprob, entropy, value = pol(obs, u, out=out)
                    ro.store(obs, value, actions, logprob, rewards, terminals, masks)
                    us.append(u)
                    live.append(masks.clone())
                    obs, rewards, terminals, truncations, masks = env.step(actions)

            _no_sync(loop)
            stored = int(ro.state[0].item())
            u_stored = torch.cat([u[m] for u, m in zip(us, live)]).contiguous()
            assert stored == u_stored.numel() and stored > n
            again = DevicePolicy.from_state_dict(sd, max_agents=64, ego_width=6)
            actions, logprob, entropy, value = again(ro.obs[:stored], u_stored)
            for name, got, want in (("actions", ro.actions[:stored], actions), ("logprobs", ro.logprobs[:stored], logprob),
                                    ("values", ro.values[:stored], value)):
                g, w = got.cpu().numpy(), want.cpu().numpy()
                assert np.array_equal(g.view(np.int32), w.view(np.int32)), "stored %s differ from the recomputation" % name
            assert np.isfinite(logprob.cpu().numpy()).all() and len(np.unique(actions.cpu().numpy())) > 1
    finally:
        sim.close()
