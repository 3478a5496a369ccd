"""GPU suite: the device rollout buffer (gpudrive_lab_amd.rollout.DeviceRollout; gd_rollout_store / _sort / _gae / _gather)
against the numpy restatement of the reference's Experience and of the serial GAE loop (tests/ppo_reference.py).

Every comparison is bitwise (floats viewed as int32) except the advantages, which are compared as float32 values
(np.array_equal): csrc/gae_chain.hpp documents the two corner cases, both outside finite inputs' values, in which cutting the
chain at a done differs from the serial loop in a NaN or in the sign of a zero."""
import contextlib

import numpy as np
import pytest
import torch

from tests import ppo_reference as PR
from tests import rollout_cases as RC
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

CANARY_BITS = 0x7FC0DEAD  # a NaN payload no kernel writes
GUARD = 64                # int32 words either side of every carved tensor (16-byte pieces keep their alignment)
STORAGE = ("obs", "actions", "logprobs", "rewards", "dones", "values")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.itemsize == 1 else a.view(np.int32)


def _equal_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    x, y = _bits(got), _bits(want)
    if not np.array_equal(x, y):
        bad = np.argwhere(x != y)
        raise AssertionError("%s: %d words differ, first at %s" % (what, len(bad), bad[0].tolist()))


class Carver:
    """Tensors carved from canary-filled int32 buffers, with GUARD words (+ skew) in front and GUARD behind."""

    def __init__(self):
        self.whole = {}

    def carve(self, name, shape, dtype, skew=0):
        words = int(np.prod(shape, dtype=np.int64)) * (2 if dtype == torch.int64 else 1)
        if dtype == torch.int64:
            skew = 0  # (8-byte elements stay 8-byte aligned)
        buf = torch.full((GUARD + skew + words + GUARD,), CANARY_BITS, dtype=torch.int32, device="cuda")
        self.whole[name] = (buf, GUARD + skew, words)
        return buf[GUARD + skew:GUARD + skew + words].view(dtype).view(shape)

    def words(self, name):
        """(front guard, the tensor's words, back guard) on the host."""
        buf, lo, n = self.whole[name]
        h = buf.cpu().numpy()
        return h[:lo], h[lo:lo + n], h[lo + n:]

    def assert_guards(self, what):
        for name in self.whole:
            front, _, back = self.words(name)
            assert (front == CANARY_BITS).all() and (back == CANARY_BITS).all(), "%s: bytes beside %s were written" % (what, name)


def _carved_rollout(carver, skew, B, *args, **kw):
    """A DeviceRollout whose six storage tensors are carved from canary-filled buffers (`storage=`)."""
    from gpudrive_lab_amd.rollout import DeviceRollout
    shape = tuple(kw.get("action_shape", ()))
    spec = dict(obs=((B, kw["obs_width"]), torch.float32), actions=((B,) + shape, torch.int64), logprobs=((B,), torch.float32),
                rewards=((B,), torch.float32), dones=((B,), torch.float32), values=((B,), torch.float32))
    storage = {name: carver.carve(name, shp, dt, skew if name == "obs" else 0) for name, (shp, dt) in spec.items()}
    return DeviceRollout(B, *args, storage=storage, **kw)


def _dev(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _store_both(ro, ex, inputs, value_2d=False):
    """One step into the device buffer (no host synchronisation allowed) and into the restatement."""
    obs, value, action, logprob, reward, done, mask = inputs
    d = list(_dev(inputs))
    if value_2d:
        d[1] = d[1].view(-1, 1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ro.store(*d)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ex.store(obs, value, action, logprob, reward, done, range(len(mask)), mask)


def _check_storage(ro, ex, carver, what, canary_beyond=True):
    state = ro.state.cpu().numpy()
    assert state.tolist() == [ex.ptr, ex.step, ex.dropped, 0], (what, state.tolist(), (ex.ptr, ex.step, ex.dropped))
    for name in STORAGE:
        _, got, _ = carver.words(name)
        want = _bits(getattr(ex, name)).reshape(-1)
        per = want.size // ex.batch_size
        _equal_bits(got[:ex.ptr * per], want[:ex.ptr * per], "%s: %s[:ptr]" % (what, name))
        if canary_beyond:
            assert (got[ex.ptr * per:] == CANARY_BITS).all(), "%s: %s was written at or beyond ptr" % (what, name)
    carver.assert_guards(what)


KINDS = ("all", "none", "random", "random", "all")  # the mask of step s is KINDS[s % 5]


def _batch_size(n_rows, seed):
    """What the first four steps store and half of the fifth, whose rows are all live: the fifth step is truncated."""
    live = sum(int(RC.step_inputs(s, n_rows, 1, (), KINDS[s], seed=seed)[6].sum()) for s in range(4))
    return live + max(1, n_rows // 2)


STORE_CASES = [(n, w) for n in (1, 5, 70, 300) for w in (1, 4, 7, 1028, 2984, 2987)]


def _store_case(n_rows, width, streaming):
    k = STORE_CASES.index((n_rows, width))
    action_shape = (2,) if k % 2 else ()
    skew = 1 if (width == 4 and n_rows == 70) else 0  # once: rows of whole float4s at a pointer that is not 16-byte aligned
    B = _batch_size(n_rows, k)
    carver = Carver()
    ro = _carved_rollout(carver, skew, B, num_rows=n_rows, obs_width=width, action_shape=action_shape,
                         streaming_stores=streaming)
    assert ro.streaming_stores is streaming
    ex = PR.Experience(B, obs_width=width, action_shape=action_shape)
    _check_storage(ro, ex, carver, "empty")
    step = 0
    while not ex.full:
        assert not ro.full
        _store_both(ro, ex, RC.step_inputs(step, n_rows, width, action_shape, KINDS[step % len(KINDS)], seed=k),
                    value_2d=step % 2 == 1)
        step += 1
        _check_storage(ro, ex, carver, "step %d" % step)
        assert step < 64
    assert step == 5 and ro.full and int(ro.ptr.item()) == B and int(ro.step.item()) == step
    assert ex.dropped == n_rows - max(1, n_rows // 2) == int(ro.dropped.item())  # the last step was truncated
    assert ro.nbytes >= B * width * 4


@pytest.mark.parametrize("n_rows,width", STORE_CASES, ids=["N%d-w%d" % c for c in STORE_CASES])
def test_store_equals_the_restatement_after_every_step(n_rows, width):
    _store_case(n_rows, width, False)


# the non-temporal copy kernels: 16-byte pieces (2984), dwords (7, D + 3 = 2987, and 4 at a pointer that is not 16-byte aligned)
STREAMING_CASES = [(5, 4), (70, 4), (5, 7), (300, 2984), (70, 2987), (300, 2987)]


@pytest.mark.parametrize("n_rows,width", STREAMING_CASES, ids=["N%d-w%d" % c for c in STREAMING_CASES])
def test_store_with_streaming_stores_equals_the_restatement_after_every_step(n_rows, width):
    _store_case(n_rows, width, True)


def test_full_reads_the_device_only_once_the_host_bound_reaches_the_batch():
    from gpudrive_lab_amd.rollout import DeviceRollout
    n, B, w = 5, 23, 4
    ro = DeviceRollout(B, num_rows=n, obs_width=w)
    ex = PR.Experience(B, obs_width=w)
    for step in range(4):
        _store_both(ro, ex, RC.step_inputs(step, n, w, (), "random", seed=3))
        assert ro.full is False and ro.host_reads == 0
    step = 4
    while True:
        _store_both(ro, ex, RC.step_inputs(step, n, w, (), "random", seed=3))
        step += 1
        got = ro.full
        assert got == ex.full, step
        if step == 5:
            assert ro.host_reads == 1  # the bound has reached the batch (5 * 5 >= 23): the device is asked
        if got:
            break
        assert step < 64
    # (a read that finds ptr below the batch lowers the bound to it, so not every later answer needs one)
    assert ex.ptr == B and step > 5 and 2 <= ro.host_reads <= step - 4


def _fill(ro, ex, n_rows, width, action_shape, kind, seed):
    step = 0
    while not ex.full:
        _store_both(ro, ex, RC.step_inputs(step, n_rows, width, action_shape, kind, seed=seed))
        step += 1
    return step


def test_sort_equals_sorted_and_a_second_rollout_is_again_equal():
    n, B, w = 70, 1001, 7
    carver = Carver()
    ro = _carved_rollout(carver, 0, B, num_rows=n, obs_width=w)
    ex = PR.Experience(B, obs_width=w)
    _store_both(ro, ex, RC.step_inputs(0, n, w, (), "random", seed=5))
    with pytest.raises(RuntimeError):  # the host bound is below the batch
        ro.sort_training_data()
    for step in range(1, 15):          # the bound reaches the batch before the storage is full
        _store_both(ro, ex, RC.step_inputs(step, n, w, (), "random", seed=5))
    assert not ex.full
    with pytest.raises(RuntimeError):  # the device says so
        ro.sort_training_data()
    step = 15
    while not ex.full:
        _store_both(ro, ex, RC.step_inputs(step, n, w, (), "random", seed=5))
        step += 1
    for rollout in range(2):
        idxs = ro.sort_training_data()
        assert idxs.dtype == torch.int64 and idxs.is_cuda
        want = ex.sort_training_data()
        assert np.array_equal(idxs.cpu().numpy(), want), "rollout %d" % rollout
        assert ro.state.cpu().numpy().tolist() == [0, 0, ex.dropped, 0]
        assert int(ro._count.abs().sum().item()) == 0
        assert ro.full is False
        if rollout == 0:
            step = 0
            while not ex.full:
                _store_both(ro, ex, RC.step_inputs(100 + step, n, w, (), "random", seed=6))
                step += 1
                _check_storage(ro, ex, carver, "second rollout, step %d" % step, canary_beyond=False)
            assert ro.full


GAE_ROWS = 64


def _gae_rollout(B, d_sorted, v_sorted, r_sorted):
    """A full buffer of GAE_ROWS rows, all live, whose dones, values and rewards in SORTED order are the given ones."""
    from gpudrive_lab_amd.rollout import DeviceRollout
    n = GAE_ROWS
    steps = -(-B // n)
    dry = PR.Experience(B, obs_width=1)
    z = np.zeros(n, np.float32)
    for s in range(steps):
        dry.store(np.zeros((n, 1), np.float32), z, np.zeros(n, np.int64), z, z, z, range(n), np.ones(n, bool))
    idxs = dry.sort_training_data()
    stored = {}
    for name, x in (("d", d_sorted), ("v", v_sorted), ("r", r_sorted)):
        a = np.zeros(steps * n, np.float32)
        a[idxs] = x
        stored[name] = a.reshape(steps, n)
    ro = DeviceRollout(B, num_rows=n, obs_width=1)
    ex = PR.Experience(B, obs_width=1)
    for s in range(steps):
        obs = np.full((n, 1), s, np.float32)
        _store_both(ro, ex, (obs, stored["v"][s], np.zeros(n, np.int64), z, stored["r"][s], stored["d"][s] != 0, np.ones(n, bool)))
    return ro, ex


GAE_CASES = [(b, p) for b in (2, 64, 65, 4096) for p in RC.DONE_PATTERNS]


@pytest.mark.parametrize("B,pattern", GAE_CASES, ids=["B%d-%s" % c for c in GAE_CASES])
def test_gae_equals_the_serial_loop(B, pattern):
    d, v, r = RC.gae_inputs(pattern, B, seed=B)
    ro, ex = _gae_rollout(B, d, v, r)
    with pytest.raises(RuntimeError):
        ro.compute_gae(0.99, 0.95)  # before the sort
    assert ro.full
    idxs = ro.sort_training_data().cpu().numpy()
    want_idxs = ex.sort_training_data()
    assert np.array_equal(idxs, want_idxs)
    _equal_bits(ex.dones[want_idxs], d, "the construction: dones in sorted order")
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        adv = ro.compute_gae(gamma, lam)
        assert adv.dtype == torch.float32 and tuple(adv.shape) == (B,)
        want = PR.compute_gae(ex.dones[want_idxs], ex.values[want_idxs], ex.rewards[want_idxs], gamma, lam)
        got = adv.cpu().numpy()
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), (gamma, lam, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    assert int(ro.bad_positions.item()) == 0


GATHER_CASES = [(24, 8, 2, 5, "random"), (24, 24, 1, 5, "random"), (4096, 1024, 1, 512, "all")]


@pytest.mark.parametrize("split", [0, 1, 3])  # workgroups per sample: the default, one, and one that divides neither width
@pytest.mark.parametrize("width", [7, 2984])
@pytest.mark.parametrize("B,mbs,bptt,n_rows,kind", GATHER_CASES, ids=["B%d-mb%d-h%d" % c[:3] for c in GATHER_CASES])
def test_minibatches_and_flatten_batch_equal_the_restatement(B, mbs, bptt, n_rows, kind, width, split):
    from gpudrive_lab_amd.rollout import DeviceRollout
    action_shape = (2,) if width == 7 else ()
    ro = DeviceRollout(B, mbs, bptt, num_rows=n_rows, obs_width=width, action_shape=action_shape, gather_split=split)
    assert ro.gather_split == split
    ex = PR.Experience(B, mbs, bptt, obs_width=width, action_shape=action_shape)
    _fill(ro, ex, n_rows, width, action_shape, kind, seed=11)
    with pytest.raises(RuntimeError):
        ro.minibatch(0)  # before the sort and the advantages
    assert ro.full
    idxs = ro.sort_training_data()
    want_idxs = ex.sort_training_data()
    assert np.array_equal(idxs.cpu().numpy(), want_idxs)
    adv = ro.compute_gae(0.99, 0.95).cpu().numpy()
    want_adv = PR.compute_gae(ex.dones[want_idxs], ex.values[want_idxs], ex.rewards[want_idxs], 0.99, 0.95)
    assert np.array_equal(adv, want_adv)
    # (the outputs below carry the device's advantages: equal in value to the serial loop's, compared with them in bits)
    want = ex.flatten_batch(adv)
    names = DeviceRollout.OUT_NAMES
    assert ro.num_minibatches == B // mbs
    for mb in range(ro.num_minibatches):
        got = ro.minibatch(mb)
        for name, g, w in zip(names, got, want):
            _equal_bits(g.cpu().numpy(), w[mb], "minibatch %d %s" % (mb, name))
    flat = ro.flatten_batch()
    for name, g, w in zip(names, flat, want):
        _equal_bits(g.cpu().numpy(), w, "flatten_batch %s" % name)
        assert getattr(ro, "b_" + name) is g
    # out=: carved from canary-filled memory, fully written, nothing outside touched
    carver = Carver()
    out = tuple(carver.carve(name, shape, dt) for name, (shape, dt) in zip(names, ro.batch_shapes()))
    mb = ro.num_minibatches - 1
    back = ro.minibatch(mb, out=out)
    assert all(a is b for a, b in zip(back, out))
    for name, g, w in zip(names, out, want):
        _equal_bits(g.cpu().numpy(), w[mb], "minibatch out= %s" % name)
    carver.assert_guards("minibatch out=")
    with pytest.raises(ValueError):
        ro.minibatch(ro.num_minibatches)
    with pytest.raises(ValueError):
        ro.minibatch(0, out=out[:6])
    assert int(ro.bad_positions.item()) == 0


@contextlib.contextmanager
def _side_stream():
    st = torch.cuda.Stream()  # the learner step is a captured graph: not on the legacy null stream
    with torch.cuda.stream(st):
        yield st


@pytest.mark.parametrize("conditioned", [False, True], ids=["learner", "conditioned"])
def test_in_the_learner_loop(conditioned):
    """store, then step, with DeviceLearnerEnv ([N, D]) and ConditionedLearnerEnv ([N, D + 3]) on the suite's small scenes;
    a twin restatement is fed host copies taken at the same points."""
    from gpudrive_lab_amd.learner import ConditionedLearnerEnv, DeviceLearnerEnv, action_table
    from gpudrive_lab_amd.rollout import DeviceRollout
    from tests import parity as P
    params = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0,
                  dynamicsModel=0, isStaticAgentControlled=0, initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1,
                  roadObservationAlgorithm=1)
    sim = P.make_gpu_sim([TEST_JSON, SCENE_407, SCENE_4], max_agents=64, **params)
    try:
        with _side_stream():
            env = (ConditionedLearnerEnv if conditioned else DeviceLearnerEnv)(sim, init_steps=60)
            n = env.num_agents
            obs = env.reset()
            width = int(obs.shape[1])
            assert n > 1 and width == 2984 + (3 if conditioned else 0)
            n_actions = action_table("classic").shape[0]
            B = 40 * n + 3  # at least 41 steps: the 31 left of the episode after the warm-up, and the worlds' reset
            ro = DeviceRollout(B, num_rows=n, obs_width=width)
            ex = PR.Experience(B, obs_width=width)
            rows = torch.arange(n, device="cuda")
            step, saw_dead, saw_done = 0, False, False
            obs, rewards, terminals, truncations, masks = env.step((rows * 3) % n_actions)
            while not ro.full:
                # the stand-in policy: actions from (row, step), value and logprob from the observation's first columns
                action = (rows * 7 + step * 13) % n_actions
                value = (obs[:, 0] * 0.5 + obs[:, 1]).view(-1, 1)
                logprob = -(obs[:, 2].abs())
                ro.store(obs, value, action, logprob, rewards, terminals, masks)
                host = [t.cpu().numpy().copy() for t in (obs, value, action, logprob, rewards, terminals, masks)]
                obs, rewards, terminals, truncations, masks = env.step(action)
                ex.store(*host[:6], range(n), host[6])
                saw_dead |= not host[6].all()
                saw_done |= bool((host[5] & host[6]).any())
                step += 1
                assert step < 400
            assert ex.full and step >= 41
            # What this run is certain to cover is the end of the episode: after the 60 warm-up steps 31 are left, every
            # live agent is terminal there and its done is stored, and the worlds reset inside the rollout.  A mask goes
            # false only where an agent finishes BEFORE its world does (a collision under AgentStop, or its goal), which
            # depends on where the stand-in actions drive it and is not guaranteed by construction; it is reported, and
            # stores with dead rows are held to the restatement by the store tests' "none" and "random" masks.
            print("in the loop: %d rows, %d steps, masks went false: %s, dropped %d" % (n, step, saw_dead, ex.dropped))
            assert saw_done, "the rollout must cover the end of the episode: no done was stored"
            assert ro.state.cpu().numpy().tolist() == [ex.ptr, ex.step, ex.dropped, 0]
            for name in STORAGE:
                _equal_bits(getattr(ro, name).cpu().numpy(), getattr(ex, name), "storage %s" % name)
            idxs = ro.sort_training_data().cpu().numpy()
            want_idxs = ex.sort_training_data()
            assert np.array_equal(idxs, want_idxs)
            adv = ro.compute_gae(0.99, 0.95).cpu().numpy()
            want_adv = PR.compute_gae(ex.dones[want_idxs], ex.values[want_idxs], ex.rewards[want_idxs], 0.99, 0.95)
            assert np.array_equal(adv, want_adv)
            want = ex.flatten_batch(adv)
            for name, g, w in zip(DeviceRollout.OUT_NAMES, ro.minibatch(0), want):
                _equal_bits(g.cpu().numpy(), w[0], "minibatch %s" % name)
            assert int(ro.bad_positions.item()) == 0
    finally:
        sim.close()
