"""Host suite of the device rollout buffer: the numpy restatement (tests/ppo_reference.py) on hand-worked cases, the
prefix-sum permutation against Python's sorted, csrc/gae_chain.hpp run on the host against the serial loop, the argument
checks, and the C surface.  No device is touched."""
import os
import subprocess

import numpy as np
import pytest

from gpudrive_lab_amd import _capi
from tests import ppo_reference as PR
from tests import rollout_cases as RC
from tests.conftest import ROOT

F = np.float32


def test_gae_by_hand_with_a_done_in_the_middle():
    # gamma = 0.5, lambda = 0.5 (all products exact in binary): n = 4, done at t = 2
    d = np.array([0, 0, 1, 0], F)
    v = np.array([1, 2, 4, 8], F)
    r = np.array([0.5, 1, 2, 3], F)
    adv = PR.compute_gae(d, v, r, 0.5, 0.5)
    # t = 2: nnt = 1, delta = 3 + 0.5 * 8 - 4 = 3,  last = 3 + 0.25 * 0 = 3
    # t = 1: nnt = 0, delta = 2 + 0 - 2 = 0,        last = 0 + 0 * 3 = 0      (the done cuts the chain)
    # t = 0: nnt = 1, delta = 1 + 0.5 * 2 - 1 = 1,  last = 1 + 0.25 * 0 = 1
    assert adv.dtype == F and adv.tolist() == [1.0, 0.0, 3.0, 0.0]
    assert adv[-1] == 0
    # without the done the chain runs through: t = 1: delta = 2 + 0.5 * 4 - 2 = 2, last = 2 + 0.25 * 3 = 2.75;
    # t = 0: last = 1 + 0.25 * 2.75 = 1.6875
    assert PR.compute_gae(np.zeros(4, F), v, r, 0.5, 0.5).tolist() == [1.6875, 2.75, 3.0, 0.0]


def _store(ex, step, n, width, mask, action_shape=()):
    obs, value, action, logprob, reward, done, _ = RC.step_inputs(step, n, width, action_shape, "all")
    ex.store(obs, value, action, logprob, reward, done, range(n), mask)
    return obs


def test_a_truncated_last_step_keeps_the_lowest_live_rows():
    ex = PR.Experience(5, obs_width=3)
    _store(ex, 0, 4, 3, np.array([1, 0, 1, 1], bool))
    assert (ex.ptr, ex.step, ex.full) == (3, 1, False)
    obs = _store(ex, 1, 4, 3, np.array([0, 1, 1, 1], bool))
    assert (ex.ptr, ex.step, ex.full, ex.dropped) == (5, 2, True, 1)
    assert np.array_equal(ex.obs[3:], obs[[1, 2]])  # rows 1 and 2 of the live 1, 2, 3
    assert ex.sort_keys == [(0, 0), (2, 0), (3, 0), (1, 1), (2, 1)]
    assert ex.sort_training_data().tolist() == [0, 3, 1, 4, 2]
    assert (ex.ptr, ex.step, ex.sort_keys) == (0, 0, [])


def test_a_step_with_nothing_live_still_advances_step():
    ex = PR.Experience(4, obs_width=2)
    _store(ex, 0, 3, 2, np.zeros(3, bool))
    assert (ex.ptr, ex.step) == (0, 1)
    _store(ex, 1, 3, 2, np.array([0, 1, 0], bool))
    assert (ex.ptr, ex.step) == (1, 2) and ex.sort_keys == [(1, 1)]


def test_flatten_batch_layout():
    ex = PR.Experience(12, 4, 2, obs_width=1)
    for s in range(4):
        _store(ex, s, 3, 1, np.ones(3, bool))
    idxs = ex.sort_training_data()
    assert idxs.tolist() == [0, 3, 6, 9, 1, 4, 7, 10, 2, 5, 8, 11]
    adv = np.arange(12, dtype=F)
    b = ex.flatten_batch(adv)
    assert [x.shape for x in b] == [(3, 2, 2, 1), (3, 2, 2), (3, 2, 2), (3, 2, 2), (3, 4), (3, 4), (3, 4)]
    # minibatch mb, row r, step h <- sorted position (r * 3 + mb) * 2 + h
    assert ex.b_advantages[1].tolist() == [2, 3, 8, 9]
    assert np.array_equal(ex.b_values[1], ex.values[idxs[[2, 3, 8, 9]]])
    assert np.array_equal(ex.b_returns, ex.b_advantages + ex.b_values)


@pytest.mark.parametrize("seed", range(4))
def test_offset_plus_ordinal_is_the_sorted_order(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    keys, step = [], 0
    while len(keys) < 200:
        keys.extend((int(i), step) for i in np.where(rng.random(n) < rng.random())[0])
        step += 1
    want = sorted(range(len(keys)), key=keys.__getitem__)
    assert PR.offset_ord_permutation([k[0] for k in keys], n).tolist() == want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("pattern", RC.DONE_PATTERNS)
def test_chain_header_on_the_host_equals_the_serial_loop(n, pattern):
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        d, v, r = RC.gae_inputs(pattern, n, seed=n)
        cut, serial = RC.gae_host(d, v, r, gamma, lam)
        want = PR.compute_gae(d, v, r, gamma, lam)
        assert np.array_equal(serial.view(np.int32), want.view(np.int32))  # the C loop and the numpy loop: bits
        assert np.array_equal(cut, want)                                     # the cut form: values
        assert cut[-1] == 0


def test_arguments_are_checked_without_a_device():
    from gpudrive_lab_amd.rollout import DeviceRollout
    ok = dict(num_rows=5, obs_width=7)
    bad = [((24, 7, 1), ok), ((24, 8, 3), ok), ((0,), ok), ((24, 8, 0), ok), ((24.0,), ok), ((True,), ok),
           ((24,), dict(ok, num_rows=0)), ((24,), dict(ok, num_rows=(1 << 20) + 1)), ((24,), dict(ok, obs_width=0)),
           ((24,), dict(ok, obs_width=2.5)), ((24,), dict(ok, action_shape=(0,))), ((24,), dict(ok, action_shape=3)),
           ((24,), dict(ok, device="cpu")), ((24,), dict(ok, lstm=object())), ((24,), dict(ok, cpu_offload=True)),
           ((1 << 31,), ok), (((1 << 22) + 1,), ok), ((24,), dict(ok, gather_split=65)), ((24,), dict(ok, gather_split=1.0)),
           ((24,), dict(ok, storage=[])), ((24,), dict(ok, storage=dict(idxs=None)))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            DeviceRollout(*args, **kw)
    with pytest.raises(TypeError):
        DeviceRollout(24)  # num_rows and obs_width are required


def test_the_header_names_the_reference_and_the_symbols_are_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "gpudrive/integrations/puffer/ppo.py:530-666" in header and "ppo.py:606-620" in header
    new = {"gd_rollout_store", "gd_rollout_sort", "gd_rollout_gae", "gd_rollout_gather"}
    for name in new:
        assert "int %s(const gd_rollout *ro, " % name in header
    assert new <= set(_capi.SYMBOLS)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert new <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_rollout_store.argtypes) == 10 and len(L.gd_rollout_gather.argtypes) == 3
    import ctypes as C
    assert C.sizeof(_capi.GdRollout) == 16 + 11 * 8 and C.sizeof(_capi.GdRolloutBatch) == 16 + 24 + 7 * 8
    assert _capi.GdRolloutBatch.obs.offset == 40
    # a null table is refused on the host, before any launch
    assert L.gd_rollout_sort(None, None, None, None) == _capi.GD_ERR_INVALID
    ro = _capi.GdRollout()
    assert L.gd_rollout_gae(C.byref(ro), None, 0.99, 0.95, None, None, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_rollout_gae" in L.gd_last_error()
