"""CPU tests of the learner rows (gpudrive_lab_amd.learner, the new C exports): what can be checked without a device."""
import ctypes
import os
import subprocess
from itertools import product

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd.harness import default_action_values
from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table

NEW_SYMBOLS = ("gd_set_learner_rows", "gd_attach_packed_rows", "gd_set_discrete_actions")


def test_new_symbols_are_exported():
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in NEW_SYMBOLS:
        assert sym in names, sym
        assert sym in _capi.SYMBOLS, sym


def test_episode_buffers_append_the_flat_outputs():
    B = _capi.GdEpisodeBuffersRows
    assert [f[0] for f in B._fields_] == ["reward_rows", "terminal_rows", "truncated_rows", "mask_rows"]
    assert B.reward_rows.offset == 15 * 8 and B.mask_rows.offset == 18 * 8 and ctypes.sizeof(B) == 19 * 8
    b = B()  # zero: nothing is written through the rows
    assert b.reward_rows is None and b.mask_rows is None and b.controlled_mask is None
    # the entry points take the whole struct only
    L = _capi.lib()
    assert L.gd_episode_step.argtypes[2]._type_ is B and L.gd_episode_draw_weights.argtypes[2]._type_ is B


@pytest.mark.parametrize("model,n", [("classic", 91), ("bicycle", 91), ("delta_local", 8000)])
def test_action_table_order_and_values(model, n):
    t = action_table(model)
    assert t.dtype == torch.float32 and tuple(t.shape) == (n, 3)
    a1, a2, a3 = default_action_values(model)
    want = torch.tensor([[x.item(), y.item(), z.item()] for x, y, z in product(a1, a2, a3)], dtype=torch.float32)
    assert torch.equal(t, want)
    # index k = (i * len(a2) + j) * len(a3) + l
    i, j, l = 2, 5, len(a3) - 1
    k = (i * len(a2) + j) * len(a3) + l
    assert torch.equal(t[k], torch.stack([a1[i], a2[j], a3[l]]).to(torch.float32))


def test_action_table_refuses_state():
    with pytest.raises(ValueError):
        action_table("state")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_row_order_is_boolean_indexing_order(seed):
    rng = np.random.default_rng(seed)
    W, A = 5, 64
    mask = rng.random((W, A)) < 0.3
    mask[0] = False
    mask[-1] = True
    slot_of_row = np.flatnonzero(mask.reshape(-1))
    row_of_slot = np.full(W * A, -1)
    row_of_slot[slot_of_row] = np.arange(len(slot_of_row))
    x = torch.arange(W * A * 3, dtype=torch.float32).view(W, A, 3)
    got = x[torch.from_numpy(mask)]
    assert torch.equal(got, x.view(W * A, 3)[torch.from_numpy(slot_of_row)])
    assert (row_of_slot[slot_of_row] == np.arange(len(slot_of_row))).all()
    assert ((row_of_slot >= 0) == mask.reshape(-1)).all()


class _NoSim:
    """Stands in for a SimManager where the checks must fire before the simulator is touched."""

    def __getattr__(self, name):
        raise AssertionError("the simulator was touched (%s) before the arguments were checked" % name)


def test_device_learner_env_refuses_reward_conditioned():
    with pytest.raises(ValueError, match="reward_conditioned"):
        DeviceLearnerEnv(_NoSim(), reward_type="reward_conditioned")


@pytest.mark.parametrize("table", [torch.zeros(91, 2), torch.zeros(91, 4), torch.zeros(91), torch.zeros(0, 3),
                                   np.zeros((91, 3))])
def test_device_learner_env_refuses_a_bad_table(table):
    with pytest.raises(ValueError, match="action_table"):
        DeviceLearnerEnv(_NoSim(), action_table=table)
