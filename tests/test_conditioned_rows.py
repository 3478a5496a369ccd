"""CPU tests of the conditioned learner rows (gd_attach_packed_rows_conditioned, ConditionedLearnerEnv): the export, the
argument checks, and the span arithmetic of store_span (csrc/pack_cols.hpp) that lets every writer of a row with the odd
pitch D + 3 store exactly its own dwords."""
import os
import subprocess

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd.learner import ConditionedLearnerEnv, DeviceLearnerEnv


def test_conditioned_rows_symbol_is_exported():
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "gd_attach_packed_rows_conditioned" in names
    assert "gd_attach_packed_rows_conditioned" in _capi.SYMBOLS
    assert len(_capi.lib().gd_attach_packed_rows_conditioned.argtypes) == 5


class _NoSim:
    """Stands in for a SimManager where the checks must fire before the simulator is touched."""

    def __getattr__(self, name):
        raise AssertionError("the simulator was touched (%s) before the arguments were checked" % name)


@pytest.mark.parametrize("kwargs,match", [
    (dict(condition_mode="sometimes"), "condition_mode"),
    (dict(condition_mode="preset", agent_type="reckless"), "agent_type"),
    (dict(condition_mode="preset"), "agent_type"),
    (dict(condition_mode="fixed", agent_type=torch.zeros(4)), "shape"),
    (dict(condition_mode="fixed", agent_type=torch.zeros(1, 3)), "shape"),
    (dict(condition_mode="fixed"), "agent_type"),
    (dict(action_table=torch.zeros(91, 2)), "action_table"),
    (dict(action_table=torch.zeros(0, 3)), "action_table"),
    (dict(action_table=np.zeros((91, 3))), "action_table"),
    (dict(init_steps=-1), "init_steps"),
    (dict(init_steps=91), "init_steps"),
    (dict(init_steps=1.5), "init_steps"),
    (dict(warmup="some_worlds"), "warmup"),
    (dict(reward_type="weighted_combination"), "reward_conditioned"),
    (dict(reward_type="distance_to_logs"), "reward_conditioned"),
    (dict(reward_weight_lb=(0.0, 1.0)), "three components"),
])
def test_conditioned_learner_env_checks_arguments_first(kwargs, match):
    with pytest.raises(ValueError, match=match):
        ConditionedLearnerEnv(_NoSim(), **kwargs)


def test_device_learner_env_still_refuses_reward_conditioned():
    with pytest.raises(ValueError, match="ConditionedLearnerEnv"):
        DeviceLearnerEnv(_NoSim(), reward_type="reward_conditioned")


def test_conditioned_learner_env_is_a_device_learner_env():
    assert issubclass(ConditionedLearnerEnv, DeviceLearnerEnv)
    for name in ("step", "reset", "resample", "pop_stats", "set_reward_weights", "reward_weights_tensor"):
        assert hasattr(ConditionedLearnerEnv, name), name


# ---- store_span (pack_cols.hpp), restated: dst's dword phase, the single dwords in front, the aligned 16-byte pieces,
# the single dwords behind; threads tid, tid + nt, ... ----
def store_span(mem, dst, src, nt):
    """Writes src into mem[dst:dst + len(src)] as store_span does; returns the list of (kind, first dword, width) stores."""
    n = len(src)
    phase = dst & 3
    head = min((4 - phase) & 3, n)
    body = (n - head) >> 2
    edge = n - body * 4
    stores = []
    for tid in range(nt):
        for q in range(tid, body, nt):
            at = dst + head + 4 * q
            assert at % 4 == 0, "a 16-byte store off its boundary"
            mem[at:at + 4] += 1
            stores.append(("b128", at, 4))
        for e in range(tid, edge, nt):
            k = e if e < head else e + body * 4
            mem[dst + k] += 1
            stores.append(("b32", dst + k, 1))
    return stores


@pytest.mark.parametrize("nt", [1, 4, 64, 256])
def test_store_span_writes_every_dword_once_and_nothing_else(nt):
    for phase in range(4):
        for n in range(1, 21):
            for base in (0, 64):  # (the base of the buffer itself is 16-byte aligned)
                mem = np.zeros(base + 64, np.int32)
                dst = base + 8 + phase
                stores = store_span(mem, dst, np.arange(n), nt)
                want = np.zeros_like(mem)
                want[dst:dst + n] = 1
                assert (mem == want).all(), (phase, n, nt)
                assert sum(1 for s in stores if s[0] == "b32") <= 6
                assert sum(1 for s in stores if s[0] == "b32") == n - 4 * sum(1 for s in stores if s[0] == "b128")


def test_conditioned_row_spans_cover_each_row_once():
    """The writers of a conditioned row own disjoint dwords: the head [r R, r R + 6 A + 3) in passes of 387 and 384 floats,
    the road block [r R + 6 A + 3, (r + 1) R) in passes of 64 x 13 floats; every row phase 0..3 occurs."""
    K = 200
    for A in (64, 128):
        D = 6 + (A - 1) * 6 + K * 13
        R = D + 3
        assert R % 2 == 1
        rows = 6
        mem = np.zeros(rows * R + 16, np.int32)
        phases = set()
        for r in range(rows):
            r0 = r * R
            phases.add(r0 % 4)
            for h in range(A // 64):  # packed_head
                store_span(mem, r0 + (0 if h == 0 else h * 384 + 3), np.zeros(387 if h == 0 else 384), 64)
            for p in range((K + 63) // 64):  # the road kernels' passes
                nrows = min(64, K - p * 64)
                store_span(mem, r0 + 6 * A + 3 + p * 64 * 13, np.zeros(nrows * 13), 64)
        assert phases == {0, 1, 2, 3}
        assert (mem[:rows * R] == 1).all() and (mem[rows * R:] == 0).all(), A
