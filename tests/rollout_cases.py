"""Inputs shared by tests/test_rollout.py (host) and tests/test_gpu_rollout.py (device): the done patterns of the GAE tests,
the host program around csrc/gae_chain.hpp, and step inputs whose observations are distinct per (row, step, column)."""
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DONE_PATTERNS = ("none", "every", "first", "last", "first_and_last", "p0.1", "p0.5")
_BIN = None


def dones_of(pattern, n, seed=0):
    d = np.zeros(n, np.float32)
    if pattern == "every":
        d[:] = 1
    elif pattern in ("first", "first_and_last"):
        d[0] = 1
    if pattern in ("last", "first_and_last"):
        d[-1] = 1
    if pattern.startswith("p"):
        d[:] = np.random.default_rng(seed).random(n) < float(pattern[1:])
    return d


def gae_inputs(pattern, n, seed=0):
    """(dones, values, rewards): finite, |x| < 10."""
    rng = np.random.default_rng(1000 + seed)
    v = rng.uniform(-9.9, 9.9, n).astype(np.float32)
    r = rng.uniform(-9.9, 9.9, n).astype(np.float32)
    return dones_of(pattern, n, seed), v, r


def gae_binary():
    global _BIN
    if _BIN is None:
        out = os.path.join(tempfile.gettempdir(), "gd_gae_chain_host_%d" % os.getuid())
        src = os.path.join(HERE, "gae_chain_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "gae_chain.hpp")
        ser = os.path.join(HERE, "gae_serial.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, (src, hdr, ser))):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, src])
        _BIN = out
    return _BIN


def gae_host(d, v, r, gamma, gae_lambda):
    """(cut form, serial loop) of the host program, float32 [n] each."""
    n = len(d)
    blob = struct.pack("<iff", n, float(np.float32(gamma)), float(np.float32(gae_lambda)))
    blob += b"".join(np.ascontiguousarray(a, np.float32).tobytes() for a in (d, v, r))
    out = subprocess.run([gae_binary()], input=blob, stdout=subprocess.PIPE, check=True).stdout
    both = np.frombuffer(out, np.float32).copy()
    assert both.size == 2 * n
    return both[:n], both[n:]


def step_inputs(step, n_rows, width, action_shape, mask_kind, seed=0):
    """One step's (obs, value, action, logprob, reward, done, mask) as numpy arrays.  obs[i, c] is an integer below 2^24
    distinct per (row, step, column) for the sizes the tests use, so a misplaced or partly copied row shows."""
    rng = np.random.default_rng(seed * 7919 + step)
    i = np.arange(n_rows, dtype=np.int64)[:, None]
    c = np.arange(width, dtype=np.int64)[None, :]
    obs = ((step * n_rows + i) * width + c) % (1 << 24)
    obs = obs.astype(np.float32)
    value = ((i[:, 0] * 31 + step * 7) % 1999).astype(np.float32) / np.float32(100.0) - np.float32(9.9)
    logprob = -((i[:, 0] * 13 + step * 3) % 997).astype(np.float32) / np.float32(128.0)
    reward = ((i[:, 0] * 5 + step * 11) % 401).astype(np.float32) / np.float32(64.0) - np.float32(3.0)
    aw = int(np.prod(action_shape)) if action_shape else 1
    action = ((i * 17 + step * 91) * aw + np.arange(aw)[None, :]).reshape((n_rows,) + tuple(action_shape)).astype(np.int64)
    done = rng.random(n_rows) < 0.2
    if mask_kind == "all":
        mask = np.ones(n_rows, bool)
    elif mask_kind == "none":
        mask = np.zeros(n_rows, bool)
    else:
        mask = rng.random(n_rows) < 0.6
    return obs, value, action, logprob, reward, done, mask
