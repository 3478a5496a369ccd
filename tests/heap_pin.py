"""Runs tests/heap_pin.cpp (knn.hpp's loop on libstdc++'s heap functions) and turns its road order into the rows
agent_roadmap_tensor must hold.  Shared by the CPU suite (oracle vs libstdc++) and the GPU suite (HIP path vs libstdc++)."""
import hashlib
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_BIN = None


def binary():
    """The program built from heap_pin.cpp, named after the source's contents: a binary another version of the source left in
    the temporary directory is never taken for this one's, whatever the files' dates say.  (One small binary per version of the source stays behind there.)"""
    global _BIN
    if _BIN is None:
        src = os.path.join(HERE, "heap_pin.cpp")
        with open(src, "rb") as f:
            stamp = hashlib.sha256(f.read()).hexdigest()[:16]
        out = os.path.join(tempfile.gettempdir(), "gd_heap_pin_%d_%s" % (os.getuid(), stamp))
        if not os.path.exists(out):
            tmp = "%s.%d" % (out, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
            os.replace(tmp, out)
        _BIN = out
    return _BIN


def libstdcxx_order(keys, radius, K=200):
    """Road index per output slot (-1 = zero-filled) for one agent's key sequence."""
    keys = np.ascontiguousarray(keys, np.float32)
    blob = struct.pack("<iif", K, len(keys), float(radius)) + keys.tobytes()
    out = subprocess.run([binary()], input=blob, stdout=subprocess.PIPE, check=True).stdout
    return np.frombuffer(out, np.int32).copy()


def libstdcxx_order_f64(keys, radius, K=200):
    """The same run on float64 keys: (road index per output slot, the smallest gap between unequal keys over the comparisons
    the run performed -- |a - b| / (max(a, b) + 1), inf when it compared none)."""
    keys = np.ascontiguousarray(keys, np.float64)
    blob = struct.pack("<iid", K, len(keys), float(radius)) + keys.tobytes()
    out = subprocess.run([binary(), "f64"], input=blob, stdout=subprocess.PIPE, check=True).stdout
    assert len(out) == 4 * K + 8, len(out)
    return np.frombuffer(out[:4 * K], np.int32).copy(), float(np.frombuffer(out[4 * K:], np.float64)[0])


def expected_rows(orc, w, a, radius, K=200):
    """agent_roadmap rows of agent (w, a) as the libstdc++ run orders them: the oracle's observationOf of every road
    (position keys in float32, x*x + y*y like Vector2::length2) -> order -> rows; zero-filled rows are fillZeros
    (id 0, mapType 0: knn.hpp:19-28)."""
    obs = orc.road_obs_of(w, a)
    keys = obs[:, 0] * obs[:, 0] + obs[:, 1] * obs[:, 1]  # float32 arithmetic, no contraction
    order = libstdcxx_order(keys, radius, K)
    rows = np.zeros((K, 9), np.float32)
    sel = order >= 0
    rows[sel] = obs[order[sel]]
    return rows, order, keys
