"""Host suite of the device policy forward: the argument checks, the C surface, csrc/policy_rule.hpp run on the host against
the float64 rule, the float64 reference against a stand-in torch module, and the packed weight blob read the way the kernels
read it (an emulation of the MFMA lane maps in numpy).  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import policy_cases as PC
from tests import policy_reference as REF
from tests.conftest import ROOT


def _sd(ego_width=6, n_actions=91, seed=1):
    return PC.state_dict(seed, ego_width, n_actions)


def test_arguments_are_checked_without_a_device():
    from gpudrive_lab_amd.policy import DevicePolicy, check_policy_args
    assert check_policy_args(_sd(), 128, 6) == 91 and check_policy_args(_sd(9, 7), 64, 9) == 7
    assert check_policy_args(_sd(6, 1024), 128, 6) == 1024

    def drop(sd, key):
        sd = dict(sd)
        del sd[key]
        return sd

    def put(sd, key, value):
        return dict(sd, **{key: value})

    sd = _sd()
    wide = PC.state_dict(2, 6, 91)
    wide = put(put(wide, "shared_embed.0.weight", torch.zeros(256, 192)), "shared_embed.0.bias", torch.zeros(256))
    bad = [
        (sd, dict(max_agents=32)), (sd, dict(max_agents=128.0)), (sd, dict(ego_width=7)), (sd, dict(ego_width=True)),
        (sd, dict(act_func="gelu")), (sd, dict(vbd_in_obs=True)), (sd, dict(device="cpu")),
        (_sd(9), dict(ego_width=6)),                                    # the 9-column ego block under ego_width 6
        (_sd(6, 8000), {}),                                             # the 8000-entry delta table
        (put(sd, "actor.weight", torch.zeros(0, 128)), {}),
        (drop(sd, "critic.bias"), {}), (drop(sd, "actor.weight"), {}), (drop(sd, "road_map_embed.1.weight"), {}),
        (put(sd, "vbd_embed.0.weight", torch.zeros(64, 455)), {}),      # an extra key: the vbd embedder
        (put(sd, "partner_embed.0.weight", torch.zeros(64, 7)), {}),
        (put(sd, "ego_embed.4.weight", torch.zeros(32, 64)), {}),       # input_dim 32
        (wide, {}),                                                     # hidden_dim 256
        (put(sd, "actor.bias", sd["actor.bias"].double()), {}),
        (put(sd, "road_map_embed.4.weight", sd["road_map_embed.4.weight"].t()), {}),   # not contiguous
        (put(sd, "critic.weight", sd["critic.weight"].numpy()), {}),
        ([1, 2, 3], {}), (None, {}),
    ]
    for state, kw in bad:
        with pytest.raises(ValueError):
            DevicePolicy.from_state_dict(state, **dict(dict(max_agents=128, ego_width=6), **kw))


def test_the_header_declares_the_entry_point_and_null_is_refused():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "int gd_policy_forward(const gd_policy *p, " in header and "typedef struct gd_policy {" in header
    assert "gpudrive/networks/late_fusion.py:170-210" in header and "csrc/policy_rule.hpp" in header
    assert "gd_policy_forward" in _capi.SYMBOLS
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "gd_policy_forward" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_policy_forward.argtypes) == 10 and C.sizeof(_capi.GdPolicy) == 16 + 4 * 8
    assert L.gd_policy_forward(None, None, None, 0, None, None, None, None, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_policy_forward" in L.gd_last_error()


def test_the_blob_has_the_size_the_library_expects():
    """Nothing is launched: with the right size the call gets as far as the alignment check of `actions` (made misaligned
    here on purpose), with any other size it stops at the size."""
    from gpudrive_lab_amd.policy import pack_index
    L = _capi.lib()
    for ew, na in ((6, 91), (9, 7), (6, 1), (9, 1024), (6, 31), (6, 32)):
        p = _capi.GdPolicy()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = 3, 64, ew, na
        p.blob = p.features = p.logits = 0x1000
        args = (0x1000, 0x1000, 0, 0x1004, 0x1000, 0x1000, 0x1000, None, None)
        p.blob_floats = len(pack_index(ew, na))
        assert L.gd_policy_forward(C.byref(p), *args) == _capi.GD_ERR_INVALID and b"8-byte aligned" in L.gd_last_error()
        p.blob_floats += 1
        assert L.gd_policy_forward(C.byref(p), *args) == _capi.GD_ERR_INVALID and b"blob_floats" in L.gd_last_error()


# ---- the action rule

def _rule_cases():
    rng = np.random.default_rng(5)
    for na in (91, 7, 1, 1024) + tuple(k for k in PC.EDGE_ACTIONS if k not in (1, 1024)):
        logits = (rng.normal(0.0, 2.0, (40, na))).astype(np.float32)
        logits[0] = 0.0                      # a uniform row: every logit is the maximum
        if na > 5:
            logits[1, 5] = logits[1, 3] = logits[1].max() + 1  # two equal maxima
        yield na, logits


@pytest.mark.parametrize("na,logits", list(_rule_cases()), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_rule_header_on_the_host_equals_the_float64_rule(na, logits):
    n = len(logits)
    bound = lambda x: (na + 8) * 2.0 ** -24 * np.maximum(1.0, np.abs(x))  # noqa: E731  an fp32 sum of na terms in [0, 1]
    for u in (PC.clear_of_boundaries(logits, PC.uniforms(na, n)), PC.edge_uniforms(n)):
        for det in (False, True):
            a, lp, ent = PC.run_rule_host(logits, u, det)
            wa, wlp, went = REF.action_rule(logits, u, det)
            assert np.array_equal(a, wa), (det, np.argwhere(a != wa)[:4].tolist())
            assert (np.abs(lp - wlp) <= bound(wlp)).all() and (np.abs(ent - went) <= bound(went)).all()
            if det and na > 5:
                assert a[1] == 3 and a[0] == 0  # the first index of the maximum
    # u = 0 takes the first action with any mass, the largest u below 1 the last
    a, _, _ = PC.run_rule_host(logits, PC.edge_uniforms(n), False)
    assert (a[0::2] == 0).all() and (a[1::2] == na - 1).all()


def test_rule_host_program_under_the_sanitizers_at_the_edge_action_counts():
    """The same program as a stand-alone executable built with -fsanitize=address,undefined: it must exit cleanly and give the
    plain build's bits, at one action, at the counts around a tile of 32 and at 1024."""
    rng = np.random.default_rng(7)
    for na in PC.EDGE_ACTIONS:
        logits = rng.normal(0.0, 2.0, (5, na)).astype(np.float32)
        for u, det in ((PC.uniforms(na, 5), False), (PC.edge_uniforms(5), False), (PC.uniforms(na, 5), True)):
            plain, san = PC.run_rule_host(logits, u, det), PC.run_rule_host(logits, u, det, sanitize=True)
            assert np.array_equal(plain[0], san[0]), na
            assert all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(plain[1:], san[1:])), na
        if na == 1:
            assert (plain[0] == 0).all() and (plain[1].view(np.int32) == 0).all() and (plain[2] == 0).all()


# ---- the reference

@pytest.mark.parametrize("max_agents,ego_width,n_actions", [(64, 6, 91), (128, 9, 7)])
def test_reference_equals_the_stand_in_module_in_float64(max_agents, ego_width, n_actions):
    sd = _sd(ego_width, n_actions)
    obs = PC.observations(3, 5, max_agents, ego_width)
    logits, value, _ = REF.forward(sd, obs, max_agents, ego_width)
    tl, tv = PC.stand_in_forward(sd, obs, max_agents, ego_width, torch.float64)
    assert np.abs(logits).max() > 1.0                      # logits spread over several units
    assert np.abs(logits - tl).max() < 1e-12 and np.abs(value - tv).max() < 1e-12
    # and the stand-in carries exactly the keys the policy accepts
    from gpudrive_lab_amd.policy import expected_shapes
    net = PC.StandIn(max_agents, ego_width, n_actions)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == expected_shapes(ego_width, n_actions)


def test_constructed_cases_are_what_they_claim():
    sd = _sd(6, 7)
    obs = PC.observations(4, 3, 64, 6)
    _, _, feat = REF.forward(PC.negative_pool_state(sd), obs, 64, 6)
    assert (feat < 0).all()                                                       # (i)
    obs2 = PC.last_entity_wins(sd, obs, 64, 6)                                    # (ii) asserts its own claim
    assert not np.array_equal(obs, obs2)
    logits, _, _ = REF.forward(PC.tied_actor_state(sd), obs, 64, 6)               # (iii)
    assert (logits[:, 3] == logits[:, 5]).all() and (logits.argmax(1) == 3).all()


# ---- the blob, read as the kernels read it

def _acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


_ROWS = np.array([[_acc_row(r, lane >> 5) for lane in range(64)] for r in range(16)])  # [r][lane]
_COLS = np.arange(64) & 31


def _mfma(a, b, acc):
    """v_mfma_f32_32x32x2_f32 on per-lane operands: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]; register r of lane l
    is D[acc_row(r, l >> 5)][l & 31]."""
    d = np.einsum("ki,kj->ij", a.reshape(2, 32), b.reshape(2, 32))
    return acc + d[_ROWS, _COLS[None, :]]


def _emulate(blob, obs, max_agents, ew, na):
    """policy.hip's data flow in float64 from the packed blob: (logits, value)."""
    lane = np.arange(64)
    h, c = lane >> 5, lane & 31
    o = [0]

    def take(n):
        o[0] += n
        return blob[o[0] - n:o[0]].astype(np.float64)

    n = obs.shape[0]
    feat = np.zeros((n, 192))
    w1, b1, g, b, w2t, b2 = take(64 * ew).reshape(64, ew), take(64), take(64), take(64), take(4096).reshape(64, 64), take(64)

    def ln_tanh(x, g, b, axis):
        mean = x.mean(axis, keepdims=True)
        var = ((x - mean) ** 2).mean(axis, keepdims=True)
        return np.tanh((x - mean) / np.sqrt(var + 1e-5) * g + b)

    feat[:, :64] = ln_tanh(obs[:, :ew] @ w1.T + b1, g, b, 1) @ w2t + b2
    base = ew
    for e, (k, ks, count) in enumerate(((6, 3, max_agents - 1), (13, 7, 200))):
        w1a, b1, g, b = take(2 * ks * 64).reshape(2, ks, 64), take(64), take(64), take(64)
        w2a, b2 = take(2 * 32 * 64).reshape(2, 32, 64), take(64)
        frow = np.stack([32 * t + _ROWS for t in range(2)])  # [t][r][lane]: the feature a register holds
        for i in range(n):
            x = obs[i, base:base + k * count].astype(np.float64)
            best = np.full((2, 16, 64), -np.inf)
            for lo in range(0, count, 32):
                ent = lo + c
                live = ent < count
                acc = b1[frow].copy()
                for s in range(ks):
                    col = ks * h + s
                    ok = live & (col < k)
                    xs = np.where(ok, x[np.where(ok, ent * k + col, 0)], 0.0)
                    for t in range(2):
                        acc[t] = _mfma(w1a[t, s], xs, acc[t])
                both = np.concatenate([acc.reshape(32, 64)[:, :32], acc.reshape(32, 64)[:, 32:]], 0)  # the two lane halves
                mean, var = both.mean(0), both.var(0)
                mean, var = np.tile(mean, 2), np.tile(var, 2)
                acc = np.tanh((acc - mean) / np.sqrt(var + 1e-5) * g[frow] + b[frow])
                out = np.zeros((2, 16, 64))
                for t2 in range(2):
                    for t in range(2):
                        for r in range(16):
                            out[t2] = _mfma(w2a[t2, t * 16 + r], acc[t, r], out[t2])
                best = np.where(live[None, None, :], np.maximum(best, out), best)
            for t in range(2):
                for r in range(16):
                    for hh in range(2):
                        f = 32 * t + _acc_row(r, hh)
                        feat[i, 64 + 64 * e + f] = best[t, r, 32 * hh:32 * hh + 32].max() + b2[f]
        base += k * count
    shw, shb = take(4 * 96 * 64).reshape(4, 96, 64), take(128)
    tiles = (na + 1 + 31) // 32
    acw, acb = take(tiles * 64 * 64).reshape(tiles, 64, 64), take(tiles * 32)
    assert o[0] == len(blob)
    logits, value = np.zeros((n, na)), np.zeros(n)
    for blk in range(0, n, 32):
        row = np.minimum(blk + c, n - 1)
        hid = np.stack([shb[32 * t + _ROWS] for t in range(4)])
        for s in range(96):
            v = feat[row, 96 * h + s]
            for t in range(4):
                hid[t] = _mfma(shw[t, s], v, hid[t])
        for i in range(tiles):
            acc = np.zeros((16, 64))
            for t in range(4):
                for r in range(16):
                    acc = _mfma(acw[i, t * 16 + r], hid[t, r], acc)
            for r in range(16):
                for ln in range(64):
                    a, rw = 32 * i + _ROWS[r, ln], blk + (ln & 31)
                    if rw < n:
                        if a < na:
                            logits[rw, a] = acc[r, ln] + acb[a]
                        elif a == na:
                            value[rw] = acc[r, ln] + acb[a]
    return logits, value


# ... and at the action counts where the number of head tiles or the value's place in its tile changes (PC.EDGE_SHAPES)
_LANE_CASES = [(64, 9, 7, 2), (128, 6, 91, 1), (64, 6, 33, 34),
               (64, 6, 1, 3), (128, 9, 8, 2), (64, 9, 31, 2), (128, 6, 32, 33), (64, 6, 1024, 2), (64, 9, 1024, 33)]


def test_the_lane_order_cases_cover_the_edge_action_counts():
    assert set(PC.EDGE_ACTIONS) <= {c[2] for c in _LANE_CASES} and PC.EDGE_ACTIONS == [1, 8, 31, 32, 33, 1024]
    for na in (1, 32, 1024):  # each with both n
        assert {s[0] for s in PC.EDGE_SHAPES if s[3] == na} == {3, 33}


@pytest.mark.parametrize("ew,na", [(6 if i % 2 == 0 else 9, na) for i, na in enumerate(PC.EDGE_ACTIONS)])
def test_pack_index_and_grad_floats_round_trip_at_the_edge_action_counts(ew, na):
    """The blob holds every parameter exactly once (the padding entries point at the trailing zero), the head's tiles are
    (n_actions + 1 + 31) / 32, and the state dict comes back from the packed blob."""
    from gpudrive_lab_amd.policy import expected_shapes, grad_floats, pack_index
    sd = PC.state_dict(3, ew, na)
    shapes = expected_shapes(ew, na)
    G, index = grad_floats(ew, na), pack_index(ew, na)
    assert G == sum(v.numel() for v in sd.values()) and list(shapes) == list(sd)
    tiles = (na + 1 + 31) // 32
    assert len(index) - len(pack_index(ew, 31)) == (tiles - 1) * (64 * 64 + 32)
    assert (np.bincount(index, minlength=G + 1)[:G] == 1).all() and (index == G).sum() == len(index) - G
    flat = np.concatenate([sd[k].numpy().reshape(-1) for k in shapes] + [np.zeros(1, np.float32)])
    blob = flat[index]
    back = np.zeros(G + 1, np.float32)
    back[index] = blob
    assert np.array_equal(back.view(np.int32), flat.view(np.int32))


@pytest.mark.parametrize("max_agents,ego_width,n_actions,n", _LANE_CASES)
def test_the_packed_blob_read_in_lane_order_gives_the_reference(max_agents, ego_width, n_actions, n):
    from gpudrive_lab_amd.policy import expected_shapes, pack_index
    sd = PC.negative_pool_state(_sd(ego_width, n_actions))
    obs = PC.observations(6, n, max_agents, ego_width)
    flat = np.concatenate([sd[k].numpy().reshape(-1) for k in expected_shapes(ego_width, n_actions)] + [np.zeros(1, np.float32)])
    blob = flat[pack_index(ego_width, n_actions)]
    logits, value = _emulate(blob, obs, max_agents, ego_width, n_actions)
    wl, wv, _ = REF.forward(sd, obs, max_agents, ego_width)
    assert np.abs(logits - wl).max() < 1e-9 and np.abs(value - wv).max() < 1e-9
