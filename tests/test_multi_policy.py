"""CPU tests of the multi-policy evaluator (gd_owned_rows, gd_policy_forward_owned, gd_multi_policy_rollout,
gpudrive_lab_amd.multi_policy_rollout): the surface, the refusals before any launch, the construction errors, and the rule
(csrc/multi_policy_rule.hpp, as a host program) against the numpy restatement of the reference (tests/multi_policy_reference.py),
bit for bit."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import multi_policy_reference as MREF
from tests import ppo_rollout_reference as REF
from tests.conftest import ROOT
from tests.test_ppo_rollout import _script, _StubSim, _stub_policy

NEW = ("gd_owned_rows", "gd_policy_forward_owned", "gd_multi_policy_rollout")
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()


def test_the_symbols_are_declared_exported_and_bound():
    header = _header()
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS and name in exported, name
        assert getattr(L, name).argtypes is not None, name
    assert "#define GD_POLICY_SET_MAX 8" in header and _capi.POLICY_SET_MAX == 8
    assert len(L.gd_owned_rows.argtypes) == 10 and len(L.gd_policy_forward_owned.argtypes) == 13
    assert len(L.gd_multi_policy_rollout.argtypes) == 5


def _fields(header, name):
    body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [f for f in re.findall(r"[ *](\w+)(?:\[\w+\])?[,;]", code)]


def test_the_structs_have_the_header_layout():
    header = _header()
    S, M = _capi.GdPolicySet, _capi.GdMultiPolicyBuffers
    assert _fields(header, "gd_policy_set") == [f[0] for f in S._fields_]
    assert _fields(header, "gd_multi_policy_buffers") == [f[0] for f in M._fields_]
    assert S.policy.offset == 8 and S.features.offset == 8 + 8 * C.sizeof(_capi.GdPolicy) and C.sizeof(S) == S.logits.offset + 8
    assert C.sizeof(_capi.GdPolicy) == 48
    assert M.owner.offset == 0 and M.list_count.offset == 14 * 8 and M.reserved.offset == 15 * 8 and C.sizeof(M) == 16 * 8
    from gpudrive_lab_amd import multi_policy_rollout as mod
    assert mod.POLICY_WORLD_RESULTS == MREF.WORLD_NAMES and mod.POLICY_SUMMARY_NAMES == MREF.SUMMARY_NAMES
    assert mod.METRIC_KEYS == MREF.METRIC_KEYS
    hdr = open(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "multi_policy_rule.hpp")).read()
    enum = re.search(r"enum \{ (S_GOAL_ACHIEVED.*?) \};", hdr).group(1)
    assert [n.strip()[2:].lower() for n in enum.split(",")] == list(MREF.SUMMARY_NAMES)
    assert "MAX_POLICIES = 8" in hdr and "SEGMENT_ALIGN = 32" in hdr and _capi.OWNED_ROWS_ALIGN == 32


def test_exported_from_the_package():
    import gpudrive_lab_amd
    from gpudrive_lab_amd.multi_policy_rollout import ClosedLoopMultiPPO, MultiPolicyEpisode
    assert gpudrive_lab_amd.ClosedLoopMultiPPO is ClosedLoopMultiPPO and gpudrive_lab_amd.MultiPolicyEpisode is MultiPolicyEpisode


# ---- the refusals of the three calls come before any launch: no device is needed to provoke them
def _buf(n=64):
    """An aligned host buffer: the calls below are refused before anything would read it."""
    b = (C.c_uint64 * n)()
    return b, C.addressof(b)


def _refused(rc, match):
    assert rc == _capi.GD_ERR_INVALID, rc
    msg = _capi.lib().gd_last_error().decode()
    assert re.search(match, msg), msg


def test_owned_rows_refusals():
    L = _capi.lib()
    keep, a = _buf()
    good = [a, a, 5, 2, a, a, a, a, None, None]
    for i in (0, 1, 4, 5, 6, 7):
        args = list(good)
        args[i] = None
        _refused(L.gd_owned_rows(*args), "gd_owned_rows: null")
    for i in (4, 5, 6, 7, 8):
        args = list(good)
        args[i] = a + 2
        _refused(L.gd_owned_rows(*args), "4-byte aligned")
    for P in (0, 9, -1):
        args = list(good)
        args[3] = P
        _refused(L.gd_owned_rows(*args), r"n_policies must be in \[1, 8\]")
    for n in (0, (1 << 20) + 1):
        args = list(good)
        args[2] = n
        _refused(L.gd_owned_rows(*args), "n must be in")


def _set(keep_addr, P=2, n=5, A=64, ew=6, na=91):
    s = _capi.GdPolicySet()
    s.n_policies = P
    floats = _blob_floats(ew, na)
    for i in range(min(max(P, 0), 8)):
        g = s.policy[i]
        g.num_rows, g.max_agents, g.ego_width, g.n_actions, g.blob, g.blob_floats = n, A, ew, na, keep_addr, floats
    s.features = s.logits = keep_addr
    return s


def _blob_floats(ew, na):
    from gpudrive_lab_amd.policy import pack_index
    return int(pack_index(ew, na).size)


def test_forward_owned_refusals():
    L = _capi.lib()
    keep, a = _buf()
    tail = [a, a, 0, a, a, a, a, None, a, a, a, None]  # obs, u, deterministic, four outputs, logits_out, rows, start, count
    call = lambda s, t=tail: L.gd_policy_forward_owned(C.byref(s) if s is not None else None, *t)  # noqa: E731
    _refused(call(None), "null")
    for P in (0, 9):
        _refused(call(_set(a, P=P)), r"n_policies must be in \[1, 8\]")
    s = _set(a)
    s.reserved = 1
    _refused(call(s), "reserved")
    s = _set(a)
    s.features = None
    _refused(call(s), "features and logits")
    s = _set(a)
    s.features = a + 4
    _refused(call(s), "16-byte aligned")
    s = _set(a)
    s.policy[1].blob = None
    _refused(call(s), "blob")
    for field, value in (("n_actions", 5), ("ego_width", 9), ("max_agents", 128), ("num_rows", 6)):
        s = _set(a)
        setattr(s.policy[1], field, value)
        s.policy[1].blob_floats = _blob_floats(s.policy[1].ego_width, s.policy[1].n_actions)
        _refused(call(s), "must agree")
    for i in (8, 9, 10):
        t = list(tail)
        t[i] = None
        _refused(call(_set(a), t), "rows, start and count are required")
        t[i] = a + 2
        _refused(call(_set(a), t), "4-byte aligned")
    t = list(tail)
    t[0] = None
    _refused(call(_set(a), t), "null")


def test_multi_policy_rollout_refusals():
    L = _capi.lib()
    keep, a = _buf()
    sim = C.c_void_p(a)  # never dereferenced: every call below is refused by the checks that need no simulator
    b = _capi.GdPolicyRolloutBuffers()
    b.n_rows, b.live = 5, a
    m = _capi.GdMultiPolicyBuffers()
    for name, _ in m._fields_[:-1]:
        setattr(m, name, a)
    call = lambda s, bb, mm: L.gd_multi_policy_rollout(sim, None if s is None else C.byref(s), None if bb is None else C.byref(bb),  # noqa: E731
                                                       None if mm is None else C.byref(mm), 91)
    for args in ((None, b, m), (_set(a), None, m), (_set(a), b, None)):
        _refused(call(*args), "gd_multi_policy_rollout: null")
    _refused(L.gd_multi_policy_rollout(None, C.byref(_set(a)), C.byref(b), C.byref(m), 91), "null")
    for P in (0, 9):
        _refused(call(_set(a, P=P), b, m), r"n_policies must be in \[1, 8\]")
    for name in ("owner", "rows", "start", "count", "scratch"):
        mm = _capi.GdMultiPolicyBuffers.from_buffer_copy(m)
        setattr(mm, name, None)
        _refused(call(_set(a), b, mm), "null")
    for name in ("rows", "start", "count", "scratch", "list_count"):
        mm = _capi.GdMultiPolicyBuffers.from_buffer_copy(m)
        setattr(mm, name, a + 2)
        _refused(call(_set(a), b, mm), "4-byte aligned")
    for name in ("denominator", "frac_collided", "n_rows", "summary"):
        mm = _capi.GdMultiPolicyBuffers.from_buffer_copy(m)
        setattr(mm, name, None)
        _refused(call(_set(a), b, mm), "every buffer of gd_multi_policy_buffers")
        setattr(mm, name, a + 2)
        _refused(call(_set(a), b, mm), "4-byte aligned")
    mm = _capi.GdMultiPolicyBuffers.from_buffer_copy(m)
    mm.reserved = 3
    _refused(call(_set(a), b, mm), "reserved")


# ---- the construction errors of ClosedLoopMultiPPO
W_C, A_C = 3, 64


class _Controlled(_StubSim):
    """A stand-in whose controlled agents can be read (on the host) and nothing else."""

    def controlled_state_tensor(self):
        t = torch.zeros(W_C, A_C, 1, dtype=torch.int32)
        t[0, :5] = 1
        t[2, 7] = 1
        return types.SimpleNamespace(to_torch=lambda: t)


def _mask(*slots):
    m = torch.zeros(W_C, A_C, dtype=torch.bool)
    for w, a in slots:
        m[w, a] = True
    return m


def _all():
    return torch.ones(W_C, A_C, dtype=torch.bool)


def test_refuses_more_than_eight_policies_and_bad_entries():
    from gpudrive_lab_amd.multi_policy_rollout import ClosedLoopMultiPPO
    with pytest.raises(ValueError, match="at most 8"):
        ClosedLoopMultiPPO(_StubSim(0), {i: (_stub_policy(), _all()) for i in range(9)})
    for bad in ({}, None, [(_stub_policy(), _all())]):
        with pytest.raises(ValueError, match="dict"):
            ClosedLoopMultiPPO(_StubSim(0), bad)
    with pytest.raises(ValueError, match="pair"):
        ClosedLoopMultiPPO(_StubSim(0), {"a": _stub_policy()})
    with pytest.raises(ValueError, match="DevicePolicy"):
        ClosedLoopMultiPPO(_StubSim(0), {"a": (object(), _all())})
    for mask in (torch.ones(W_C, 63, dtype=torch.bool), torch.ones(W_C, A_C), np.ones((W_C, A_C), bool), None):
        with pytest.raises(ValueError, match="mask"):
            ClosedLoopMultiPPO(_StubSim(0), {"a": (_stub_policy(), mask)})
    with pytest.raises(ValueError, match="State"):
        ClosedLoopMultiPPO(_StubSim(3), {"a": (_stub_policy(), _all())})
    with pytest.raises(ValueError, match="at most 8"):
        ClosedLoopMultiPPO.nbytes(_StubSim(0), {i: (_stub_policy(), _all()) for i in range(9)})


@pytest.mark.parametrize("other", [dict(n_actions=5), dict(ego_width=9), dict(max_agents=128)])
def test_refuses_policies_of_different_shapes_before_any_device_call(other):
    from gpudrive_lab_amd.multi_policy_rollout import ClosedLoopMultiPPO
    with pytest.raises(ValueError, match="share one shape"):
        ClosedLoopMultiPPO(_StubSim(0), {"a": (_stub_policy(), _all()), "b": (_stub_policy(**other), _all())})
    with pytest.raises(ValueError, match="max_agents"):
        ClosedLoopMultiPPO(_StubSim(0, A=64), {"a": (_stub_policy(max_agents=128), torch.ones(3, 64, dtype=torch.bool))})


def test_refuses_masks_that_overlap_or_do_not_cover():
    from gpudrive_lab_amd.multi_policy_rollout import ClosedLoopMultiPPO
    sim = _Controlled(0)
    first, rest = _mask((0, 0), (0, 1), (0, 2)), _mask((0, 3), (0, 4), (2, 7))
    with pytest.raises(ValueError, match="do not cover the controlled agents: 1 controlled"):
        ClosedLoopMultiPPO(sim, {"a": (_stub_policy(), first), "b": (_stub_policy(), _mask((0, 3), (0, 4)))})
    with pytest.raises(ValueError, match="share a controlled slot"):
        ClosedLoopMultiPPO(sim, {"a": (_stub_policy(), first | _mask((0, 3))), "b": (_stub_policy(), rest)})
    # slots no agent is controlled in may be shared and need no cover: the next refusal is the stand-in's, past the checks
    shared = _mask((1, 9))
    with pytest.raises((AssertionError, AttributeError)):
        ClosedLoopMultiPPO(sim, {"a": (_stub_policy(), first | shared), "b": (_stub_policy(), rest | shared)})


def test_owner_and_denominator():
    from gpudrive_lab_amd.multi_policy_rollout import _owners
    controlled = _Controlled(0).controlled_state_tensor().to_torch().squeeze(-1) == 1
    first, rest = _mask((0, 0), (0, 2), (1, 9), (1, 10)), _mask((0, 1), (0, 3), (0, 4), (2, 7), (1, 9))
    owner, den = _owners(controlled, (first, rest))
    assert owner[controlled].tolist() == [0, 1, 0, 1, 1, 1] and bool((owner[~controlled] == 255).all())
    assert den.tolist() == [5, 3, 1] and den.dtype == torch.float32  # (world 1: three mask slots, none controlled)


def test_nbytes_counts_the_list_and_the_per_policy_results():
    from gpudrive_lab_amd.multi_policy_rollout import ClosedLoopMultiPPO
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    sim = _Controlled(0)
    pols = {"a": (_stub_policy(), _all()), "b": (_stub_policy(), _all()), "c": (_stub_policy(), _all())}
    n, P = 6, 3
    extra = 4 * ((n + 32 * P) + (P + 1) + P + P * 1) + 91 * P * 4 + 7 * P * W_C * 4 + P * 4 * 4
    for kw in (dict(), dict(record=True), dict(stochastic=True)):
        assert ClosedLoopMultiPPO.nbytes(sim, pols, **kw) == ClosedLoopPPO.nbytes(sim, _stub_policy(), **kw) + extra


# ---- the rule header as a host program against the numpy restatement
COUNTS = {1: [[0], [1], [31], [32], [33], [1000]],
          2: [[0, 0], [0, 1], [1, 0], [31, 33], [32, 32], [33, 31], [64, 0], [5, 1]],
          3: [[32, 0, 32], [64, 0, 1], [0, 0, 0], [1, 1, 1], [31, 32, 33], [33, 0, 0], [0, 0, 7]],
          8: [[0] * 8, [1] * 8, [32, 0, 32, 0, 31, 33, 1, 0], [0, 0, 0, 0, 0, 0, 0, 5], [33, 32, 31, 1, 0, 64, 65, 2]]}


@pytest.mark.parametrize("P", sorted(COUNTS))
def test_segment_starts_host_program_equals_numpy(P):
    for count in COUNTS[P]:
        start, seg = MREF.run_starts_host(count)
        want = MREF.segment_starts(count)
        assert start.tolist() == want.tolist(), (count, start, want)
        assert (start % 32 == 0).all() and start[0] == 0
        assert all(start[p + 1] - (start[p] + count[p]) in range(32) for p in range(P))
        n = sum(count)
        assert np.array_equal(seg, MREF.segments(want[:-1], count, n + 32 * P)), count
        assert [(seg == p).sum() for p in range(P)] == list(count)
    assert MREF.segment_starts([32, 0, 32]).tolist() == [0, 32, 32, 64] if P == 3 else True


def _constructed():
    """5 worlds x 8 slots, 3 policies.  World 0 has no rows (NaN fractions); world 1: policy 1 has no rows; world 2: a
    denominator larger than the number of rows; world 3: every slot a row, all policies; world 4: one row, of policy 2."""
    W, A = 5, 8
    owner = np.full((W, A), -1, np.int32)
    goal, coll, off = (np.zeros((W, A), f32) for _ in range(3))
    owner[1, [0, 3, 4]] = [0, 2, 0]
    goal[1, 0], coll[1, 3], off[1, 4] = 1, 2, 3
    goal[1, 6] = 5  # a slot that is no row: never counted
    owner[2, [1, 2, 5]] = [0, 1, 2]
    goal[2, 1] = goal[2, 2] = 1
    off[2, 2] = 1
    owner[3] = [0, 1, 2, 0, 1, 2, 0, 1]
    goal[3, :5] = 1
    coll[3, 4:] = [1, 2, 1, 3]
    off[3, 7] = 1
    owner[4, 7] = 2
    denominator = np.array([0, 3, 7, 8, 1], f32)
    return owner, goal, coll, off, denominator


def _want_metrics(owner, goal, coll, off, denominator, P):
    """compute_metrics on the reference's own layout: per-policy [W, A] accumulators, zero outside the policy's slots."""
    acc = [dict(goal_achieved=np.where(owner == p, goal, 0).astype(f32), collided=np.where(owner == p, coll, 0).astype(f32),
                off_road=np.where(owner == p, off, 0).astype(f32)) for p in range(P)]
    per = MREF.compute_metrics(acc, denominator)
    for p, m in enumerate(per):
        m["n_rows"] = (owner == p).sum(1).astype(f32)
    return per, MREF.summary(per)


def _same_f32(g, w, what):
    g, w = np.asarray(g), np.asarray(w)
    assert g.dtype == np.float32 and w.dtype == np.float32 and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan]), (what, g, w)


@pytest.mark.parametrize("sanitize", [False, True])
def test_metrics_host_program_equals_compute_metrics(sanitize):
    """sanitize: the same through a stand-alone executable built with -fsanitize=address,undefined."""
    P = 3
    args = _constructed()
    got, got_summary = MREF.run_metrics_host(*args, P, sanitize=sanitize)
    want, want_summary = _want_metrics(*args, P)
    for p in range(P):
        for k in MREF.WORLD_NAMES:
            _same_f32(got[p][k], want[p][k], "policy %d %s" % (p, k))
    _same_f32(got_summary, want_summary, "summary")
    assert all(np.isnan(want[p]["frac_goal_achieved"][0]) for p in range(P)), "world 0 has no rows and a denominator of 0"
    assert want[1]["n_rows"][1] == 0 and want[1]["frac_collided"][1] == 0, "world 1: policy 1 has no rows"
    assert want[0]["frac_goal_achieved"][2] == f32(1) / f32(7) and want[0]["n_rows"][2] == 1, "world 2: denominator > rows"
    assert want_summary.tolist() == [[4, 1, 1, 6], [3, 2, 2, 4], [1, 2, 0, 5]]
    if sanitize:
        for count in COUNTS[8]:
            assert MREF.run_starts_host(count, sanitize=True)[0].tolist() == MREF.segment_starts(count).tolist()


def test_258_worlds_cross_the_lanes_of_the_summary():
    rng = np.random.default_rng(5)
    W, A, P = 258, 8, 2
    owner = rng.integers(-1, P, (W, A)).astype(np.int32)
    goal, coll, off = ((rng.random((W, A)) < 0.3).astype(f32) * rng.integers(1, 4, (W, A)) for _ in range(3))
    den = rng.integers(0, 12, W).astype(f32)
    got, got_summary = MREF.run_metrics_host(owner, goal, coll, off, den, P)
    want, want_summary = _want_metrics(owner, goal.astype(f32), coll.astype(f32), off.astype(f32), den, P)
    for p in range(P):
        for k in MREF.WORLD_NAMES:
            _same_f32(got[p][k], want[p][k], "policy %d %s" % (p, k))
    _same_f32(got_summary, want_summary, "summary")


# ---- the metrics half of the restated loop on scripted sequences
def _split(control):
    """Two policies by slot parity, with a mask slot that holds no controlled agent in world 0 of policy 1."""
    even = np.zeros_like(control)
    even[:, 0::2] = True
    odd = ~even
    return [even & control, (odd & control) | _uncontrolled(control)]


def _uncontrolled(control):
    extra = np.zeros_like(control)
    extra[0, 1] = True
    assert not control[0, 1]
    return extra


def test_restated_metrics_on_scripted_sequences():
    control, done, info = _script()
    single = REF.metrics(control, done, info)
    one = MREF.metrics(control, [control], done, info)
    assert one["iterations"] == single["iterations"] == 91
    assert np.array_equal(one["episode_lengths"], single["episode_lengths"]) and np.array_equal(one["live"], single["live"])
    m = one["policies"][0]
    for k in ("goal_achieved", "collided", "off_road", "goal_achieved_count", "collided_count", "off_road_count",
              "frac_goal_achieved", "frac_collided", "frac_off_road"):
        _same_f32(m[k], single[k], "one policy " + k)
    assert np.array_equal(one["list_count"][:91, 0], [int(x) for x in _live_counts(control, done)])

    masks = _split(control)
    two = MREF.metrics(control, masks, done, info)
    assert two["iterations"] == 91 and np.array_equal(two["episode_lengths"], single["episode_lengths"])
    for k in ("goal_achieved", "collided", "off_road"):
        _same_f32(two["policies"][0][k] + two["policies"][1][k], single[k], "the policies' sums add up: " + k)
        assert not (two["policies"][0][k][:, 1::2]).any() and not (two["policies"][1][k][:, 0::2]).any()
    for k in ("goal_achieved_count", "collided_count", "off_road_count"):
        _same_f32(two["policies"][0][k] + two["policies"][1][k], single[k], k)
    assert two["denominator"].tolist() == [1, 1, 3, 2, 2, 8], "world 0: one mask slot, no controlled agent"
    assert two["policies"][0]["frac_goal_achieved"][0] == 0 and not np.isnan(two["policies"][1]["frac_off_road"][0])
    # world 5: every slot a row; the four goals are slots 0..3, two of each parity
    assert two["policies"][0]["goal_achieved_count"][5] == 2 and two["policies"][1]["frac_goal_achieved"][5] == f32(2) / f32(8)
    assert two["summary"][:, 3].tolist() == [8, 8] and (two["list_count"][0] == [8, 8]).all()
    assert np.array_equal(two["list_count"].sum(1), one["list_count"][:, 0])
    # the device's layout: owner per slot and the accumulators over all rows give the same per-policy numbers
    owner = np.where(control, np.where(masks[0], 0, 1), -1).astype(np.int32)
    got, got_summary = MREF.run_metrics_host(owner, single["goal_achieved"], single["collided"], single["off_road"],
                                             two["denominator"], 2)
    for p in range(2):
        for k in MREF.WORLD_NAMES:
            _same_f32(got[p][k], two["policies"][p][k], "host program, policy %d %s" % (p, k))
    _same_f32(got_summary, two["summary"], "host program summary")


def _live_counts(control, done):
    live = control.copy()
    for t in range(done.shape[0]):
        yield live.sum()
        live[done[t] != 0] = False


def test_restated_metrics_break_and_prefix():
    control, done, info = _script()
    keep = [0, 1, 3, 4, 5]
    r = MREF.metrics(control[keep], _split(control[keep]), done[:, keep], info[:, keep])
    assert r["iterations"] == 61 and bool((r["list_count"][61:] == 0).all())
    p = MREF.metrics(control, _split(control), done[:7], info[:7])
    full = MREF.metrics(control, _split(control), done, info)
    assert p["iterations"] == 7 and np.array_equal(p["list_count"][:7], full["list_count"][:7])


# ---- the restatements by block, position, wave and lane, and the wrong rules the new GPU cases are built to see
SMALL = (1, 31, 32, 33, 1023, 1024, 1025, 2100)            # the sizes of test_owned_rows_equals_the_restatement
MANY_BLOCKS = (262144, 262145, 1 << 20)                     # and of test_owned_rows_at_more_blocks_than_lanes
BLOCK_RULES = (None, "one_trip", "before_le")


def _lists_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_the_list_by_blocks_is_the_list_on_the_small_sizes_under_every_rule(P):
    """The restatement by blocks of 1024 rows equals `owned_list` on every existing size and pattern; so do the rule whose sums
    stop at 256 blocks and the rule whose split is `i <= block` from the second trip on (no existing size has more than 3
    blocks)."""
    rng = np.random.default_rng(100 + P)
    for n in SMALL:
        for name, (mask, owner) in MREF.list_patterns(n, P, rng).items():
            want = MREF.owned_list(mask, owner, P, -7)
            for wrong in BLOCK_RULES:
                assert _lists_equal(MREF.owned_list_blocks(mask, owner, P, -7, wrong=wrong), want), (n, P, name, wrong)


@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("n", MANY_BLOCKS)
def test_the_many_block_cases_see_the_rules_they_are_built_for(P, n):
    """At more than 256 blocks `late` and `straddle` differ under 'one_trip' (at exactly 256 blocks that rule is the right one,
    and is asserted equal), and so under 'before_le'; `late` under 'one_trip' loses owner P - 1's count and, at
    P = 8, nothing else, which is what it is built to isolate.  The restatement stays fast at 2^20 rows (it is `owned_list`'s
    cost, a few hundred milliseconds for all the patterns)."""
    import time
    rng = np.random.default_rng(1000 * P + n % 1000)
    blocks = -(-n // 1024)
    cases = dict(MREF.list_patterns(n, P, rng), **MREF.many_block_patterns(n, P, rng))
    t0 = time.perf_counter()
    want = {name: MREF.owned_list(mask, owner, P, -7) for name, (mask, owner) in cases.items()}
    spent = time.perf_counter() - t0
    print("MULTI owned_list n=%d P=%d: %d patterns in %.3f s" % (n, P, len(cases), spent))
    for name, (mask, owner) in cases.items():
        assert _lists_equal(MREF.owned_list_blocks(mask, owner, P, -7), want[name]), (n, P, name)
    for name in ("late", "straddle"):
        mask, owner = cases[name]
        rows, start, count = want[name]
        got = MREF.owned_list_blocks(mask, owner, P, -7, wrong="one_trip")
        assert _lists_equal(got, want[name]) == (blocks <= 256), (n, P, name)
        le = MREF.owned_list_blocks(mask, owner, P, -7, wrong="before_le")
        assert _lists_equal(le, want[name]) == (blocks <= 256), (n, P, name)
        assert _lists_equal(le[1:], want[name][1:]), "the counts and starts are the right ones: only positions move"
        if blocks > 256 and name == "late":
            assert got[2][P - 1] == 0 < count[P - 1] and got[2][:P - 1].tolist() == count[:P - 1].tolist()
        if blocks > 256 and name == "straddle":
            assert 0 < got[2][0] < count[0], "owner 0 keeps block 255's rows and loses the others"


def test_the_restatement_of_the_list_is_vectorised():
    """2^20 rows, 8 owners: well under a second, so the GPU case's time is the device's."""
    import time
    rng = np.random.default_rng(3)
    n = 1 << 20
    mask, owner = (rng.random(n) < 0.7).astype(np.uint8), rng.integers(0, 10, n).astype(np.uint8)
    best = 1e9
    for _ in range(2):
        t0 = time.perf_counter()
        MREF.owned_list(mask, owner, 8, -7)
        best = min(best, time.perf_counter() - t0)
    print("MULTI owned_list 2^20 rows, P = 8: %.3f s" % best)
    assert best < 1.0


N_EIGHT = 140


def test_weights_from_blob_p_mod_4_show_at_eight_policies_only():
    """Which weights the forward on an owned list gives a row, read off the list position by position: the owner's.  A rule
    that takes blob[p % 4] is the same rule for P <= 4 -- every existing case -- and at P = 8 gives every listed row of owners
    4 .. 7 other weights, in every pattern of the new case that lists such a row."""
    for n, Ps in ((1, (1, 2, 3)), (33, (1, 2, 3)), (70, (1, 2, 3)), (1100, (1, 2, 3)), (N_EIGHT, (5, 8))):
        rng = np.random.default_rng(7 * n + 64)
        for P in Ps:
            for name, (mask, owner) in MREF.owner_patterns(n, P, rng).items():
                right = MREF.blob_of_rows(mask, owner, P)
                listed = mask & (owner < P)
                assert np.array_equal(right, np.where(listed, owner.astype(np.int32), -1)), (n, P, name)
                bad = MREF.blob_of_rows(mask, owner, P, wrong="blob_mod4")
                moved = listed & (owner >= 4)
                assert np.array_equal(bad != right, moved), (n, P, name)
                if P <= 3:
                    assert not moved.any()
                elif P == 8 and name != "empty":
                    assert moved.any(), (name, "lists no row of an owner >= 4")
    assert sum(MREF.OWNER_SIZES) == 132 <= N_EIGHT < 132 + 32


def _mod8_world(A=128):
    """Three worlds of 128 slots, owner = slot % 8 among the controlled slots: world 0 controlled below slot 64 only, world 1
    from slot 64 on only, world 2 on both sides.  Accumulators > 0 on both sides."""
    rng = np.random.default_rng(8)
    ctrl = rng.random((3, A)) < 0.5
    ctrl[0, 64:] = False
    ctrl[1, :64] = False
    owner = np.where(ctrl, np.arange(A) % 8, -1).astype(np.int32)
    goal, coll, off = ((rng.random((3, A)) < 0.4).astype(f32) * rng.integers(1, 4, (3, A)) for _ in range(3))
    den = ctrl.sum(1).astype(f32)
    return owner, goal.astype(f32), coll.astype(f32), off.astype(f32), den


def test_counts_of_the_first_wave_only_show_at_128_slots():
    """The counts per wave of 64 slots, added over the waves, are compute_metrics' and the host program's on every existing
    case (all of one wave: 8 slots), and so is the rule that adds the first wave only.  On 128 slots with eight policies on
    either side of slot 64 that rule differs for every policy, in the world with rows on both sides and in the one with rows
    in the second wave only."""
    rng = np.random.default_rng(5)
    W, A = 258, 8
    big = (rng.integers(-1, 2, (W, A)).astype(np.int32),) + tuple(
        ((rng.random((W, A)) < 0.3) * rng.integers(1, 4, (W, A))).astype(f32) for _ in range(3)) + (rng.integers(0, 12, W).astype(f32),)
    for args, P in ((_constructed(), 3), (big, 2)):
        want, _ = _want_metrics(*args, P)
        for wrong in (None, "wave0"):
            got = MREF.world_counts_by_wave(*args[:4], P, wrong=wrong)
            for p in range(P):
                for j, k in enumerate(("goal_achieved_count", "collided_count", "off_road_count", "n_rows")):
                    assert np.array_equal(got[p, :, j].astype(f32), want[p][k]), (P, p, k, wrong)
    args, P = _mod8_world(), 8
    host, _ = MREF.run_metrics_host(*args, P)
    want, _ = _want_metrics(*args, P)
    right, bad = (MREF.world_counts_by_wave(*args[:4], P, wrong=wrong) for wrong in (None, "wave0"))
    for p in range(P):
        for j, k in enumerate(("goal_achieved_count", "collided_count", "off_road_count", "n_rows")):
            assert np.array_equal(right[p, :, j].astype(f32), want[p][k]) and np.array_equal(host[p][k], want[p][k]), (p, k)
        assert np.array_equal(bad[p, 0], right[p, 0]), "world 0 has no row from slot 64 on"
        assert (bad[p, 1] == 0).all() and right[p, 1, 3] > 0 and 0 < bad[p, 2, 3] < right[p, 2, 3], p
        assert (bad[p, :, :3] != right[p, :, :3]).any(), (p, "no flag of the second wave counts")


def test_a_summary_of_the_first_256_worlds_shows_at_258():
    """The rule that adds a lane's first world only is the right rule on every existing case of up to 256 worlds, and at 258
    worlds with three policies, owner = (world + slot) % 3, it differs for every policy in every one of the four totals once
    worlds 256 and 257 hold a row and a count of each (they do here by construction; the GPU case asserts it on its run)."""
    per, _ = _want_metrics(*_constructed(), 3)
    assert np.array_equal(MREF.summary(per, wrong="first_256"), MREF.summary(per))
    control, done, info = _script()
    two = MREF.metrics(control, _split(control), done, info)
    assert np.array_equal(MREF.summary(two["policies"], wrong="first_256"), two["summary"])
    rng = np.random.default_rng(11)
    W, A, P = 258, 64, 3
    ctrl = rng.random((W, A)) < 0.1
    ctrl[256:, :6] = True
    owner = np.where(ctrl, (np.arange(W)[:, None] + np.arange(A)[None, :]) % P, -1).astype(np.int32)
    goal, coll, off = ((rng.random((W, A)) < 0.3).astype(f32) for _ in range(3))
    goal[256:, :6] = coll[256:, :6] = off[256:, :6] = 1
    den = ctrl.sum(1).astype(f32)
    got, got_summary = MREF.run_metrics_host(owner, goal, coll, off, den, P)
    want, want_summary = _want_metrics(owner, goal, coll, off, den, P)
    _same_f32(got_summary, want_summary, "summary")
    for p in range(P):
        assert (want[p]["n_rows"][256:] > 0).all() and all(want[p][k][256:].sum() > 0 for k in MREF.WORLD_NAMES[0:5:2])
        for k in MREF.WORLD_NAMES[0:5:2] + ("n_rows",):
            v = want[p][k].astype(np.float64)
            assert (v == np.round(v)).all() and float(REF.ordered_sum(want[p][k])) == v.sum() < 2 ** 24
    assert (MREF.summary(want, wrong="first_256") != want_summary).all()
