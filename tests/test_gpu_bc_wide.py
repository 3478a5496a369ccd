"""GPU suite: the BC policy forward and the closed-loop driver at network_dim = 128 (gd_bc_forward_dim, gd_bc_forward_rows_dim,
gd_bc_rollout_dim; csrc/bc_policy.hip at T = 4) against the float64 restatement, which takes the width from the state dict
(tests/bc_reference.py, pinned to the reference module at 128 by tests/test_bc_wide.py) on the cases of tests/bc_wide_cases.py.

context, means, clamped raw covariances, weights, NLL and ego_attn_score: the yardstick E of a case and an output is the maximum
absolute error of torch's float32 CPU forward of the stand-in at that width (bc_cases.StandIn) against float64 on that case --
the reference side's own error, not the kernel's; the kernel's error must be <= K E with the project's K = 32, and a ratio above
16 would be a bug to find.  Ratios measured on an MI355X (printed per case by this test with -s):
    name (B, A, R)          context  means  log_covariances  weights  nll    ego_attn_score
    wide_min (3, 64, 1)     1.17     1.21   1.92             0 / 0    2.28   3.11
    wide_sweep (3, 64, 5)   1.30     1.55   0.98             4.29     0.49   1.59
    wide_a128 (2, 128, 2)   1.18     1.98   2.58             0.54     0.51   1.02
The edge configurations of bc_wide_cases.EDGE_CASES run through this file's `_forward_checks` from tests/test_gpu_bc_wide_edges.py,
whose docstring has their ratios (the largest 4.55, wide_top's weights).
(`wide_min` has one component: its weight is exactly 1 on both sides; its nll is of magnitude 1e9, a covariance clamped at
exp(-20) under a squared error, and E is 820 there.)  The largest, 4.29, is three rows' weights at E = 4.3e-7, a few float32
ulps of a weight near 1, as the one-sample case is at 64.
Actions, the component and the draw are held to the rule in float64 on the kernel's OWN mixture parameters, as at 64
(tests/test_gpu_bc_policy._check_rule): the deterministic action is exactly the mean of the first component of maximal weight,
the draw is where u falls.  Everything else is bit-identity: chunks, the row list, out= between guard words, two calls,
load_state_dict against a fresh policy, uint8 against bool masks, gd_bc_forward_dim at 64 against gd_bc_forward, and the
closed-loop episode against the restated loop (tests/bc_rollout_reference.py) with the wide policy in it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bc_cases as BC
from tests import bc_wide_cases as WC
from tests.test_gpu_bc_policy import ALL, CANARY_BITS, EPS, _carved_outputs, _check_rule, _dev, _host, _no_sync, _same_bits

pytestmark = pytest.mark.gpu

K = 32
KEYS = BC.COMPARED + ("nll", "ego_attn_score")
F_CANARY = 1234.5


def _policy(c, **kw):
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    return DeviceBCPolicy.from_state_dict(kw.pop("sd", c["sd"]), max_agents=c["A"], num_stack=c["R"], network_dim=128, **c["cfg"], **kw)


def _inputs(c):
    return _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["u"], c["z"])


@pytest.mark.parametrize("name", WC.GOLDEN_CASES)
def test_forward_against_the_float64_restatement(name):
    _forward_checks(name)


def _forward_checks(name):
    """Everything the wide forward is held to at one case of bc_wide_cases (tests/test_gpu_bc_wide_edges.py runs the edge
    configurations through it).  Returns (case, the outputs on the host, the ratios)."""
    c = WC.case(name)
    B, A, C_ = c["B"], c["A"], c["cfg"]["n_components"]
    bc = _policy(c)
    assert bc.network_dim == 128 and bc._OUT_SHAPES["context"](bc, B) == (B, 384)
    assert bc.nbytes(B) == 4 * (bc.blob.numel() + bc.chunk_rows * 3 * (A + 200) * 128) \
        + B * 4 * (384 + 9 * C_ + C_ + 3 + 1 + 1 + 4 * (A - 1))
    obs, pm, rm, expert, u, z = _inputs(c)
    fresh = _host(bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert))
    assert fresh["context"].shape == (B, 384) and fresh["ego_attn_score"].shape == (B, 4, A - 1)
    carver, out = _carved_outputs(bc, B)
    # the second call of the shape: no host synchronisation, out= buffers, guard words either side, every byte written
    _no_sync(lambda: bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert, out=out))
    carver.assert_guards(name)
    got = _host(out)
    _same_bits(fresh, got, name + " out= against fresh tensors")
    _same_bits(got, _host(bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert)), name + " two calls")
    ratios = {}
    for k in KEYS:
        want = c["ref"][k]
        err = float(np.abs(got[k].astype(np.float64).reshape(want.shape) - want).max())
        E = c["E"][k]
        ratios[k] = err / E if E > 0 else (0.0 if err == 0 else np.inf)
        print("BC WIDE RATIO %s %s err %.3e E %.3e ratio %.2f" % (name, k, err, E, ratios[k]))
    assert max(ratios.values()) <= K, (name, ratios)
    _check_rule(name + " deterministic", got, None, None, True, A)
    s = got["ego_attn_score"].astype(np.float64)
    assert (np.abs(s.sum(-1) - 1.0) <= (A + 8) * EPS).all()
    for i, kind in enumerate(c["kinds"]):
        if "a" in kind:  # every partner masked: uniform over all A - 1 keys
            assert np.abs(got["ego_attn_score"][i] - 1.0 / (A - 1)).max() <= 4 * EPS
    # the public methods are views of the same call
    assert np.array_equal(bc(obs, pm, rm, deterministic=True).cpu().numpy(), got["actions"])
    assert np.array_equal(bc.context(obs, pm, rm).cpu().numpy(), got["context"])
    m, cv, w = bc.gmm_params(obs, pm, rm)
    assert np.array_equal(m.cpu().numpy(), got["means"]) and np.array_equal(cv.cpu().numpy(), got["covariances"])
    assert np.array_equal(w.cpu().numpy(), got["weights"]) and np.array_equal(bc.nll(obs, pm, rm, expert).cpu().numpy(), got["nll"])
    # the draw: seeded uniforms, then u = 0 and u just below 1
    for uu in (c["u"], BC.edge_uniforms(B)):
        d_u, = _dev(uu)
        drawn = _host(bc.forward(obs, pm, rm, ALL, deterministic=False, u=d_u, z=z, expert_actions=expert))
        same = ("context", "means", "weights", "nll", "ego_attn_score")
        _same_bits({k: got[k] for k in same}, {k: drawn[k] for k in same}, name + " drawn against deterministic")
        _check_rule(name + " drawn", drawn, uu, c["z"], False, A)
        assert np.array_equal(bc(obs, pm, rm, u=d_u, z=z).cpu().numpy(), drawn["actions"])
    # raw covariances outside the clamp are clamped exactly
    clip = c["cfg"]["clip_value"]
    lc = got["log_covariances"][:, 0].reshape(B, -1)
    raw = c["ref"]["raw"][:, 3 * C_:6 * C_]
    below, above = raw < clip - 1e-3, raw > 3.58352 + 1e-3
    assert below.any() and above.any()
    assert (lc[below] == np.float32(clip)).all() and (lc[above] == np.float32(3.58352)).all()
    # uint8 masks are bool masks
    _same_bits(got, _host(bc.forward(obs, pm.to(torch.uint8), rm.to(torch.uint8), ALL, deterministic=True, expert_actions=expert)),
               name + " uint8 masks")
    return c, got, ratios


def test_chunks_rows_and_reloaded_weights_give_the_same_bits():
    c = WC.case("wide_chunks")
    B = c["B"]
    obs, pm, rm, expert, u, z = _inputs(c)
    small, whole = _policy(c, chunk_rows=2), _policy(c, chunk_rows=8)
    kw = dict(deterministic=False, u=u, z=z, expert_actions=expert)
    full = _host(whole.forward(obs, pm, rm, ALL, **kw))
    _same_bits(full, _host(small.forward(obs, pm, rm, ALL, **kw)), "chunk_rows 2 against 8")
    # rows=: a shuffled list of 3 of the 5 rows, with both chunk sizes; the others keep the canary
    from gpudrive_lab_amd.policy import LiveRows
    listed = [3, 0, 4]
    for bc in (small, whole):
        lr = LiveRows(B, bc.device)
        lr.rows[:3] = torch.tensor(listed, dtype=torch.int32, device="cuda")
        lr.count.fill_(3)
        out = {}
        for k in ALL:
            shape = bc._OUT_SHAPES[k](bc, B)
            out[k] = torch.full(shape, -7, dtype=torch.int32, device="cuda") if k == "component" else \
                torch.full(shape, F_CANARY, dtype=torch.float32, device="cuda")
        _no_sync(lambda: bc.forward(obs, pm, rm, ALL, out=out, rows=lr, **kw))
        got = _host(out)
        for k in ALL:
            assert np.array_equal(got[k][listed].view(np.int32), full[k][listed].view(np.int32)), (k, "listed rows")
            rest = got[k][[1, 2]]
            assert (rest == (-7 if k == "component" else np.float32(F_CANARY))).all(), (k, "rows that are not listed were written")
    # load_state_dict with other weights equals a fresh policy of those weights
    sd2 = BC.state_dict(c["R"], c["cfg"], seed=11, network_dim=WC.DIM)
    small.load_state_dict({k: v.cuda() for k, v in sd2.items()})
    fresh = _policy(c, sd=sd2, chunk_rows=8)
    a = _host(small.forward(obs, pm, rm, ALL, **kw))
    _same_bits(a, _host(fresh.forward(obs, pm, rm, ALL, **kw)), "load_state_dict against a fresh policy")
    assert np.abs(a["context"] - full["context"]).max() > 0.1
    with pytest.raises(ValueError, match="shape"):
        small.load_state_dict(BC.state_dict(c["R"], c["cfg"], network_dim=64))


def test_the_dim_entry_points_at_64_are_the_64_wide_forward():
    from gpudrive_lab_amd import _capi
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    B, A, R = 3, 64, 1
    obs, pm, rm, expert, u, z, _ = BC.inputs(B, A, R)
    obs, pm, rm, expert, u, z = _dev(obs, pm, rm, expert, u, z)
    bc = DeviceBCPolicy.from_state_dict(BC.state_dict(R), max_agents=A, num_stack=R, **BC.CFG)
    assert bc.network_dim == 64
    want = _host(bc.forward(obs, pm, rm, ALL, deterministic=False, u=u, z=z, expert_actions=expert))
    carver, out = _carved_outputs(bc, B)
    o = _capi.GdBCOutputs()
    for k, t in out.items():
        setattr(o, k, t.data_ptr())
    p = bc.c_struct_dim()
    assert p.network_dim == 64
    L = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _no_sync(lambda: _capi.check(L.gd_bc_forward_dim(C.byref(p), obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), B, 0, u.data_ptr(),
                                                     z.data_ptr(), expert.data_ptr(), C.byref(o), stream)))
    carver.assert_guards("gd_bc_forward_dim at 64")
    _same_bits(want, _host(out), "gd_bc_forward_dim at 64 against gd_bc_forward")
    from gpudrive_lab_amd.policy import LiveRows
    lr = LiveRows(B, bc.device)
    lr.rows[:2] = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    lr.count.fill_(2)
    _, out2 = _carved_outputs(bc, B)
    for k, t in out2.items():
        setattr(o, k, t.data_ptr())
    _capi.check(L.gd_bc_forward_rows_dim(C.byref(p), obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), B, 0, u.data_ptr(), z.data_ptr(),
                                         expert.data_ptr(), C.byref(o), lr.rows.data_ptr(), lr.count.data_ptr(), stream))
    got = _host(out2)
    for k in ALL:
        assert np.array_equal(got[k][[2, 0]].view(np.int32), want[k][[2, 0]].view(np.int32)), k
        assert (got[k][1].view(np.int32) == CANARY_BITS).all(), (k, "the row that is not listed was written")


def test_what_reads_64_wide_tokens_refuses_a_wide_policy():
    from gpudrive_lab_amd import ClosedLoopBC
    from gpudrive_lab_amd.bc_readout import ProbeReadout
    from gpudrive_lab_amd.lp_probe import DeviceLinearProbe
    from tests.test_gpu_bc_rollout import _Env, _sim
    c = WC.case("wide_min")
    bc = _policy(c)
    obs, pm, rm = _inputs(c)[:3]
    with pytest.raises(ValueError, match="network_dim"):
        bc.hidden(obs, pm, rm)
    with pytest.raises(ValueError, match="network_dim"):
        bc.read(obs, pm, rm, object())
    with pytest.raises(ValueError, match="network_dim"):
        ProbeReadout(bc, "ro_attn", 0, ego=[])
    w = {"head.weight": torch.zeros(64, 64, device="cuda"), "head.bias": torch.zeros(64, device="cuda")}
    with pytest.raises(ValueError, match="network_dim"):
        DeviceLinearProbe(bc, w, model="early_lp", exp="ego")
    with _Env("linear"):
        sim = _sim(64, "delta_local", 2, "linear")
        try:
            with pytest.raises(ValueError, match="network_dim"):
                ClosedLoopBC(sim, bc).run(readout=object())
        finally:
            sim.close()


# ---- the closed loop

# "matrix": the delta_local case of tests/test_gpu_bc_rollout.MATRIX at A = 64 (R = 5, its six scenes, 91 steps).  Under its
# IGNORE collision behaviour no row of these weights dies before the last step, so everything about dead rows would pass there by
# exercising nothing; "removed" is the same case under REMOVED, where rows leave the road and collide early (asserted below).
LOOPS = {"matrix": "64-5-delta-ignore-linear", "removed": (64, 5, "delta_local", 1, "linear")}
LOOP_CFG = BC._cfg((1, 1), 0, 6, -20.0)
_LOOPS = {}


def _loop_case(name):
    """The wide policy in the loop, computed once: run(record=True), run(compact=True, record=True), run(attention=True), the
    restated loop on a twin simulator, and the prefixes that end at the chosen steps."""
    _LOOP = _LOOPS.setdefault(name, {})
    if not _LOOP:
        from gpudrive_lab_amd import ClosedLoopBC
        from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
        from tests.test_gpu_bc_rollout import MATRIX, _Env, _loop, _sim
        A, R, model, cb, roads = MATRIX[LOOPS[name]] if name == "matrix" else LOOPS[name]
        with _Env(roads):
            rsim, tsim = _sim(A, model, cb, roads), _sim(A, model, cb, roads)
            try:
                pol = DeviceBCPolicy.from_state_dict(BC.state_dict(R, LOOP_CFG, network_dim=WC.DIM), max_agents=A, num_stack=R, network_dim=128, **LOOP_CFG)
                loop = ClosedLoopBC(rsim, pol)
                c = _LOOP
                c["N"], c["A"], c["R"], c["pol"] = loop.num_agents, A, R, pol
                c["nbytes"] = ClosedLoopBC.nbytes(rsim, pol, record=True)
                c["ep"] = loop.run(record=True)
                c["epc"] = loop.run(record=True, compact=True)
                c["attn"] = loop.run(attention=True)
                c["attn_c"] = loop.run(attention=True, compact=True)
                g = lambda: torch.Generator(device="cuda").manual_seed(5)  # noqa: E731
                c["drawn"] = loop.run(deterministic=False, generator=g(), record=True)
                torch.cuda.synchronize()
                c["r"] = _loop(tsim, pol, model, R)
                c["r_drawn"] = _loop(tsim, pol, model, R, deterministic=False, u=c["drawn"].u, z=c["drawn"].z)
                steps = int(c["ep"].steps)
                c["chosen"] = (0, steps // 2, steps - 1)
                c["prefix"] = {t: loop.run(n_steps=t + 1) for t in c["chosen"]}
                first = loop.run(n_steps=3, attention=True)
                c["nosync"] = (first, _no_sync(lambda: loop.run(n_steps=3, attention=True)),
                               _no_sync(lambda: loop.run(n_steps=3, attention=True, compact=True)))
                torch.cuda.synchronize()
            finally:
                rsim.close()
                tsim.close()
    return _LOOP


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_closed_loop_equals_the_restated_loop(name):
    from tests.test_gpu_bc_rollout import PER_ROW, PER_STEP, _compare, _same
    c = _loop_case(name)
    ep, epc, r = c["ep"], c["epc"], c["r"]
    print("BC WIDE ROLLOUT %s rows %d steps %d dead %d summary %s" % (name, c["N"], r["iterations"], int(r["dead"].sum()), r["summary"].tolist()))
    assert c["N"] >= 26 and bool((ep.actions != 0).any()) and bool(torch.isfinite(ep.actions).all())
    _compare(ep, r, "wide run(record=True)")
    _compare(c["drawn"], c["r_drawn"], "wide run(deterministic=False)")
    # compact: the same bits except a dead row's row_actions
    for k in PER_STEP + PER_ROW + ("window", "partner_value", "partner_mask", "road_mask", "summary_tensor", "any_alive"):
        _same(getattr(epc, k), getattr(ep, k), "compact %s" % k)
    live = ~ep.dead
    _same(epc.row_actions[live], ep.row_actions[live], "compact row_actions of live rows")
    dead_before = ep.dead_mask.t()[:int(ep.steps)]
    if name == "removed":
        assert bool(dead_before.any()) and bool((~dead_before[-1]).any()), "no row is dead before a step: compact skips nothing"
        assert not torch.equal(epc.row_actions, ep.row_actions)  # a dead row keeps the action of the last step it was alive at
    want_count = (~ep.dead_mask).sum(0).to(torch.int32)
    want_count[int(ep.steps):] = 0
    _same(epc.live_count, want_count, "live_count")
    assert c["nbytes"] > 0


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_closed_loop_attention_scores(name):
    from tests.test_gpu_bc_rollout import PER_ROW, _same
    c = _loop_case(name)
    ep, at, N, A, R, pol = c["ep"], c["attn"], c["N"], c["A"], c["R"], c["pol"]
    for k in PER_ROW + ("window", "partner_value", "partner_mask", "road_mask", "summary_tensor", "any_alive", "row_actions"):
        _same(getattr(at, k), getattr(ep, k), "attention=True leaves %s alone" % k)
    _same(at.dead_mask, ep.dead_mask, "dead_mask")
    _same(c["attn_c"].ego_attn_score, at.ego_attn_score, "compact scores")
    assert tuple(at.ego_attn_score.shape) == (91, N, 4, A - 1)
    if name == "removed":
        assert any(bool(ep.dead_mask[:, t].any()) for t in c["chosen"]), "no chosen step has a dead row"
    for t in c["chosen"]:
        pre = c["prefix"][t]  # the window and masks the policy saw at step t
        pm = pre.partner_mask[:, None, :].expand(N, R, A - 1).contiguous()
        rm = pre.road_mask[:, None, :].expand(N, R, 200).contiguous()
        score = torch.empty((N, 4, A - 1), dtype=torch.float32, device="cuda")
        pol.context(pre.window.contiguous(), pm, rm, ego_attn_score=score)
        dead = ep.dead_mask[:, t]
        assert bool((~dead).any())
        _same(at.ego_attn_score[t][~dead], score[~dead], "scores of the rows live before step %d" % t)
        assert bool((at.ego_attn_score[t][dead] == 0).all()), "a dead row's scores at step %d" % t
    assert bool((at.ego_attn_score[int(ep.steps):] == 0).all())
    first, a, b = c["nosync"]
    _same(a.ego_attn_score, first.ego_attn_score, "no host synchronisation")
    _same(b.ego_attn_score, first.ego_attn_score, "no host synchronisation, compact")
