"""GPU suite: the device BC update (gpudrive_lab_amd.bc_opt.DeviceBC; gd_bc_train_rows, gd_bc_adamw, gd_bc_update).

The kernels are held to the host program of csrc/bc_opt_rule.hpp BIT FOR BIT (tests/test_bc_update.py holds that program to
torch in float64), the fused call to its four parts bit for bit, its gradient to `TrainableBCPolicy`'s bit for bit, and one
whole step to the float64 pipeline of the differentiable stand-in (tests/bc_update_reference.pipeline) within the bound
tests/test_gpu_bc_grad.py derives for a step, with the same K.  Small models: 64 agent slots, B in {1, 3, 8, 17},
R in {1, 5}; and of bc_cases.EDGE_CASES `top` (288 tensors: the optimiser's kernels past their first 256, and the update's
gradient in three chunks) and `defaults` (130 rows under the default chunk_rows and partials)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from tests import bc_cases as BC
from tests import bc_grad_reference as GR
from tests import bc_reference as REF
from tests import bc_update_reference as UR
from tests.test_bc_policy import case
from tests.test_gpu_bc_grad import K, _reference, _train
from tests.test_gpu_bc_policy import K as K_FORWARD
from tests.test_gpu_bc_policy import Carver, _dev, _no_sync, _yardstick

pytestmark = pytest.mark.gpu

SMALL = dict(chunk_rows=8, partials=3)


def _trainer(sd, A, R, cfg=BC.CFG, **kw):
    from gpudrive_lab_amd import DeviceBC
    return DeviceBC(sd, max_agents=A, num_stack=R, **cfg, **kw)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()


def _state(bc, n=0):
    """Everything an update writes, as bit patterns (the row scratch up to n rows)."""
    torch.cuda.synchronize()
    s = dict(flat=bc.flat, exp_avg=bc.exp_avg, exp_avg_sq=bc.exp_avg_sq, step=bc._step, beta_pow=bc._beta_pow, stats=bc.stats,
             stats_sum=bc.stats_sum, tensor_norms=bc.tensor_norms, max_grad_tensor=bc.max_grad_tensor, blob=bc.policy.blob,
             grad=bc.grad, actions=bc._actions[:n], nll=bc._nll[:n], grad_nll=bc._grad_nll[:n])
    return {k: _bits(v) for k, v in s.items()}


def _same(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _f32(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _assert_blob_follows(bc, what):
    lay = (bc.num_stack, bc.num_layer, bc.head_num_layers, bc.n_components)
    index = BP.pack_index(*lay)
    flat = bc.flat.cpu().numpy()
    assert flat[bc.G] == 0 and np.signbit(flat[bc.G]) == False, what + ": the trailing zero was written"  # noqa: E712
    blob = bc.policy.blob.cpu().numpy()
    assert np.array_equal(blob.view(np.int32), flat[index].view(np.int32)), what + ": blob != flat[pack_index]"
    assert (blob.view(np.int32)[index == bc.G] == 0).all(), what + ": a padding entry was written"


def _four_calls(bc, obs, expert, pm, rm):
    """gd_bc_update's four parts as four C calls on bc's own structs."""
    L, n = _capi.lib(), int(obs.shape[0])
    out = _capi.GdBCOutputs()
    out.actions, out.nll = bc._actions.data_ptr(), bc._nll.data_ptr()
    p, g, o = C.byref(bc._p), C.byref(bc._g), C.byref(bc._o)
    ex = expert.view(n, 3)
    _capi.check(L.gd_bc_forward(p, obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), n, 1, None, None, ex.data_ptr(), C.byref(out), None))
    _capi.check(L.gd_bc_train_rows(o, n, bc._nll.data_ptr(), bc._actions.data_ptr(), ex.data_ptr(), bc._grad_nll.data_ptr(), None))
    _capi.check(L.gd_bc_backward(p, g, obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), n, ex.data_ptr(), bc._grad_nll.data_ptr(), None,
                                 bc.grad.data_ptr(), None))
    _capi.check(L.gd_bc_adamw(o, bc.grad.data_ptr(), None))


def _case_tensors(B, A, R, cfg=BC.CFG):
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R, cfg)
    return sd, _dev(obs, expert, pm, rm)


# ---- the kernels against the host program

def test_adamw_three_steps_are_the_host_programs_bit_for_bit():
    """gd_bc_adamw on the synthetic gradients of test_bc_update.py (above 20 with one whole tensor of zeros, below 20, above
    20), uploaded as they are: every word the three launches write against the host program, after every step."""
    R = 1
    _adamw_three_steps(R, BC.CFG, BC.state_dict(R), UR.gradients(UR.layout(R)[1]), UR.zero_tensor(UR.layout(R)[1]))


def test_adamw_three_steps_at_288_tensors_are_the_host_programs_bit_for_bit():
    """bc_cases' `top` layout: 288 tensors, bc_opt_rule::MAX_TENSORS.  The tensor of zeros and the tensor of the largest norm
    both have an index >= 256, so max_grad_tensor, the clip norm and tensor_norms[256:] can only be the host program's if the
    workgroup of 256 made its second trip over the tensors."""
    _, _, R, cfg = BC.EDGE["top"]
    _, end, _ = UR.layout(R, cfg)
    grads, zt, largest = UR.top_gradients(end)
    assert len(end) == 288 and zt >= 256 and largest >= 256
    host = _adamw_three_steps(R, cfg, GR.state_dict(R, cfg), grads, zt)
    for h in host:
        assert h["max_grad_tensor"] == largest and (np.delete(h["tensor_norms"][256:], zt - 256) > 0).all()
        assert h["tensor_norms"][:256].max() < h["tensor_norms"][largest]


def _adamw_three_steps(R, cfg, sd, grads, zt):
    bc = _trainer(sd, 64, R, cfg, batch_size=4, **SMALL)
    names, end, G = UR.layout(R, cfg)
    assert names == bc._names and G == bc.G and np.array_equal(bc._tensor_end.cpu().numpy(), end)
    p0 = np.concatenate([sd[k].numpy().reshape(-1) for k in names])
    z = np.zeros(G, np.float32)
    host = UR.run_adamw_host(p0, z, z, grads, end, **UR.ADAMW)
    _assert_blob_follows(bc, "before")
    L, sums = _capi.lib(), np.zeros(2, np.float32)
    for s, g in enumerate(grads):
        what = "step %d" % (s + 1)
        g_dev, = _dev(g)
        _no_sync(lambda: _capi.check(L.gd_bc_adamw(C.byref(bc._o), g_dev.data_ptr(), None)))
        got, h = _state(bc), host[s]
        assert np.array_equal(got["flat"][:G], _f32(h["params"])), what + ": params"
        assert np.array_equal(got["exp_avg"], _f32(h["exp_avg"])) and np.array_equal(got["exp_avg_sq"], _f32(h["exp_avg_sq"])), what
        assert got["step"][0] == h["step"] == s + 1 and np.array_equal(got["beta_pow"], h["beta_pow"].view(np.int64)), what
        assert np.array_equal(got["tensor_norms"], _f32(h["tensor_norms"])), what + ": tensor_norms"
        assert np.array_equal(got["stats"][4:], _f32([h["total"], h["max_grad_norm"]])), what + ": stats[4..6)"
        assert (got["stats"][:4] == 0).all() and (got["stats_sum"][:4] == 0).all(), what + ": the rows' statistics were written"
        assert got["max_grad_tensor"][0] == h["max_grad_tensor"], what
        sums = sums + np.array([h["total"], h["max_grad_norm"]], np.float32)
        assert np.array_equal(got["stats_sum"][4:], sums.view(np.int32)), what + ": stats_sum[4..6)"
        _assert_blob_follows(bc, what)
    assert host[0]["total"] > 20 and host[1]["total"] < 20 and host[0]["tensor_norms"][zt] == 0
    # the scalars the last launch read
    scal = bc._scal.cpu().numpy()
    assert scal[0] == host[2]["total"] and scal[1] == np.float32(20.0) / (host[2]["total"] + np.float32(1e-6))
    sq = scal[4:].view(np.float64)
    assert sq.shape == (len(end),) and np.array_equal(np.sqrt(sq.astype(np.float32)), host[2]["tensor_norms"])
    return host


@pytest.mark.parametrize("n", UR.ROWS)
def test_train_rows_are_the_host_programs_bit_for_bit(n):
    bc = _trainer(GR.state_dict(1, GR.MINIMAL), 64, 1, GR.MINIMAL, batch_size=4, **SMALL)
    nll, actions, expert = UR.row_inputs(n)
    want, w = UR.run_rows_host(nll, actions, expert)
    carver = Carver()
    grad_nll = carver.carve("grad_nll", (n,))
    d_nll, d_act, d_ex = _dev(nll, actions, expert)
    L = _capi.lib()
    for call in (1, 2):
        _no_sync(lambda: _capi.check(L.gd_bc_train_rows(C.byref(bc._o), n, d_nll.data_ptr(), d_act.data_ptr(), d_ex.data_ptr(),
                                                         grad_nll.data_ptr(), None)))
        torch.cuda.synchronize()
        carver.assert_guards("gd_bc_train_rows n = %d" % n)
        assert np.array_equal(_bits(grad_nll), _f32(w))
        got = _state(bc)
        assert np.array_equal(got["stats"][:4], _f32(want)), (n, got["stats"][:4].view(np.float32), want)
        total = want if call == 1 else want + want   # (float32: x + x is exact)
        assert np.array_equal(got["stats_sum"][:4], _f32(total)) and (got["stats_sum"][4:] == 0).all() and (got["stats"][4:] == 0).all()
    assert got["step"][0] == 0 and (bc.exp_avg == 0).all()


# ---- the fused call

def test_the_updates_gradient_is_the_trainable_policys_bit_for_bit():
    for B, A, R in ((17, 64, 5), (3, 64, 1)):
        _same_gradient_bits(B, A, R, BC.CFG, 32, SMALL)


@pytest.mark.parametrize("name", ["top", "defaults"])
def test_the_updates_gradient_at_the_edge_configurations(name):
    """`top` with three chunks; `defaults` with the chunk_rows and partials every caller gets (128 each) and 130 rows."""
    B, A, R, cfg = BC.EDGE[name]
    bc, tbp = _same_gradient_bits(B, A, R, cfg, B, dict(chunk_rows=2, partials=3) if name == "top" else {})
    if name == "defaults":
        assert bc.policy.chunk_rows == tbp.chunk_rows == BP.DEFAULT_CHUNK == 128 and bc._g.num_partials == tbp.partials == 128 < B


def _same_gradient_bits(B, A, R, cfg, batch_size, kw):
    sd, (obs, expert, pm, rm) = _case_tensors(B, A, R, cfg)
    bc = _trainer(sd, A, R, cfg, batch_size=batch_size, **kw)
    tbp = _train(sd, A, R, cfg, **kw)
    bc.update(obs, expert, pm, rm)
    tbp(obs, pm, rm, expert).mean().backward()
    flat = torch.cat([p.grad.reshape(-1) for p in tbp.parameters()])
    assert [k for k, _ in tbp.named_parameters()] == list(bc._names)
    assert np.array_equal(_bits(bc.grad), _bits(flat)), (B, A, R)
    assert np.abs(bc.grad.cpu().numpy()).max() > 0
    return bc, tbp


def test_update_is_the_four_calls_bit_for_bit():
    """B = 17 with chunk_rows = 8 (three chunks, a short last one), then B = 3 on the same objects (a short last batch): the
    fused call without a synchronisation or an allocation, against the four C calls, and against itself from the same state."""
    A, R = 64, 5
    sd, big = _case_tensors(17, A, R)
    _, small = _case_tensors(5, A, R)
    small = [t[:3].contiguous() for t in small]
    fused, parts, again = (_trainer(sd, A, R, batch_size=17, **SMALL) for _ in range(3))
    G, end, f32 = fused.G, fused._tensor_end.cpu().numpy(), np.float32
    prev = _state(fused)
    for what, (obs, expert, pm, rm) in (("B = 17", big), ("B = 3", small)):
        n = int(obs.shape[0])
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        _no_sync(lambda: fused.update(obs, expert, pm, rm))
        assert torch.cuda.memory_allocated() == before, what + ": the update allocated"
        _four_calls(parts, obs, expert, pm, rm)
        again.update(obs, expert, pm, rm)
        a = _state(fused, n)
        _same(a, _state(parts, n), what + " against the four calls")
        _same(a, _state(again, n), what + " twice from the same state")
        _assert_blob_follows(fused, what)
        assert np.isfinite(a["flat"].view(f32)).all() and (a["grad_nll"].view(f32) == f32(1) / f32(n)).all()
        # the optimiser step is the host program's on the gradient the device computed, read back
        host, = UR.run_adamw_host(prev["flat"][:G].view(f32), prev["exp_avg"].view(f32), prev["exp_avg_sq"].view(f32),
                                  [a["grad"].view(f32)], end, step=int(prev["step"][0]), beta_pow=prev["beta_pow"].view(np.float64),
                                  **UR.ADAMW)
        assert np.array_equal(a["flat"][:G], _f32(host["params"])) and np.array_equal(a["exp_avg"], _f32(host["exp_avg"])), what
        assert np.array_equal(a["exp_avg_sq"], _f32(host["exp_avg_sq"])) and a["step"][0] == host["step"], what
        assert np.array_equal(a["beta_pow"], host["beta_pow"].view(np.int64)), what
        assert np.array_equal(a["tensor_norms"], _f32(host["tensor_norms"])), what
        assert np.array_equal(a["stats"][4:], _f32([host["total"], host["max_grad_norm"]])), what
        assert a["max_grad_tensor"][0] == host["max_grad_tensor"], what
        # and the rows' statistics the host program's on the forward's outputs, read back
        want, _ = UR.run_rows_host(a["nll"].view(f32), a["actions"].view(f32), expert.cpu().numpy().reshape(n, 3))
        assert np.array_equal(a["stats"][:4], _f32(want)), what
        prev = a
    assert fused._updates == 2 and prev["step"][0] == 2


def test_one_update_against_the_float64_pipeline():
    """The bound of test_gpu_bc_grad.test_one_training_step_against_float64 (its docstring derives it), with its K, on the
    same case; and the step's statistics within the forward tests' K E of float64."""
    B, A, R = 3, 64, 1
    c = _reference(B, A, R, BC.CFG, "mean")
    want, losses = UR.pipeline(c, A, BC.CFG)
    bc = _trainer(c["sd"], A, R, batch_size=B, **SMALL)
    obs, expert, pm, rm = _dev(c["obs"], c["expert"], c["pm"], c["rm"])
    bc.update(obs, expert, pm, rm)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in bc.state_dict().items()}
    lr, eps = UR.ADAMW["lr"], UR.ADAMW["eps"]
    d = {k: K * c["E"][k] for k in c["g64"]}
    norm = np.sqrt(sum(float((g * g).sum()) for g in c["g64"].values()))
    s = min(1.0, 20.0 / (norm + 1e-6))
    dnorm = np.sqrt(sum(g.size * d[k] ** 2 for k, g in c["g64"].items()))
    assert list(got) == list(want)
    for k in want:
        p0 = c["sd"][k].double().numpy()
        bound = lr * (s * d[k] + np.abs(c["g64"][k]) * s * dnorm / norm) / eps + 8 * 2.0 ** -24 * (np.abs(p0) + lr)
        err = np.abs(got[k] - want[k])
        print("BCUPDATE STEP %s err/bound %.3f" % (k, float((err / bound).max())))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        assert np.abs(want[k] - p0).max() > 0 and np.abs(got[k] - p0).max() > 0, (k, "did not move")
    # the statistics: loss and the three action errors of the weights before the step
    f = case(B, A, R)
    assert np.array_equal(f["obs"], c["obs"]) and np.array_equal(f["expert"][:, 0], c["expert"]), "the forward tests' case"
    E = _yardstick(f, A)
    w = np.sort(f["ref"]["weights"], -1)
    assert (w[:, -1] - w[:, -2] > 1e-3).all(), "no float32 rounding can change the deterministic component"
    _, act = REF.deterministic_action(f["ref"]["means"], f["ref"]["weights"])
    ref = np.concatenate([[f["ref_nll"].mean()], np.abs(act - c["expert"]).mean(0)])
    assert abs(ref[0] - losses[0]) <= 1e-9 * abs(ref[0]), "the two float64 restatements agree on the loss"
    stats = bc.stats.cpu().numpy().astype(np.float64)
    for i, name in enumerate(UR.STATS):
        bound = K_FORWARD * (E["nll"] if i == 0 else E["means"])
        print("BCUPDATE STAT %s got %.6f want %.6f err/bound %.3f" % (name, stats[i], ref[i], abs(stats[i] - ref[i]) / bound))
        assert abs(stats[i] - ref[i]) <= bound, (name, stats[i], ref[i], bound)
    assert abs(stats[4] - norm) <= dnorm + 2.0 ** -22 * norm, "grad_norm is the norm before clipping (the norm is 1-Lipschitz)"
    out = bc.losses()
    n64 = {k: float(np.sqrt((g * g).sum())) for k, g in c["g64"].items()}
    assert n64[out["max_grad_name"]] >= max(n64.values()) - 2 * max(np.sqrt(g.size) * d[k] for k, g in c["g64"].items())
    # (the coefficient moves by at most s dnorm / norm, the largest norm by at most dnorm, and it is at most norm)
    assert abs(stats[5] - s * max(n64.values())) <= 2 * s * dnorm + 2.0 ** -21 * s * max(n64.values())
    assert out["loss"] == pytest.approx(ref[0], rel=1e-3) and out["grad_norm"] == pytest.approx(norm, rel=1e-3)


def test_the_policy_follows_the_optimiser_in_place():
    A, R = 64, 5
    sd, (obs, expert, pm, rm) = _case_tensors(5, A, R)
    bc = _trainer(sd, A, R, batch_size=8, **SMALL)
    ptr = bc.policy.blob.data_ptr()
    before = bc.policy.nll(obs, pm, rm, expert)
    for _ in range(2):
        bc.update(obs, expert, pm, rm)
    assert bc.policy.blob.data_ptr() == ptr
    fresh = BP.DeviceBCPolicy.from_state_dict(bc.state_dict(), max_agents=A, num_stack=R, chunk_rows=8, **BC.CFG)
    want = ("nll", "actions")
    a = bc.policy.forward(obs, pm, rm, want, deterministic=True, expert_actions=expert)
    b = fresh.forward(obs, pm, rm, want, deterministic=True, expert_actions=expert)
    for k in want:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert not np.array_equal(_bits(a["nll"]), _bits(before)), "the weights moved"
    assert np.array_equal(_bits(bc.policy.blob), _bits(fresh.blob))
    sd2 = bc.state_dict()
    assert list(sd2) == list(sd) and all(sd2[k].shape == sd[k].shape for k in sd)
    ev = bc.evaluate([(obs, expert, pm, rm, None)])
    assert ev["test_loss"] == pytest.approx(float(a["nll"].mean()), rel=1e-5)


# ---- the loop

def _tiny_dataset(A=64, samples=7):
    """Two recorded rows of which `samples` (row, time) pairs are alive: that many samples at rollout_len 1, pred_len 1."""
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    rng = np.random.default_rng(21)
    N, T, D = 2, 91, BP.obs_width(A)
    dead = np.ones((N, T), bool)
    alive = [(0, 3), (0, 4), (0, 40), (1, 0), (1, 17), (1, 18), (1, 90)][:samples]
    for n, t in alive:
        dead[n, t] = False
    ep = dict(obs=rng.normal(0.0, 1.0, (N, T, D)).astype(np.float32),
              actions=(rng.uniform(-1.0, 1.0, (N, T, 3)) * np.array([4.0, 0.4, 0.15])).astype(np.float32), dead_mask=dead,
              partner_mask=rng.integers(0, 3, (N, T, A - 1)).astype(np.uint8), road_mask=rng.random((N, T, 200)) < 0.3,
              keep=np.ones(N, bool))
    ds = DeviceExpertDataset({k: torch.from_numpy(v).cuda() for k, v in ep.items()}, rollout_len=1, pred_len=1)
    assert len(ds) == samples
    return ds


def test_fit_is_the_hand_written_loop_bit_for_bit():
    """Seven samples in batches of three (3, 3, 1: a short last batch), five steps: the loop stops after the second batch of
    the second epoch."""
    A, R, steps = 64, 1, 5
    ds = _tiny_dataset(A)
    sd = GR.state_dict(R, GR.MINIMAL)
    a, b = (_trainer(sd, A, R, GR.MINIMAL, batch_size=3, **SMALL) for _ in range(2))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    assert a.fit(ds, steps, generator=gen) == steps
    gen.manual_seed(5)
    made, sizes = 0, []
    while made < steps:
        for obs, expert, pm, rm, _ in ds.batches(3, shuffle=True, generator=gen):
            if made >= steps:
                break
            b.update(obs, expert, pm, rm)
            made += 1
            sizes.append(int(obs.shape[0]))
    assert sizes == [3, 3, 1, 3, 3]
    _same(_state(a), _state(b), "fit against the loop", skip=("actions", "nll", "grad_nll"))
    assert int(a._step.item()) == steps and int(ds.bad_indices.item()) == 0
    sums = a.stats_sum.cpu().numpy().astype(np.float64)
    last = int(a.max_grad_tensor.item())
    reads = a.host_reads
    real, counted = torch.Tensor.cpu, []

    def cpu(t, *args, **kw):   # the one read is let through; any other synchronisation inside losses() raises
        torch.cuda.set_sync_debug_mode(0)
        counted.append(1)
        try:
            return real(t, *args, **kw)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    torch.cuda.synchronize()
    torch.Tensor.cpu = cpu
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = a.losses()
    finally:
        torch.cuda.set_sync_debug_mode(0)
        torch.Tensor.cpu = real
    assert len(counted) == 1, "losses() reads the device once"
    assert a.host_reads == reads + 1
    assert list(out) == list(_capi.BC_STATS) + ["max_grad_name"] and out["max_grad_name"] == a._names[last]
    for k, v in zip(_capi.BC_STATS, sums):
        assert out[k] == v / steps and np.isfinite(out[k]), k
    assert out["grad_norm"] > 0 and out["max_grad_norm"] > 0 and out["max_grad_norm"] <= min(out["grad_norm"], 20.0) * (1 + 1e-6)
    again = a.losses()
    assert all(again[k] == 0 for k in _capi.BC_STATS) and again["max_grad_name"] == out["max_grad_name"]
    assert a.fit(ds, 0) == 0 and int(a._step.item()) == steps
    with pytest.raises(ValueError, match="batch_size"):
        a.update(*[t for t in next(iter(ds.batches(4, shuffle=False)))[:4]])


def test_twenty_steps_lower_the_loss():
    """The fixed batch of test_gpu_bc_grad.test_twenty_steps_lower_the_loss (8 rows; the float64 CPU run of the same twenty
    steps ends lower for that seed, 45.61 -> 1.35)."""
    A, R = 64, 5
    sd, (obs, expert, pm, rm) = _case_tensors(8, A, R)
    bc = _trainer(sd, A, R, batch_size=8, chunk_rows=8, partials=16)
    losses = []
    for _ in range(20):
        bc.update(obs, expert, pm, rm)
        losses.append(bc.stats[0].clone())
    losses.append(bc.policy.nll(obs, pm, rm, expert).mean())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print("BCUPDATE LOSSES", " ".join("%.4f" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert bc.losses()["loss"] == pytest.approx(np.mean(losses[:20]), rel=1e-5)


# ---- the optimiser state

def _torch_step(tbp, opt, obs, expert, pm, rm):
    opt.zero_grad()
    tbp(obs, pm, rm, expert).mean().backward()
    torch.nn.utils.clip_grad_norm_(tbp.parameters(), 20)
    opt.step()


def _assert_one_step_apart(bc, tbp, what):
    """One optimiser step on the SAME gradient bits by both sides: what differs is float32's rounding of the update itself
    and of the clip coefficient, a relative 2^-23 of gc that changes m / (sqrt(v) + eps) by that fraction of its value, which
    is at most 1.004 within the first three steps (Cauchy-Schwarz on the two moments' weights).  The bound is the rounding term of the
    one-step bound: 8 * 2^-24 (|p| + lr)."""
    mine = bc.state_dict()
    for k, p in tbp.named_parameters():
        a, b = mine[k].cpu().numpy().astype(np.float64), p.detach().cpu().numpy().astype(np.float64)
        bound = 8 * 2.0 ** -24 * (np.abs(b) + bc.learning_rate)
        assert (np.abs(a - b) <= bound).all(), (what, k, float((np.abs(a - b) / bound).max()))


def test_the_optimiser_state_round_trips_with_torch_adamw():
    A, R = 64, 1
    sd, (obs, expert, pm, rm) = _case_tensors(3, A, R)
    bc = _trainer(sd, A, R, batch_size=3, **SMALL)
    bc.update(obs, expert, pm, rm)
    # DeviceBC -> torch
    tbp = _train(bc.state_dict(), A, R, **SMALL)
    opt = torch.optim.AdamW(tbp.parameters(), lr=1e-3, eps=1e-4, weight_decay=0.5)
    osd = bc.optimizer_state_dict()
    opt.load_state_dict(osd)
    group = opt.param_groups[0]
    assert group["lr"] == 5e-4 and group["weight_decay"] == 0.01 and group["eps"] == 1e-4 and group["betas"] == (0.9, 0.999)
    assert not group["amsgrad"]
    o = 0
    for p in tbp.parameters():
        st = opt.state[p]
        assert float(st["step"]) == 1
        for name, mine in (("exp_avg", bc.exp_avg), ("exp_avg_sq", bc.exp_avg_sq)):
            assert np.array_equal(_bits(st[name]).reshape(-1), _bits(mine[o:o + p.numel()])), name
        o += p.numel()
    assert o == bc.G
    _torch_step(tbp, opt, obs, expert, pm, rm)
    bc.update(obs, expert, pm, rm)
    _assert_one_step_apart(bc, tbp, "DeviceBC -> torch")
    # torch -> DeviceBC: another learning rate and weight decay travel with the state
    for g in opt.param_groups:
        g["lr"], g["weight_decay"] = 2e-4, 0.02
    other = _trainer(tbp.state_dict(), A, R, batch_size=3, **SMALL)
    other.load_optimizer_state_dict(opt.state_dict())
    assert int(other._step.item()) == 2 and other.learning_rate == 2e-4 and other.weight_decay == 0.02
    assert float(other._lr.item()) == np.float32(2e-4) and other._o.weight_decay == np.float32(0.02)
    assert np.array_equal(other._beta_pow.cpu().numpy(), np.array([0.9 * 0.9, 0.999 * 0.999]))
    back = other.optimizer_state_dict()
    assert back["param_groups"][0]["lr"] == 2e-4 and back["param_groups"][0]["weight_decay"] == 0.02
    for i, p in enumerate(tbp.parameters()):
        for name in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(_bits(back["state"][i][name]), _bits(opt.state[p][name])), (i, name)
        assert float(back["state"][i]["step"]) == 2
    _torch_step(tbp, opt, obs, expert, pm, rm)
    other.update(obs, expert, pm, rm)
    _assert_one_step_apart(other, tbp, "torch -> DeviceBC")
    # an empty state is a fresh optimiser
    other.load_optimizer_state_dict(torch.optim.AdamW(tbp.parameters(), lr=5e-4, eps=1e-4).state_dict())
    assert int(other._step.item()) == 0 and (other.exp_avg == 0).all() and (other._beta_pow == 1).all()
    with pytest.raises(ValueError):
        other.load_optimizer_state_dict(torch.optim.AdamW(tbp.parameters(), lr=5e-4, eps=1e-4, amsgrad=True).state_dict())
