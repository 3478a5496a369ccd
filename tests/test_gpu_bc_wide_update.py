"""GPU suite: the device BC update at network_dim 128 (gpudrive_lab_amd.bc_opt.DeviceBCDim; gd_bc_adamw_dim, gd_bc_update_dim) on
the cases of tests/bc_wide_cases.py.

As at 64 (tests/test_gpu_bc_update.py): the optimiser's kernels are held to the host program of csrc/bc_opt_rule.hpp BIT FOR BIT
on the sweep's layout (1.4 M parameters, 252 tensors; tests/test_bc_wide_update.py holds that program to torch in float64
there), the fused call to its four parts bit for bit, its gradient to `TrainableBCPolicyDim`'s bit for bit, and one whole step
to the float64 pipeline of the differentiable restatement at that width (tests/bc_wide_update_reference.pipeline) within the
bound tests/test_gpu_bc_grad.py derives for a step, with the wide backward's yardstick (K = 32, E_p of
tests/bc_wide_grad_reference.py).  tests/test_gpu_bc_wide_edges.py runs `_one_update_against_the_float64_pipeline` and
`_update_against_its_parts` at wide_top (288 tensors: the optimiser's kernels past their first 256; at most 0.11 of the step's
bound) and `DeviceBCDim` with every default on wide_defaults' 130 rows."""
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
from tests import bc_wide_cases as WC
from tests import bc_wide_grad_reference as WGR
from tests import bc_wide_update_reference as WUR
from tests.test_gpu_bc_grad import K
from tests.test_gpu_bc_policy import CANARY_BITS, GUARD, Carver, _dev, _no_sync
from tests.test_gpu_bc_wide import K as K_FORWARD

pytestmark = pytest.mark.gpu

SMALL = dict(chunk_rows=8, partials=3)


def _trainer(c, **kw):
    from gpudrive_lab_amd.bc_opt import DeviceBCDim
    return DeviceBCDim(c["sd"], max_agents=c["A"], num_stack=c["R"], network_dim=WC.DIM, **c["cfg"], **kw)


def _train(c, sd=None, **kw):
    from gpudrive_lab_amd import TrainableBCPolicyDim
    return TrainableBCPolicyDim.from_state_dict(c["sd"] if sd is None else sd, max_agents=c["A"], num_stack=c["R"], device="cuda",
                                                network_dim=WC.DIM, **c["cfg"], **kw)


def _inputs(c):
    """obs, expert, pm, rm on the device, in `update`'s order."""
    return _dev(c["obs"], c["expert"], c["pm"], c["rm"])


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


def _index(bc):
    return BP.pack_index(bc.num_stack, bc.num_layer, bc.head_num_layers, bc.n_components, network_dim=bc.network_dim)


def _assert_blob_follows(bc, what, padding=0):
    """The blob, gathered through the layout, is the flat weights; its padding words hold `padding`'s bits."""
    index = _index(bc)
    flat = bc.flat.cpu().numpy()
    assert flat[bc.G] == 0 and np.signbit(flat[bc.G]) == False, what + ": the trailing zero was written"  # noqa: E712
    blob = bc.policy.blob.cpu().numpy().view(np.int32)
    real = index != bc.G
    assert np.array_equal(blob[real], flat.view(np.int32)[index[real]]), what + ": blob != flat[pack_index]"
    assert (blob[~real] == padding).all(), what + ": a padding entry was written"


def _four_calls(bc, obs, expert, pm, rm):
    """gd_bc_update_dim's four parts as four C calls on bc's own structs."""
    L, n = _capi.lib(), int(obs.shape[0])
    out = _capi.GdBCOutputs()
    out.actions, out.nll = bc._actions.data_ptr(), bc._nll.data_ptr()
    p, g, o = C.byref(bc._pd), C.byref(bc._g), C.byref(bc._o)
    ex = expert.view(n, 3)
    _capi.check(L.gd_bc_forward_dim(p, obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), n, 1, None, None, ex.data_ptr(), C.byref(out), None))
    _capi.check(L.gd_bc_train_rows(o, n, bc._nll.data_ptr(), bc._actions.data_ptr(), ex.data_ptr(), bc._grad_nll.data_ptr(), None))
    _capi.check(L.gd_bc_backward_dim(p, g, obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), n, ex.data_ptr(), bc._grad_nll.data_ptr(), None,
                                     bc.grad.data_ptr(), None))
    _capi.check(L.gd_bc_adamw_dim(o, bc.network_dim, bc.grad.data_ptr(), None))


# ---- the optimiser's kernels against the host program

def test_adamw_dim_three_steps_at_the_sweeps_layout_are_the_host_programs_bit_for_bit():
    """gd_bc_adamw_dim at 128 on the planted gradients of test_bc_wide_update.py (the largest tensor, 24,576 floats, has the
    largest norm; one whole tensor of zeros), uploaded as they are: every word the three launches write against the host
    program after every step, the blob against the flat weights, and a pattern planted in the blob's padding words."""
    c = WGR.case_inputs("wide_sweep")
    c = dict(sd=c[0], A=c[6], R=WC.CASES["wide_sweep"][2], cfg=c[7])
    bc = _trainer(c, batch_size=4, chunk_rows=2, partials=1)
    names, end, G = WUR.layout("wide_sweep")
    assert bc.network_dim == 128 and names == bc._names and G == bc.G == WUR.SWEEP_G and len(end) == WUR.SWEEP_T
    assert np.array_equal(bc._tensor_end.cpu().numpy(), end)
    grads, zt, largest = WUR.planted_gradients("wide_sweep")
    p0 = WUR.flat_params(c["sd"], names)
    z = np.zeros(G, np.float32)
    host = UR.run_adamw_host(p0, z, z, grads, end, **UR.ADAMW)
    _assert_blob_follows(bc, "before")
    pad = torch.from_numpy(np.flatnonzero(_index(bc) == G)).cuda()
    assert pad.numel() > 0 and pad.numel() == bc.policy.blob.numel() - G
    bc.policy.blob.view(torch.int32)[pad] = CANARY_BITS
    L, sums = _capi.lib(), np.zeros(2, np.float32)
    for s, g in enumerate(grads):
        what = "step %d" % (s + 1)
        g_dev, = _dev(g)
        _no_sync(lambda: _capi.check(L.gd_bc_adamw_dim(C.byref(bc._o), 128, g_dev.data_ptr(), None)))
        got, h = _state(bc), host[s]
        assert np.array_equal(got["flat"][:G], _f32(h["params"])), what + ": params"
        assert np.array_equal(got["exp_avg"], _f32(h["exp_avg"])) and np.array_equal(got["exp_avg_sq"], _f32(h["exp_avg_sq"])), what
        assert got["step"][0] == h["step"] == s + 1 and np.array_equal(got["beta_pow"], h["beta_pow"].view(np.int64)), what
        assert np.array_equal(got["tensor_norms"], _f32(h["tensor_norms"])), what + ": tensor_norms"
        assert np.array_equal(got["stats"][4:], _f32([h["total"], h["max_grad_norm"]])), what + ": stats[4..6)"
        assert (got["stats"][:4] == 0).all() and (got["stats_sum"][:4] == 0).all(), what + ": the rows' statistics were written"
        assert got["max_grad_tensor"][0] == h["max_grad_tensor"] == largest, what
        sums = sums + np.array([h["total"], h["max_grad_norm"]], np.float32)
        assert np.array_equal(got["stats_sum"][4:], sums.view(np.int32)), what + ": stats_sum[4..6)"
        _assert_blob_follows(bc, what, padding=np.int32(CANARY_BITS))
    assert host[0]["total"] > 20 and host[1]["total"] < 20 and host[0]["tensor_norms"][zt] == 0
    # the same struct is refused by the 64-wide entry, and by this one at 64
    assert L.gd_bc_adamw(C.byref(bc._o), g_dev.data_ptr(), None) == _capi.GD_ERR_INVALID
    assert L.gd_bc_adamw_dim(C.byref(bc._o), 64, g_dev.data_ptr(), None) == _capi.GD_ERR_INVALID
    assert np.array_equal(_state(bc)["flat"], got["flat"]) and int(bc._step.item()) == 3


# ---- the fused call

def _update_against_its_parts(name, **kw):
    """Two consecutive updates: the fused call against the four C calls and against itself from the same state, bit for bit;
    its gradient against `TrainableBCPolicyDim`'s on the weights before each update; the optimiser step against the host
    program on the gradient the device computed.  Returns the state after the first update."""
    c = WGR.case(name)
    B = len(c["obs"])
    obs, expert, pm, rm = _inputs(c)
    fused, parts, again = (_trainer(c, batch_size=B, **kw) for _ in range(3))
    assert fused._wide and fused._pd.network_dim == 128
    G, end, f32 = fused.G, fused._tensor_end.cpu().numpy(), np.float32
    prev, first = _state(fused), None
    for what in ("first update", "second update"):
        tbp = _train(c, sd=fused.state_dict(), **kw)
        tbp(obs, pm, rm, expert).mean().backward()
        want = torch.cat([p.grad.reshape(-1) for p in tbp.parameters()])
        assert [k for k, _ in tbp.named_parameters()] == list(fused._names)
        _no_sync(lambda: fused.update(obs, expert, pm, rm))
        _four_calls(parts, obs, expert, pm, rm)
        again.update(obs, expert, pm, rm)
        a = _state(fused, B)
        _same(a, _state(parts, B), "%s %s against the four calls" % (name, what))
        _same(a, _state(again, B), "%s %s twice from the same state" % (name, what))
        assert np.array_equal(a["grad"], _bits(want)), "%s %s: the gradient is not TrainableBCPolicyDim's" % (name, what)
        assert np.abs(a["grad"].view(f32)).max() > 0 and np.isfinite(a["flat"].view(f32)).all()
        assert (a["grad_nll"].view(f32) == f32(1) / f32(B)).all()
        _assert_blob_follows(fused, what)
        host, = UR.run_adamw_host(prev["flat"][:G].view(f32), prev["exp_avg"].view(f32), prev["exp_avg_sq"].view(f32),
                                  [a["grad"].view(f32)], end, step=int(prev["step"][0]), beta_pow=prev["beta_pow"].view(np.float64),
                                  **UR.ADAMW)
        assert np.array_equal(a["flat"][:G], _f32(host["params"])) and np.array_equal(a["exp_avg"], _f32(host["exp_avg"])), what
        assert np.array_equal(a["exp_avg_sq"], _f32(host["exp_avg_sq"])) and a["step"][0] == host["step"], what
        assert np.array_equal(a["tensor_norms"], _f32(host["tensor_norms"])), what
        assert np.array_equal(a["stats"][4:], _f32([host["total"], host["max_grad_norm"]])), what
        assert a["max_grad_tensor"][0] == host["max_grad_tensor"], what
        rows, _ = UR.run_rows_host(a["nll"].view(f32), a["actions"].view(f32), c["expert"].reshape(B, 3))
        assert np.array_equal(a["stats"][:4], _f32(rows)), what
        prev, first = a, first or a
    assert fused._updates == 2 and prev["step"][0] == 2
    return first


def test_update_is_its_four_parts_bit_for_bit_on_wide_min():
    _update_against_its_parts("wide_min", **SMALL)


def test_update_is_its_four_parts_bit_for_bit_in_several_chunks():
    """wide_chunks, five rows: chunk_rows 2 (three chunks, a short last one) against chunk_rows 8 (one), four partials.  The
    rows' outputs and statistics do not depend on the chunking (the forward's per-row bits do not)."""
    two = _update_against_its_parts("wide_chunks", chunk_rows=2, partials=4)
    eight = _update_against_its_parts("wide_chunks", chunk_rows=8, partials=4)
    for k in ("actions", "nll", "grad_nll"):
        assert np.array_equal(two[k], eight[k]), k
    assert np.array_equal(two["stats"][:4], eight["stats"][:4])


def test_one_update_against_the_float64_pipeline():
    """tests/test_gpu_bc_update.py's test and bound (tests/test_gpu_bc_grad.py derives it) on wide_min with the wide backward's
    yardstick, d = K E_p; the step's statistics within the wide forward tests' K E of float64."""
    _one_update_against_the_float64_pipeline("wide_min", **SMALL)


def _one_update_against_the_float64_pipeline(name, **kw):
    c = WGR.case(name, "mean")
    B = len(c["obs"])
    want, losses = WUR.pipeline(c)
    bc = _trainer(c, batch_size=B, **kw)
    bc.update(*_inputs(c))
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
        print("BCWIDEUPDATE STEP %s err/bound %.3f" % (k, float((err / bound).max())))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        assert np.abs(want[k] - p0).max() > 0 and np.abs(got[k] - p0).max() > 0, (k, "did not move")
    # the statistics: loss and the three action errors of the weights before the step
    f = WC.case(name)
    assert np.array_equal(f["obs"], c["obs"]) and np.array_equal(f["expert"][:, 0], c["expert"]), "the forward tests' case"
    E = f["E"]
    if c["cfg"]["n_components"] > 1:
        w = np.sort(f["ref"]["weights"], -1)
        assert (w[:, -1] - w[:, -2] > 1e-3).all(), "no float32 rounding can change the deterministic component"
    _, act = REF.deterministic_action(f["ref"]["means"], f["ref"]["weights"])
    ref = np.concatenate([[f["ref"]["nll"].mean()], np.abs(act - c["expert"]).mean(0)])
    assert abs(ref[0] - losses[0]) <= 1e-9 * abs(ref[0]), "the two float64 restatements agree on the loss"
    stats = bc.stats.cpu().numpy().astype(np.float64)
    for i, stat in enumerate(UR.STATS):
        bound = K_FORWARD * (E["nll"] if i == 0 else E["means"])
        print("BCWIDEUPDATE STAT %s got %.6f want %.6f err/bound %.3f" % (stat, stats[i], ref[i], abs(stats[i] - ref[i]) / bound))
        assert abs(stats[i] - ref[i]) <= bound, (stat, stats[i], ref[i], bound)
    assert abs(stats[4] - norm) <= dnorm + 2.0 ** -22 * norm, "grad_norm is the norm before clipping (the norm is 1-Lipschitz)"
    out = bc.losses()
    n64 = {k: float(np.sqrt((g * g).sum())) for k, g in c["g64"].items()}
    assert n64[out["max_grad_name"]] >= max(n64.values()) - 2 * max(np.sqrt(g.size) * d[k] for k, g in c["g64"].items())
    # (the coefficient moves by at most s dnorm / norm, the largest norm by at most dnorm, and it is at most norm)
    assert abs(stats[5] - s * max(n64.values())) <= 2 * s * dnorm + 2.0 ** -21 * s * max(n64.values())
    assert out["loss"] == pytest.approx(ref[0], rel=1e-3) and out["grad_norm"] == pytest.approx(norm, rel=1e-3)


def test_the_policy_follows_the_optimiser_in_place():
    c = WGR.case("wide_sweep")
    obs, expert, pm, rm = _inputs(c)
    bc = _trainer(c, batch_size=8, chunk_rows=2, partials=3)
    assert bc.policy.network_dim == 128 and bc.policy.blob.numel() == bc._o.blob_floats
    ptr = bc.policy.blob.data_ptr()
    before = bc.policy.nll(obs, pm, rm, expert)
    for _ in range(2):
        bc.update(obs, expert, pm, rm)
    assert bc.policy.blob.data_ptr() == ptr == bc._o.blob == bc._pd.base.blob
    fresh = BP.DeviceBCPolicy.from_state_dict(bc.state_dict(), max_agents=c["A"], num_stack=c["R"], chunk_rows=2, network_dim=128,
                                              **c["cfg"])
    a, b = bc.policy.nll(obs, pm, rm, expert), fresh.nll(obs, pm, rm, expert)
    assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(_bits(a), _bits(before)), "the weights moved"
    assert np.array_equal(_bits(bc.policy.blob), _bits(fresh.blob))
    sd2 = bc.state_dict()
    assert list(sd2) == list(c["sd"]) and all(sd2[k].shape == c["sd"][k].shape for k in sd2)
    ev = bc.evaluate([(obs, expert, pm, rm, None)])
    assert ev["test_loss"] == pytest.approx(float(a.mean()), rel=1e-5)


def test_a_64_wide_instance_is_device_bc_bit_for_bit():
    from gpudrive_lab_amd.bc_opt import DeviceBC, DeviceBCDim
    B, A, R = 3, 64, 1
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R)
    t = _dev(obs, expert, pm, rm)
    kw = dict(max_agents=A, num_stack=R, batch_size=B, **BC.CFG, **SMALL)
    plain, dim, said = DeviceBC(sd, **kw), DeviceBCDim(sd, **kw), DeviceBCDim(sd, network_dim=64, **kw)
    assert not dim._wide and dim._pd is None and dim.network_dim == said.network_dim == 64 and dim.nbytes == plain.nbytes
    for n in (1, 2):
        for bc in (plain, dim, said):
            bc.update(*t)
        a = _state(plain, B)
        _same(a, _state(dim, B), "update %d" % n)
        _same(a, _state(said, B), "update %d, network_dim=64 said" % n)
    assert a["step"][0] == 2 and np.abs(a["grad"].view(np.float32)).max() > 0


# ---- buffers and synchronisation

def _guards(carver, what):
    for name, (buf, words) in carver.whole.items():
        h = buf.cpu().numpy()
        assert (h[:GUARD] == CANARY_BITS).all() and (h[GUARD + words:] == CANARY_BITS).all(), "%s: bytes beside %s were written" % (what, name)


def test_carved_buffers_no_sync_no_allocation():
    """gd_bc_update_dim at 128 with everything it writes carved from canary-filled buffers: nothing beside them is written,
    and a full batch writes the rows' scratch, the gradient, its partials and the optimiser's state whole.  Then B = 1."""
    c = WGR.case("wide_chunks", "seeded")
    M = len(c["obs"])
    obs, expert, pm, rm = _inputs(c)
    bc = _trainer(c, batch_size=M, chunk_rows=2, partials=3)
    G, T = bc.G, len(bc._names)
    written, scratch = Carver(), Carver()

    def swap(name, field, struct, carver=written, dtype=torch.float32):
        old = getattr(bc, name)
        new = carver.carve(name, tuple(old.shape), dtype)
        if carver is written:
            new.copy_(old)
        setattr(bc, name, new)
        setattr(struct, field, new.data_ptr())
        return new

    o, g = bc._o, bc._g
    for name, field in (("flat", "params"), ("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"), ("grad", "grad"),
                        ("_actions", "actions"), ("_nll", "nll"), ("_grad_nll", "grad_nll"), ("tensor_norms", "tensor_norms"),
                        ("stats", "stats"), ("_scal", "scal")):
        swap(name, field, o)
    read = swap("_read", "stats_sum", o, dtype=torch.int32)
    bc.stats_sum, bc.max_grad_tensor = read[:6].view(torch.float32), read[6:]
    o.max_grad_tensor = bc.max_grad_tensor.data_ptr()
    swap("_partials", "partials", g)
    swap("_grad_scratch", "scratch", g, carver=scratch)
    blob = written.carve("blob", tuple(bc.policy.blob.shape))
    blob.copy_(bc.policy.blob)
    bc.policy.blob = blob
    o.blob = bc._pd.base.blob = blob.data_ptr()
    for name in ("_nll", "_grad_nll", "grad", "_partials", "tensor_norms"):   # what a full batch must write whole
        getattr(bc, name).view(torch.int32).fill_(CANARY_BITS)
    bc._actions.view(torch.int32).fill_(CANARY_BITS)
    bc._scal.view(torch.int32).fill_(CANARY_BITS)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    _no_sync(lambda: bc.update(obs, expert, pm, rm))
    assert torch.cuda.memory_allocated() == before, "the update allocated"
    torch.cuda.synchronize()
    written.assert_guards("gd_bc_update_dim B = %d" % M)
    _guards(scratch, "gd_bc_update_dim B = %d" % M)
    assert int(bc._step.item()) == 1 and np.isfinite(bc.flat.cpu().numpy()).all()
    _assert_blob_follows(bc, "carved")
    assert bc._scal.numel() == 4 + 2 * T and bc.flat.numel() == G + 1
    # one row, and the full batch again, on the same objects
    one = [t[:1].contiguous() for t in (obs, expert, pm, rm)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    _no_sync(lambda: bc.update(*one))
    _no_sync(lambda: bc.update(obs, expert, pm, rm))
    assert torch.cuda.memory_allocated() == before, "the update allocated"
    torch.cuda.synchronize()
    _guards(written, "B = 1")
    _guards(scratch, "B = 1")
    assert int(bc._step.item()) == 3 and np.isfinite(bc.flat.cpu().numpy()).all()
    _assert_blob_follows(bc, "after B = 1")
    more = [torch.cat([t, t[:1]]) for t in (obs, expert, pm, rm)]
    with pytest.raises(ValueError, match="batch_size"):
        bc.update(*more)
    assert int(bc._step.item()) == 3


# ---- the loop and the optimiser state

def _tiny_dataset(A=64, samples=7):
    """tests/test_gpu_bc_update.py's recipe: two recorded rows of which `samples` (row, time) pairs are alive."""
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
    the second epoch.  wide_min's model (R = 1, 64 agent slots)."""
    c = WGR.case("wide_min")
    steps = 5
    ds = _tiny_dataset(c["A"])
    a, b = (_trainer(c, batch_size=3, **SMALL) for _ in range(2))
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
    reads = a.host_reads
    out = a.losses()
    assert a.host_reads == reads + 1 and out["max_grad_name"] in a._names
    for k, v in zip(_capi.BC_STATS, sums):
        assert out[k] == v / steps and np.isfinite(out[k]), k
    assert out["grad_norm"] > 0 and 0 < out["max_grad_norm"] <= min(out["grad_norm"], 20.0) * (1 + 1e-6)


def _torch_step(tbp, opt, obs, expert, pm, rm):
    opt.zero_grad()
    tbp(obs, pm, rm, expert).mean().backward()
    torch.nn.utils.clip_grad_norm_(tbp.parameters(), 20)
    opt.step()


def _assert_one_step_apart(bc, tbp, what):
    """tests/test_gpu_bc_update.py's bound for one optimiser step on the SAME gradient bits by both sides: the rounding term of
    the one-step bound, 8 * 2^-24 (|p| + lr)."""
    mine = bc.state_dict()
    for k, p in tbp.named_parameters():
        a, b = mine[k].cpu().numpy().astype(np.float64), p.detach().cpu().numpy().astype(np.float64)
        bound = 8 * 2.0 ** -24 * (np.abs(b) + bc.learning_rate)
        assert (np.abs(a - b) <= bound).all(), (what, k, float((np.abs(a - b) / bound).max()))


def test_the_optimiser_state_round_trips_with_torch_adamw():
    c = WGR.case("wide_min")
    obs, expert, pm, rm = _inputs(c)
    bc = _trainer(c, batch_size=3, **SMALL)
    bc.update(obs, expert, pm, rm)
    # DeviceBCDim -> torch
    tbp = _train(c, sd=bc.state_dict(), **SMALL)
    opt = torch.optim.AdamW(tbp.parameters(), lr=1e-3, eps=1e-4, weight_decay=0.5)
    opt.load_state_dict(bc.optimizer_state_dict())
    group = opt.param_groups[0]
    assert group["lr"] == 5e-4 and group["weight_decay"] == 0.01 and group["eps"] == 1e-4 and group["betas"] == (0.9, 0.999)
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
    _assert_one_step_apart(bc, tbp, "DeviceBCDim -> torch")
    # torch -> DeviceBCDim: another learning rate and weight decay travel with the state
    for g in opt.param_groups:
        g["lr"], g["weight_decay"] = 2e-4, 0.02
    other = _trainer(dict(c, sd=tbp.state_dict()), batch_size=3, **SMALL)
    other.load_optimizer_state_dict(opt.state_dict())
    assert int(other._step.item()) == 2 and other.learning_rate == 2e-4 and other.weight_decay == 0.02
    assert np.array_equal(other._beta_pow.cpu().numpy(), np.array([0.9 * 0.9, 0.999 * 0.999]))
    back = other.optimizer_state_dict()
    for i, p in enumerate(tbp.parameters()):
        for name in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(_bits(back["state"][i][name]), _bits(opt.state[p][name])), (i, name)
        assert float(back["state"][i]["step"]) == 2
    _torch_step(tbp, opt, obs, expert, pm, rm)
    other.update(obs, expert, pm, rm)
    _assert_one_step_apart(other, tbp, "torch -> DeviceBCDim")


def test_twenty_updates_lower_the_loss():
    """Twenty updates on wide_min's three rows: `losses()` after the tenth update is the mean loss of the first ten, after the
    twentieth the mean of the last ten.  wide_min has one component and covariances pushed to the clamp, so its loss is large
    and not monotonic; the float64 CPU run of the same twenty steps (tests/bc_wide_update_reference.pipeline, 40 s, run when
    the case was chosen) goes 6.65e8, 3.15e9, 7.74e8, .. 2.57e7 with the two means 5.75e8 and 5.27e7, a factor of ten apart."""
    c = WGR.case("wide_min")
    t = _inputs(c)
    bc = _trainer(c, batch_size=3, **SMALL)
    means, every = [], []
    for i in range(20):
        bc.update(*t)
        every.append(bc.stats[0].clone())
        if i in (9, 19):
            means.append(bc.losses()["loss"])
    every = [float(v) for v in torch.stack(every).cpu()]
    print("BCWIDEUPDATE LOSSES", " ".join("%.4g" % v for v in every))
    assert np.isfinite(every).all() and means[1] < means[0]
    assert means[0] == pytest.approx(np.mean(every[:10]), rel=1e-5) and means[1] == pytest.approx(np.mean(every[10:]), rel=1e-5)
    assert every[0] == pytest.approx(c["nll"].mean(), rel=1e-3) and bc.host_reads == 2
