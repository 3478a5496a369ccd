"""GPU suite: the device BC backward at network_dim 128 (gpudrive_lab_amd.bc_train.TrainableBCPolicyDim; gd_bc_backward_dim)
against float64 autograd of the differentiable restatement at that width (tests/bc_wide_grad_reference.py, itself pinned to
the reference module's backward by tests/test_bc_wide_grad.py) on the cases of tests/bc_wide_cases.py.

The yardstick is tests/test_gpu_bc_grad.py's: E_p of a case and a parameter tensor is the maximum absolute error of the SAME
restatement under torch's float32 CPU autograd against float64, floored at 2^-23 max |g|; every gradient must be within
K = 32 E_p (this test prints the ratios per case and tensor with -s).  The worst E_p ratio of each case, measured once on an
MI355X: wide_min 2.76 (mean) and 2.92 (seeded), wide_a128 5.11, wide_sweep 2.77; wide_chunks with chunk_rows 2 and partials
1 / 3 / 128: 11.33 / 4.22 / 2.84 (the 11.33 is ego_rg_attn's v_proj bias, 1,000 keys summed in one chain); wide_sweep's row c
with the masked entities' features overwritten 4.55; the C call on carved buffers 4.22; one training step at wide_sweep 0.089
of its bound.  DESIGN section 6 has the table.  The edge configurations of bc_wide_cases.EDGE_CASES (tests/test_gpu_bc_wide_edges.py):
wide_top 3.08, wide_clip10 2.85, wide_c9 5.66, wide_c10 6.07, wide_deep_branch 5.75, wide_deep_fusion 2.68, wide_defaults 2.30."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from gpudrive_lab_amd import bc_train as BT
from tests import bc_cases as BC
from tests import bc_grad_reference as GR
from tests import bc_wide_cases as WC
from tests import bc_wide_grad_reference as WGR
from tests.test_gpu_bc_grad import K, _ratios
from tests.test_gpu_bc_policy import Carver, _dev, _no_sync

pytestmark = pytest.mark.gpu


def _train(c, **kw):
    from gpudrive_lab_amd import TrainableBCPolicyDim
    return TrainableBCPolicyDim.from_state_dict(c["sd"], max_agents=c["A"], num_stack=c["R"], device="cuda", network_dim=WC.DIM,
                                                **c["cfg"], **kw)


def _device(c, obs=None, w=None, pm=None, **kw):
    """One forward and backward on the device: (gradients by name as numpy, nll)."""
    tbp = _train(c, **kw)
    obs_t, pm_t, rm_t, ex_t, w_t = _dev(c["obs"] if obs is None else obs, c["pm"] if pm is None else pm, c["rm"], c["expert"],
                                        c["w"] if w is None else w)
    nll = tbp(obs_t, pm_t, rm_t, ex_t)
    (nll * w_t).sum().backward()
    return {k: p.grad.cpu().numpy().copy() for k, p in tbp.named_parameters()}, nll.detach().cpu().numpy()


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


# wide_min: 63 and 200 keys, odd first-layer widths, no residual block, C = 1; wide_a128: 127 keys, branch > fusion;
# wide_sweep: the sweep's model.  The upstream gradients alternate
CASES = [("wide_min", "mean"), ("wide_a128", "seeded"), ("wide_sweep", "mean"), ("wide_min", "seeded")]


@pytest.mark.parametrize("name,kind", CASES)
def test_every_parameter_gradient_against_float64(name, kind):
    c = WGR.case(name, kind)
    assert min(c["margins"].values()) > GR.MARGIN, c["margins"]
    got, nll = _device(c)
    assert list(got) == list(c["g64"])
    worst, at = _ratios("%s %s" % (name, kind), got, c)
    assert worst <= K, (worst, at)
    assert np.abs(nll - c["nll"]).max() <= 1e-3 * (1 + np.abs(c["nll"]).max())
    if name == "wide_sweep":
        # the raw covariances bc_cases.state_dict pushes outside the clamp get exactly zero rows of head.head
        C_ = c["cfg"]["n_components"]
        for r in (3 * C_ + 1, 3 * C_ + 5):
            assert (c["g64"]["head.head.weight"][r] == 0).all()
            assert (got["head.head.weight"][r] == 0.0).all() and got["head.head.bias"][r] == 0.0, r
        assert np.abs(got["head.head.weight"][3 * C_:6 * C_]).max() > 0


def test_forward_is_the_device_policys_nll_bit_for_bit():
    c = WGR.case("wide_sweep", "mean")
    tbp = _train(c, chunk_rows=2, partials=3)
    bc = BP.DeviceBCPolicy.from_state_dict(tbp.state_dict(), max_agents=c["A"], num_stack=c["R"], chunk_rows=2, network_dim=WC.DIM,
                                           **c["cfg"])
    obs, pm, rm, ex = _dev(c["obs"], c["pm"], c["rm"], c["expert"])
    a, b = tbp(obs, pm, rm, ex), bc.nll(obs, pm, rm, ex)
    assert a.requires_grad and np.array_equal(a.detach().cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    bc.load_state_dict(tbp.state_dict())  # a DeviceBCPolicy of the same width follows training


@pytest.mark.parametrize("partials", [1, 3, None])
def test_three_chunks_with_a_short_last_one(partials):
    c = WGR.case("wide_chunks", "seeded")
    got, _ = _device(c, chunk_rows=2, partials=partials)
    worst, at = _ratios("wide_chunks chunk 2 partials %s" % partials, got, c)
    assert worst <= K, (worst, at)
    again, _ = _device(c, chunk_rows=2, partials=partials)
    _same_bits(got, again)


def test_zero_upstream_gradient_gives_exact_zeros():
    c = WGR.case("wide_min", "seeded")
    got, _ = _device(c, w=np.zeros(len(c["obs"]), np.float32))
    for k, g in got.items():
        assert (g == 0.0).all(), k


def test_exact_zeros_with_every_partner_masked():
    c = WGR.case("wide_min", "seeded")
    pm = np.ones_like(c["pm"])
    g64, _, _ = WGR.gradients(c["sd"], c["obs"], pm, c["rm"], c["expert"], c["w"], c["A"], c["cfg"])
    got, _ = _device(c, pm=pm)
    p = "ego_ro_attn.0.module."
    for name in (p + "attention.q_proj", p + "attention.k_proj", p + "q_norm"):
        assert (g64[name + ".weight"] == 0).all() and (g64[name + ".bias"] == 0).all(), name
        assert (got[name + ".weight"] == 0.0).all() and (got[name + ".bias"] == 0.0).all(), name
    for name in (p + "attention.v_proj", p + "attention.o_proj", p + "kv_norm"):
        assert np.abs(got[name + ".weight"]).max() > 0 and np.abs(got[name + ".bias"]).max() > 0, name


def test_masked_entities_features_do_not_matter():
    """wide_sweep's row c (one unmasked key in every segment; rows a and b have a segment with none): other features for the
    masked entities change their tokens but no gradient beyond K E_p -- a masked key has p = 0 exactly and receives nothing.
    (Five rows of the sweep's model would carry kinds d and r too; at three rows the case has kind c alone.)"""
    name = "wide_sweep"
    kinds = WGR.case(name, "mean")["kinds"]
    rows = [i for i, k in enumerate(kinds) if k in ("c", "d", "r")]
    assert rows
    c = WGR.case(name, "mean", rows=rows)
    got, _ = _device(c, obs=BC.overwrite_masked(c["obs"], c["pm"], c["rm"], c["A"]))
    worst, at = _ratios("wide overwrite_masked", got, c)
    assert worst <= K, (worst, at)


def test_backward_dim_at_64_is_gd_bc_backward_bit_for_bit():
    from gpudrive_lab_amd import TrainableBCPolicy, TrainableBCPolicyDim
    B, A, R = 3, 64, 1
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R)
    t = _dev(obs, pm, rm, expert)
    w = _dev(GR.grad_weights(B, "seeded"))[0]
    bc = BP.DeviceBCPolicy.from_state_dict(sd, max_agents=A, num_stack=R, chunk_rows=2, **BC.CFG)
    G, P = BT.grad_floats(R, BC.CFG["num_layer"], BC.CFG["head_num_layers"], BC.CFG["n_components"]), 3
    scratch = torch.empty(BT.grad_scratch_floats(A, 2, BC.CFG["num_layer"], bc.blob.numel()), device="cuda")
    partials = torch.empty(P * G, device="cuda")
    pd, g = _capi.GdBCPolicyDim(), _capi.GdBCGrad()
    pd.base, pd.network_dim, pd.reserved = bc.c_struct(), 64, 0
    g.scratch, g.scratch_floats, g.partials, g.grad_floats, g.num_partials = scratch.data_ptr(), scratch.numel(), partials.data_ptr(), G, P
    out = {}
    L = _capi.lib()
    for who, fn, p in (("dim", L.gd_bc_backward_dim, pd), ("plain", L.gd_bc_backward, pd.base)):
        grad, nll = torch.full((G,), np.nan, device="cuda"), torch.full((B,), np.nan, device="cuda")
        _capi.check(fn(C.byref(p), C.byref(g), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), B, t[3].data_ptr(), w.data_ptr(),
                       nll.data_ptr(), grad.data_ptr(), None))
        torch.cuda.synchronize()
        out[who] = (grad.cpu().numpy(), nll.cpu().numpy())
    assert np.isfinite(out["plain"][0]).all() and np.abs(out["plain"][0]).max() > 0
    assert np.array_equal(out["dim"][0].view(np.int32), out["plain"][0].view(np.int32))
    assert np.array_equal(out["dim"][1].view(np.int32), out["plain"][1].view(np.int32))
    # ... and a 64-wide instance of either class gives the same bits
    got = []
    for cls in (TrainableBCPolicy, TrainableBCPolicyDim):
        tbp = cls.from_state_dict(sd, max_agents=A, num_stack=R, device="cuda", chunk_rows=2, partials=3, **BC.CFG)
        (tbp(*t) * w).sum().backward()
        got.append({k: p.grad.cpu().numpy() for k, p in tbp.named_parameters()})
    _same_bits(got[0], got[1])


def test_guards_and_no_sync():
    """gd_bc_backward_dim at 128 on carved buffers: nothing beside them is written, partials, grad and nll are written whole;
    and a whole step through the module under torch's sync debug mode."""
    c = WGR.case("wide_chunks", "seeded")
    A, R, cfg, B = c["A"], c["R"], c["cfg"], len(c["obs"])
    bc = BP.DeviceBCPolicy.from_state_dict(c["sd"], max_agents=A, num_stack=R, chunk_rows=2, network_dim=WC.DIM, **cfg)
    G, P = BT.grad_floats(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], network_dim=WC.DIM), 3
    carver = Carver()
    scratch = carver.carve("scratch", (BT.grad_scratch_floats(A, 2, cfg["num_layer"], bc.blob.numel(), network_dim=WC.DIM),))
    carver.assert_guards("before", written=False)
    written = Carver()
    partials, grad, nll = written.carve("partials", (P * G,)), written.carve("grad", (G,)), written.carve("nll", (B,))
    obs, pm, rm, ex, w = _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["w"])
    g = _capi.GdBCGrad()
    pd = bc.c_struct_dim()
    g.scratch, g.scratch_floats, g.partials, g.grad_floats, g.num_partials = scratch.data_ptr(), scratch.numel(), partials.data_ptr(), G, P
    L = _capi.lib()
    args = (obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), B, ex.data_ptr(), w.data_ptr(), nll.data_ptr(), grad.data_ptr(), None)
    _capi.check(L.gd_bc_backward_dim(C.byref(pd), C.byref(g), *args))
    torch.cuda.synchronize()
    written.assert_guards("gd_bc_backward_dim")
    h = carver.whole["scratch"][0].cpu().numpy()
    assert (h[:64] == 0x7FC0DEAD).all() and (h[-64:] == 0x7FC0DEAD).all()
    worst, at = _ratios("C call", dict(zip(c["g64"], np.split(grad.cpu().numpy(), np.cumsum([v.size for v in c["g64"].values()])[:-1]))),
                        {**c, "g64": {k: v.reshape(-1) for k, v in c["g64"].items()}})
    assert worst <= K, (worst, at)
    assert np.array_equal(nll.cpu().numpy().view(np.int32), bc.nll(obs, pm, rm, ex).cpu().numpy().view(np.int32))
    for field, bad, word in (("num_partials", 0, "num_partials"), ("grad_floats", G - 1, "grad_floats"), ("scratch_floats", 64, "scratch_floats")):
        keep = getattr(g, field)
        setattr(g, field, bad)
        assert L.gd_bc_backward_dim(C.byref(pd), C.byref(g), *args) == _capi.GD_ERR_INVALID and word in L.gd_last_error().decode()
        setattr(g, field, keep)
    tbp = _train(c, chunk_rows=2, partials=3)
    tbp(obs, pm, rm, ex).mean().backward()  # (the workspace and the .grad tensors exist now)

    def step():
        tbp(obs, pm, rm, ex).mean().backward()
    _no_sync(step)


def test_memory_does_not_depend_on_the_batch():
    B0, A, R, cfg = WC.CASES["wide_chunks"]
    sd, rises = BC.state_dict(R, cfg, network_dim=WC.DIM), {}
    for B in (3, 17):
        obs, pm, rm, expert, _, _, _ = BC.inputs(B, A, R)
        tbp = _train(dict(sd=sd, A=A, R=R, cfg=cfg), chunk_rows=2, partials=3)
        t = _dev(obs, pm, rm, expert[:, 0])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        tbp(*t).mean().backward()
        torch.cuda.synchronize()
        rises[B] = torch.cuda.max_memory_allocated() - before
        assert 0 < rises[B] <= tbp.nbytes(B), (B, rises[B], tbp.nbytes(B))
        del tbp, t
    assert abs(rises[17] - rises[3]) <= 14 * 12 + 4 * 512, rises  # the per-row outputs and the allocator's rounding of them


def _cpu_steps(c, steps):
    """The reference's training step in float64 on the CPU: clip_grad_norm_(20), AdamW(lr=5e-4, eps=1e-4)."""
    net = WGR.Net(c["sd"], c["A"], c["cfg"])
    params = list(net.params.values())
    opt = torch.optim.AdamW(params, lr=5e-4, eps=1e-4)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = net.nll(c["obs"], c["pm"], c["rm"], c["expert"]).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 20)
        opt.step()
        losses.append(float(loss.detach()))
    return {k: v.detach().numpy() for k, v in net.params.items()}, losses


def _gpu_steps(c, steps, **kw):
    tbp = _train(c, **kw)
    opt = torch.optim.AdamW(tbp.parameters(), lr=5e-4, eps=1e-4)
    t = _dev(c["obs"], c["pm"], c["rm"], c["expert"])
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = tbp(*t).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(tbp.parameters(), 20)
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        losses.append(tbp(*t).mean())
    return tbp, [float(v) for v in torch.stack(losses).cpu()]


def test_one_training_step_at_the_sweeps_model():
    """tests/test_gpu_bc_grad.py's bound (`test_one_training_step_against_float64` derives it) with the wide reference: after one
    AdamW step |p' - p'_64| <= lr dgc / eps + 8 * 2^-24 (|p| + lr), dgc = s d + |g| s |dg|_2 / |g|_2, d = K E_p."""
    c = WGR.case("wide_sweep", "mean")
    want, _ = _cpu_steps(c, 1)
    tbp, _ = _gpu_steps(c, 1)
    lr, eps = 5e-4, 1e-4
    d = {k: K * c["E"][k] for k in c["g64"]}
    norm = np.sqrt(sum(float((g * g).sum()) for g in c["g64"].values()))
    s = min(1.0, 20.0 / (norm + 1e-6))
    dnorm = np.sqrt(sum(g.size * d[k] ** 2 for k, g in c["g64"].items()))
    worst = 0.0
    for k, p in tbp.named_parameters():
        p0 = c["sd"][k].double().numpy()
        bound = lr * (s * d[k] + np.abs(c["g64"][k]) * s * dnorm / norm) / eps + 8 * 2.0 ** -24 * (np.abs(p0) + lr)
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want[k])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        assert np.abs(want[k] - p0).max() > 0
    print("BCWIDE STEP wide_sweep worst err/bound %.3f" % worst)


TWENTY = dict(B=8, A=64, R=1, cfg=BC._cfg((1, 1), 1, 2, -20.0), seed=1)


def _twenty_case():
    """One fixed batch of 8 rows on a small 128-wide model; the seed is one with which the float64 CPU run of the same twenty
    steps also ends lower (the docstring of the test has its figures)."""
    t = TWENTY
    obs, pm, rm, expert, _, _, _ = BC.inputs(t["B"], t["A"], t["R"], seed=t["seed"])
    return dict(sd=BC.state_dict(t["R"], t["cfg"], network_dim=WC.DIM), obs=obs, pm=pm, rm=rm, expert=expert[:, 0], A=t["A"], R=t["R"],
                cfg=t["cfg"])


def test_twenty_steps_lower_the_loss():
    """Twenty AdamW steps on 8 rows end lower than they began; the float64 CPU run of the same steps does too (checked
    when the seed was chosen, and again here: it costs a second).  Mean NLL 186.38 -> 3.13 on the device, 186.38 -> 3.55 after
    the twentieth step's forward in float64 on the CPU (neither monotonic; the two agree to four digits through step 12)."""
    c = _twenty_case()
    _, cpu = _cpu_steps(c, 20)
    assert cpu[-1] < cpu[0], cpu
    _, losses = _gpu_steps(c, 20, chunk_rows=4, partials=8)
    print("BCWIDE LOSSES gpu", " ".join("%.4f" % v for v in losses))
    print("BCWIDE LOSSES cpu", " ".join("%.4f" % v for v in cpu))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
