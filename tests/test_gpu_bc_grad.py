"""GPU suite: the device BC backward (gpudrive_lab_amd.bc_train.TrainableBCPolicy; gd_bc_backward) against float64 autograd of
the differentiable restatement (tests/bc_grad_reference.py, itself pinned to the reference module's backward by
tests/test_bc_grad.py) on the shapes and constructed samples of tests/bc_cases.py and one minimal model.

The yardstick E_p of a case and a parameter tensor is the maximum absolute error of the SAME stand-in under torch's float32
CPU autograd against float64, floored at 2^-23 max |g|; every gradient must be within K E_p.  K and the measured ratios:
DESIGN section 6 (this test prints them per case and tensor with -s).  The worst E_p ratio of each of bc_cases.EDGE_CASES,
measured once on an MI355X: top 2.99 (2.94 with chunk_rows 2 and three partials), sweep 3.22, c9 3.49, c10 4.04,
deep_branch 2.29, deep_fusion 3.89, defaults 2.51; one training step at sweep: 0.10 of its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from tests import bc_cases as BC
from tests import bc_grad_reference as GR
from tests.test_gpu_bc_policy import Carver, _dev, _no_sync

pytestmark = pytest.mark.gpu

K = 32
_REF = {}


def _train(sd, A, R, cfg=BC.CFG, **kw):
    from gpudrive_lab_amd import TrainableBCPolicy
    return TrainableBCPolicy.from_state_dict(sd, max_agents=A, num_stack=R, device="cuda", **cfg, **kw)


def _reference(B, A, R, cfg, kind, rows=None):
    """The case's float64 gradients, their yardstick and inputs, computed once and shared (nobody writes into it)."""
    key = (GR.case_key(B, A, R, cfg), kind, None if rows is None else tuple(rows))
    if key not in _REF:
        sd, obs, pm, rm, expert, kinds = GR.case_inputs(B, A, R, cfg)
        if rows is not None:
            obs, pm, rm, expert, kinds = obs[rows], pm[rows], rm[rows], expert[rows], [kinds[i] for i in rows]
        w = GR.grad_weights(len(obs), kind)
        g64, nll, margins = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg)
        g32, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, dtype=torch.float32)
        assert min(margins.values()) > GR.MARGIN, margins
        _REF[key] = dict(sd=sd, obs=obs, pm=pm, rm=rm, expert=expert, kinds=kinds, w=w, g64=g64, nll=nll, E=GR.yardstick(g32, g64))
    return _REF[key]


def _device(c, A, R, cfg=BC.CFG, obs=None, w=None, pm=None, **kw):
    """One forward and backward on the device: (gradients by name as numpy, nll)."""
    tbp = _train(c["sd"], A, R, cfg, **kw)
    obs_t, pm_t, rm_t, ex_t, w_t = _dev(c["obs"] if obs is None else obs, c["pm"] if pm is None else pm, c["rm"], c["expert"],
                                        c["w"] if w is None else w)
    nll = tbp(obs_t, pm_t, rm_t, ex_t)
    (nll * w_t).sum().backward()
    return {k: p.grad.cpu().numpy().copy() for k, p in tbp.named_parameters()}, nll.detach().cpu().numpy()


def _ratios(what, got, c, want=None):
    want = c["g64"] if want is None else want
    worst, at = 0.0, None
    for k, g in want.items():
        assert got[k].shape == g.shape and np.isfinite(got[k]).all(), (what, k)
        err = float(np.abs(got[k].astype(np.float64) - g).max())
        ratio = err / c["E"][k] if c["E"][k] > 0 else (0.0 if err == 0 else np.inf)  # (E_p = 0: float32 and float64 give exact zeros)
        print("BCGRAD RATIO %s %s err %.3e E %.3e max|g| %.3e ratio %.2f" % (what, k, err, c["E"][k], np.abs(g).max(), ratio))
        if ratio > worst:
            worst, at = ratio, k
    print("BCGRAD WORST %s %.2f at %s" % (what, worst, at))
    return worst, at


# bc_cases.EDGE_CASES alternate between the two upstream gradients; `defaults` (130 rows, the default chunk_rows and partials
# of 128: a second chunk behind a full one) takes the mean
EDGE_KINDS = dict(top="seeded", sweep="mean", c9="seeded", c10="mean", deep_branch="seeded", deep_fusion="mean", defaults="mean")
CASES = [(1, 64, 5, BC.CFG, "mean"), (3, 64, 1, BC.CFG, "seeded"), (17, 64, 5, BC.CFG, "mean"), (2, 128, 5, BC.CFG, "seeded"),
         (3, 64, 1, GR.MINIMAL, "mean")] + [(B, A, R, cfg, EDGE_KINDS[name]) for name, B, A, R, cfg in BC.EDGE_CASES]
_CFG_IDS = {id(GR.MINIMAL): "min", id(BC.CFG): "full", **{id(cfg): name for name, _, _, _, cfg in BC.EDGE_CASES}}


@pytest.mark.parametrize("B,A,R,cfg,kind", CASES, ids=lambda v: _CFG_IDS[id(v)] if isinstance(v, dict) else str(v))
def test_every_parameter_gradient_against_float64(B, A, R, cfg, kind):
    c = _reference(B, A, R, cfg, kind)
    got, nll = _device(c, A, R, cfg)
    assert list(got) == list(c["g64"])
    worst, at = _ratios("%s %s" % (GR.case_key(B, A, R, cfg), kind), got, c)
    assert worst <= K, (worst, at)
    assert np.abs(nll - c["nll"]).max() <= 1e-3 * (1 + np.abs(c["nll"]).max())
    if cfg is BC.EDGE["deep_fusion"][3]:
        # a floor above 0: the covariances every row has below it (the pushed one among them) and the one pushed above
        # 3.58352 get exactly zero rows of head.head, as float64 gives them; the others do not
        C_ = cfg["n_components"]
        w64 = c["g64"]["head.head.weight"][3 * C_:6 * C_]
        dead = np.flatnonzero((w64 == 0).all(1))
        assert {1, 5} <= set(dead.tolist()) and 2 < len(dead) < 3 * C_, dead
        for r in dead + 3 * C_:
            assert (got["head.head.weight"][r] == 0.0).all() and got["head.head.bias"][r] == 0.0, r
        live = np.setdiff1d(np.arange(3 * C_), dead) + 3 * C_
        assert (np.abs(got["head.head.weight"][live]).max(1) > 0).all()


def test_the_largest_model_in_three_chunks():
    """`top` (288 tensors, every count at its limit) once more with chunk_rows = 2 and three partials: a short last chunk, a
    partial that takes two chunks' sums; equal bits between two runs, and within K E_p."""
    B, A, R, cfg = BC.EDGE["top"]
    c = _reference(B, A, R, cfg, EDGE_KINDS["top"])
    got, _ = _device(c, A, R, cfg, chunk_rows=2, partials=3)
    worst, at = _ratios("top chunk 2 partials 3", got, c)
    assert worst <= K, (worst, at)
    again, _ = _device(c, A, R, cfg, chunk_rows=2, partials=3)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k


@pytest.mark.parametrize("partials", [1, 3, None])
def test_three_chunks_with_a_short_last_one(partials):
    c = _reference(5, 64, 5, BC.CFG, "seeded")
    got, _ = _device(c, 64, 5, chunk_rows=2, partials=partials)
    worst, at = _ratios("chunk 2 partials %s" % partials, got, c)
    assert worst <= K, (worst, at)
    again, _ = _device(c, 64, 5, chunk_rows=2, partials=partials)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k


def test_exact_zeros_outside_the_clamp():
    """bc_cases.state_dict pushes raw covariances 1 and 5 outside the clamp through the bias: their rows get exactly 0."""
    c = _reference(3, 64, 1, BC.CFG, "seeded")
    got, _ = _device(c, 64, 1)
    C_ = BC.CFG["n_components"]
    for r in (3 * C_ + 1, 3 * C_ + 5):
        assert (got["head.head.weight"][r] == 0.0).all() and got["head.head.bias"][r] == 0.0
    assert np.abs(got["head.head.weight"][3 * C_:6 * C_]).max() > 0


def test_exact_zeros_with_every_partner_masked():
    c = _reference(3, 64, 1, BC.CFG, "seeded")
    got, _ = _device(c, 64, 1, pm=np.ones_like(c["pm"]))
    p = "ego_ro_attn.0.module."
    for name in (p + "attention.q_proj", p + "attention.k_proj", p + "q_norm"):
        assert (got[name + ".weight"] == 0.0).all() and (got[name + ".bias"] == 0.0).all(), name
    for name in (p + "attention.v_proj", p + "attention.o_proj", p + "kv_norm"):
        assert np.abs(got[name + ".weight"]).max() > 0 and np.abs(got[name + ".bias"]).max() > 0, name


def test_zero_upstream_gradient_gives_exact_zeros():
    c = _reference(3, 64, 1, BC.CFG, "seeded")
    got, _ = _device(c, 64, 1, w=np.zeros(3, np.float32))
    for k, g in got.items():
        assert (g == 0.0).all(), k


def test_masked_entities_features_do_not_matter():
    """Rows with at least one unmasked key in every segment (kinds c, d, r): other features for the masked entities change
    the tokens' embeddings but no gradient beyond K E_p -- a masked key has p = 0 exactly and receives nothing."""
    B, A, R = 17, 64, 5
    kinds = BC.sample_kinds(B)
    rows = [i for i, k in enumerate(kinds) if k in ("c", "d", "r")]
    c = _reference(B, A, R, BC.CFG, "mean", rows=rows)
    got, _ = _device(c, A, R, obs=BC.overwrite_masked(c["obs"], c["pm"], c["rm"], A))
    worst, at = _ratios("overwrite_masked", got, c)
    assert worst <= K, (worst, at)


def test_forward_is_the_device_policys_nll_bit_for_bit():
    c = _reference(17, 64, 5, BC.CFG, "mean")
    tbp = _train(c["sd"], 64, 5, chunk_rows=8)
    bc = BP.DeviceBCPolicy.from_state_dict(tbp.state_dict(), max_agents=64, num_stack=5, chunk_rows=8, **BC.CFG)
    obs, pm, rm, ex = _dev(c["obs"], c["pm"], c["rm"], c["expert"])
    a, b = tbp(obs, pm, rm, ex), bc.nll(obs, pm, rm, ex)
    assert a.requires_grad and np.array_equal(a.detach().cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    bc.load_state_dict(tbp.state_dict())
    first = tbp(obs, pm, rm, ex[:, None, :].contiguous())  # two forwards before one backward
    (a.mean() + first.mean()).backward()
    g = {k: p.grad.cpu().numpy().astype(np.float64) / 2 for k, p in tbp.named_parameters()}
    worst, at = _ratios("two forwards", g, c)
    assert worst <= K, (worst, at)
    with pytest.raises(ValueError, match="require grad"):
        tbp(obs.clone().requires_grad_(True), pm, rm, ex)


def test_guards_and_no_sync():
    """gd_bc_backward on carved buffers: nothing beside them is written, partials, grad and nll are written whole; and a whole
    step through the module under torch's sync debug mode."""
    B, A, R = 5, 64, 5
    c = _reference(B, A, R, BC.CFG, "seeded")
    bc = BP.DeviceBCPolicy.from_state_dict(c["sd"], max_agents=A, num_stack=R, chunk_rows=2, **BC.CFG)
    from gpudrive_lab_amd import bc_train as BT
    G, P = BT.grad_floats(R, BC.CFG["num_layer"], BC.CFG["head_num_layers"], BC.CFG["n_components"]), 3
    carver = Carver()
    scratch = carver.carve("scratch", (BT.grad_scratch_floats(A, 2, BC.CFG["num_layer"], bc.blob.numel()),))
    carver.assert_guards("before", written=False)
    written = Carver()
    partials, grad, nll = written.carve("partials", (P * G,)), written.carve("grad", (G,)), written.carve("nll", (B,))
    obs, pm, rm, ex, w = _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["w"])
    p, g = _capi.GdBCPolicy(), _capi.GdBCGrad()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers = A, R, *BC.CFG["num_layer"]
    p.head_layers, p.n_components, p.clip_value, p.chunk_rows = BC.CFG["head_num_layers"], BC.CFG["n_components"], -20.0, 2
    p.blob, p.blob_floats, p.scratch, p.scratch_floats = bc.blob.data_ptr(), bc.blob.numel(), bc._scratch.data_ptr(), bc._scratch.numel()
    g.scratch, g.scratch_floats, g.partials, g.grad_floats, g.num_partials = scratch.data_ptr(), scratch.numel(), partials.data_ptr(), G, P
    L = _capi.lib()
    args = (obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), B, ex.data_ptr(), w.data_ptr(), nll.data_ptr(), grad.data_ptr(), None)
    _capi.check(L.gd_bc_backward(C.byref(p), C.byref(g), *args))
    torch.cuda.synchronize()
    written.assert_guards("gd_bc_backward")
    h = carver.whole["scratch"][0].cpu().numpy()
    assert (h[:64] == 0x7FC0DEAD).all() and (h[-64:] == 0x7FC0DEAD).all()
    worst, at = _ratios("C call", dict(zip(c["g64"], np.split(grad.cpu().numpy(), np.cumsum([v.size for v in c["g64"].values()])[:-1]))),
                        {**c, "g64": {k: v.reshape(-1) for k, v in c["g64"].items()}})
    assert worst <= K, (worst, at)
    assert np.array_equal(nll.cpu().numpy().view(np.int32), bc.nll(obs, pm, rm, ex).cpu().numpy().view(np.int32))
    for field, bad, word in (("num_partials", 0, "num_partials"), ("grad_floats", G - 1, "grad_floats"), ("scratch_floats", 64, "scratch_floats")):
        keep = getattr(g, field)
        setattr(g, field, bad)
        assert L.gd_bc_backward(C.byref(p), C.byref(g), *args) == _capi.GD_ERR_INVALID and word in L.gd_last_error().decode()
        setattr(g, field, keep)
    tbp = _train(c["sd"], A, R, chunk_rows=2, partials=3)
    tbp(obs, pm, rm, ex).mean().backward()  # (the workspace and the .grad tensors exist now)

    def step():
        tbp(obs, pm, rm, ex).mean().backward()
    _no_sync(step)


def test_memory_does_not_depend_on_the_batch():
    A, R, rises = 64, 5, {}
    sd = BC.state_dict(R)
    for B in (3, 17):
        obs, pm, rm, expert, _, _, _ = BC.inputs(B, A, R)
        tbp = _train(sd, A, R, chunk_rows=2, partials=3)
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


def _cpu_step(c, A, cfg, steps):
    """The reference's training step in float64 on the CPU: module surface, clip_grad_norm_(20), AdamW(lr=5e-4, eps=1e-4)."""
    net = GR.Net(c["sd"], A, cfg)
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


def _gpu_steps(c, A, R, steps, cfg=BC.CFG):
    tbp = _train(c["sd"], A, R, cfg)
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


def test_one_training_step_against_float64():
    """After one step p' = p (1 - lr wd) - lr gc / (|gc| + eps), gc = s g the clipped gradient, s = min(1, 20 / (|g|_2 + 1e-6))
    (AdamW's first step: m / (1 - b1) = gc, sqrt(v / (1 - b2)) = |gc|).  A gradient within d = K E_p of float64 moves
      s by at most s |dg|_2 / |g|_2 with |dg|_2 <= sqrt(sum_p n_p d_p^2)     (the norm is 1-Lipschitz),
      gc by at most dgc = s d + |g| s |dg|_2 / |g|_2,
      gc / (|gc| + eps) by at most dgc / eps                                 (its derivative is eps / (|gc| + eps)^2 <= 1 / eps),
    so |p' - p'_64| <= lr dgc / eps + 8 * 2^-24 (|p| + lr): the second term is float32's rounding of the update itself."""
    _one_step_within_the_bound(3, 64, 1, BC.CFG)


def test_one_training_step_at_the_sweeps_model():
    """The same bound at bc_cases' `sweep`: num_layer (4, 3), 252 tensors, the clip10 clamp."""
    _one_step_within_the_bound(*BC.EDGE["sweep"])


def _one_step_within_the_bound(B, A, R, cfg):
    c = _reference(B, A, R, cfg, "mean")
    want, _ = _cpu_step(c, A, cfg, 1)
    tbp, _ = _gpu_steps(c, A, R, 1, cfg)
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
    print("BCGRAD STEP %s worst err/bound %.3f" % (GR.case_key(B, A, R, cfg), worst))


def test_twenty_steps_lower_the_loss():
    """One fixed batch of 8 rows; the seed is one with which the float64 CPU run of the same twenty steps also ends lower
    (45.61 -> 1.35 there, not monotonically)."""
    c = _reference(8, 64, 5, BC.CFG, "mean")
    _, losses = _gpu_steps(c, 64, 5, 20)
    print("BCGRAD LOSSES", " ".join("%.4f" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
