"""GPU suite: the device linear probe (gpudrive_lab_amd.lp_probe.DeviceLinearProbe and DeviceBCPolicy.hidden; gd_bc_hidden,
gd_lp_forward, gd_lp_update, gd_lp_eval_accumulate) against the float64 restatement (tests/probe_reference.py, itself pinned
to the reference's modules by tests/test_lp_probe.py) on the shapes of tests/bc_cases.py and the constructed batches of
tests/probe_cases.py.

Hidden states, logits and the gradient: the yardstick E of a case and an output is the maximum absolute error of torch's
float32 CPU run of bc_cases.StandIn's own layers (then F.linear and F.cross_entropy's autograd) against float64 on that case;
the kernel's error must be <= K E.  K was set from ratios measured ONCE on an MI355X (printed per case by these tests with -s):
    (B, A, R)    hidden fusion / ro   logits early other / ego, late other / ego   baseline other / ego   grad
    (1, 64, 5)   0.81  1.05           0.79  1.19  1.23  1.00                                              1.64 (early, other)
    (3, 64, 1)   1.17  1.15           1.04  1.27  1.10  1.19                       0.84  0.93             0.53 (early, ego), 0.32 (baseline, ego)
    (17, 64, 5)  0.94  1.07           0.92  1.16  0.89  1.02                       0.99  1.01             1.48 (early, other), 2.54 (late, ego),
                                                                                                          0.52 (baseline, other)
    (2, 128, 5)  1.19  1.27           1.55  0.94  1.21  1.05                                              0.89 (late, other)
The largest, 2.54, is the gradient of the 'ego' probe on 17 samples, of which 8 are selected: both the yardstick (1.1e-6) and the
kernel's error (2.8e-6) are single draws of a few float32 roundings of a mean over 8 rows.  K = 8.
K is the next power of two at or above twice the largest (5.08).  A ratio above 16 would be a bug, not a bound to raise.
The taps of bc_cases.EDGE_CASES at every layer index (test_hidden_at_every_layer_of_the_edge_configurations), fusion layers
then ro layers, the last of each the tap itself:
    top (4, 4)          1.12 1.20 1.11 1.13   1.19 1.16 1.07 0.98
    deep_branch (1, 4)  1.10                  1.17 1.04 1.06 1.14
    deep_fusion (4, 1)  1.24 1.06 0.82 1.02   0.95
pred, loss_row, the counters, the reduction of the partials and AdamW are held to the host program of csrc/lp_rule.hpp on the
kernel's OWN logits, partials and gradient: exactly, except loss_row, where expf and logf stand between (4 float32 ulps of
its terms, as the header states)."""
import numpy as np
import pytest
import torch

from gpudrive_lab_amd import lp_probe as LP
from tests import bc_cases as BC
from tests import probe_cases as PC
from tests import probe_reference as PREF
from tests.conftest import SCENE_4, SCENE_407
from tests.test_bc_policy import case
from tests.test_gpu_bc_policy import EPS, Carver, _dev, _no_sync, _policy

pytestmark = pytest.mark.gpu

K = 8
ULPS = 4
LR, ADAM_EPS = 0.0015, 1e-4
_TAPS = {}


def _chunk(B):
    return 8 if B == 17 else 128  # B = 17 crosses chunks


def _taps(B, A, R):
    """The float64 taps and the float32 stand-in's, computed once per case and shared."""
    key = (B, A, R)
    if key not in _TAPS:
        c = case(B, A, R)
        _TAPS[key] = (PREF.taps(c["sd"], c["obs"], c["pm"], c["rm"], A, BC.CFG["num_layer"]),
                      PC.standin_taps(c["sd"], c["obs"], c["pm"], c["rm"], A))
    return _TAPS[key]


def _rows64_32(B, A, R, model, exp):
    """The probe's input rows in float64 and as the float32 yardstick has them."""
    c = case(B, A, R)
    if model == "baseline":
        x = PREF.baseline_rows(c["obs"], A, exp)
        return x, x  # obs is float32 already: the gather is exact
    t64, t32 = _taps(B, A, R)
    return PREF.rows(t64[PC.TAP_OF[model]], exp), PREF.rows(t32[PC.TAP_OF[model]], exp)


def _probe(B, A, R, model="early_lp", exp="other", hd=None, **kw):
    c = case(B, A, R)
    Kin = LP.in_features(model, exp, R)
    hd = hd if hd is not None else PC.head(Kin)
    if model == "baseline":
        return None, LP.DeviceLinearProbe(None, hd, model=model, exp=exp, lr=LR, eps=ADAM_EPS, max_agents=A, num_stack=R, **kw), hd
    bc = _policy(A, R, c["sd"], chunk_rows=_chunk(B))
    return bc, LP.DeviceLinearProbe(bc, hd, model=model, exp=exp, lr=LR, eps=ADAM_EPS, **kw), hd


def _batch(B, A, R, exp, kind="plain"):
    c = case(B, A, R)
    mask, lab = PC.labels(B, A, exp, kind)
    obs, pm, rm, expert, m, l_ = _dev(c["obs"], c["pm"], c["rm"], c["expert"], mask, lab)
    valid = torch.ones(B, dtype=torch.bool, device="cuda")
    ego_mask = torch.ones((B, R), dtype=torch.bool, device="cuda")
    return (obs, expert, valid, ego_mask, pm, rm, m, l_), mask, lab


def _ratio(what, err, E):
    r = err / E if E > 0 else (0.0 if err == 0 else np.inf)
    print("LP RATIO %s err %.3e E %.3e ratio %.2f" % (what, err, E, r))
    assert r <= K, (what, err, E, r)
    return r


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()


OPTIMISER = ("flat", "packed", "exp_avg", "exp_avg_sq", "_step", "_beta_pow")


def _state_bits(p, keys=OPTIMISER + ("grad", "stats")):
    return {k: _bits(getattr(p, k)) for k in keys}


def _carve_int64(carver, name, shape):
    return carver.carve(name, tuple(shape) + (2,), torch.int32).view(torch.int64).view(tuple(shape))


# ---- 1. the tap

@pytest.mark.parametrize("B,A,R", BC.SHAPES, ids=lambda v: str(v))
def test_hidden_of_both_taps_against_float64(B, A, R):
    c = case(B, A, R)
    t64, t32 = _taps(B, A, R)
    bc = _policy(A, R, c["sd"], chunk_rows=_chunk(B))
    obs, pm, rm = _dev(c["obs"], c["pm"], c["rm"])
    for tap in PC.TAPS:
        what = "hidden %s B=%d A=%d R=%d" % (tap, B, A, R)
        fresh = bc.hidden(obs, pm, rm, tap=tap).cpu().numpy()
        carver = Carver()
        out = carver.carve("hidden", (B, A, 64))
        _no_sync(lambda: bc.hidden(obs, pm, rm, tap=tap, out=out))  # no host synchronisation, no allocation with out=
        carver.assert_guards(what)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.int32), fresh.view(np.int32)), what
        _ratio(what, float(np.abs(got.astype(np.float64) - t64[tap]).max()), float(np.abs(t32[tap] - t64[tap]).max()))
    ctx = bc.context(obs, pm, rm).cpu().numpy()
    assert np.array_equal(got[:, 0].view(np.int32), ctx[:, :64].view(np.int32))  # ro_attn's token 0 IS the context's first third


@pytest.mark.parametrize("name", ["top", "deep_branch", "deep_fusion"])
def test_hidden_at_every_layer_of_the_edge_configurations(name):
    """bc_cases.EDGE_CASES with the maximal and both asymmetric layer counts: `gd_bc_hidden` at both taps and
    `gd_bc_hidden_layer` at every layer index the block has, each against its own float64 tap (a wrong layer offset gives
    another layer's tokens).  The last index is the tap itself, bit for bit."""
    B, A, R, cfg = BC.EDGE[name]
    c = case(B, A, R, cfg)
    t64 = PREF.taps(c["sd"], c["obs"], c["pm"], c["rm"], A, cfg["num_layer"])
    t32 = PC.standin_taps(c["sd"], c["obs"], c["pm"], c["rm"], A, cfg=cfg)
    bc = _policy(A, R, c["sd"], cfg, chunk_rows=2)  # a short last chunk
    obs, pm, rm = _dev(c["obs"], c["pm"], c["rm"])
    for tap, layers in zip(PC.TAPS, cfg["num_layer"]):
        whole = bc.hidden(obs, pm, rm, tap=tap).cpu().numpy()
        _ratio("hidden %s %s" % (tap, name), float(np.abs(whole.astype(np.float64) - t64[tap]).max()), float(np.abs(t32[tap] - t64[tap]).max()))
        for i in range(layers):
            what = "hidden %s layer %d %s" % (tap, i, name)
            carver = Carver()
            out = carver.carve("hidden", (B, A, 64))
            bc.hidden(obs, pm, rm, tap=tap, layer=i, out=out)
            carver.assert_guards(what)
            got = out.cpu().numpy()
            _ratio(what, float(np.abs(got.astype(np.float64) - t64[(tap, i)]).max()), float(np.abs(t32[(tap, i)] - t64[(tap, i)]).max()))
        assert np.array_equal(got.view(np.int32), whole.view(np.int32)), what
        if layers > 1:  # and a neighbouring layer's float64 tokens are far outside the bound: the index selects
            assert np.abs(t64[(tap, layers - 2)] - t64[tap]).max() > 1000 * K * np.abs(t32[tap] - t64[tap]).max()


def test_hidden_rows_above_the_chunk_equal_the_concatenation_of_the_chunks():
    B, A, R = 17, 64, 5
    c = case(B, A, R)
    obs, pm, rm = _dev(c["obs"], c["pm"], c["rm"])
    small, whole = _policy(A, R, c["sd"], chunk_rows=5), _policy(A, R, c["sd"])
    for tap in PC.TAPS:
        got = small.hidden(obs, pm, rm, tap=tap).cpu().numpy()
        parts = [whole.hidden(obs[i:i + 5], pm[i:i + 5], rm[i:i + 5], tap=tap).cpu().numpy() for i in range(0, B, 5)]
        assert np.array_equal(got.view(np.int32), np.concatenate(parts).view(np.int32)), tap
        assert np.array_equal(got.view(np.int32), whole.hidden(obs, pm, rm, tap=tap).cpu().numpy().view(np.int32)), tap


# ---- 2. logits and the row rule

CASES = [(B, A, R, m, e) for (B, A, R) in BC.SHAPES for m, e in (("early_lp", "other"), ("early_lp", "ego"), ("late_lp", "other"), ("late_lp", "ego"))] \
    + [(B, A, R, "baseline", e) for (B, A, R) in PC.BASELINE_SHAPES for e in PC.EXPS]


@pytest.mark.parametrize("B,A,R,model,exp", CASES, ids=lambda v: str(v))
def test_logits_and_the_row_rule(B, A, R, model, exp):
    what = "logits %s %s B=%d A=%d R=%d" % (model, exp, B, A, R)
    bc, probe, hd = _probe(B, A, R, model, exp, partials=7)
    batch, mask, lab = _batch(B, A, R, exp, "bad")
    obs, pm, rm = batch[0], batch[4], batch[5]
    x64, x32 = _rows64_32(B, A, R, model, exp)
    z64 = PREF.logits(x64, hd)
    z32, _ = PC.float32_head(x32.reshape(-1, x32.shape[-1]), hd, mask, lab, exp)
    shape = PC.row_shape(B, A, exp)
    carver = Carver()
    out = carver.carve("logits", shape + (64,))
    fresh = probe.logits(obs, pm, rm).cpu().numpy()
    _no_sync(lambda: probe.logits(obs, pm, rm, out=out))
    carver.assert_guards(what)
    z = out.cpu().numpy()
    assert z.shape == z64.shape and np.array_equal(z.view(np.int32), fresh.view(np.int32))
    _ratio(what, float(np.abs(z.astype(np.float64) - z64).max()), float(np.abs(z32.reshape(z64.shape) - z64).max()))
    # the rule on the kernel's own logits: pred exactly, loss_row within the header's ulps, the counters exactly
    host = PC.host_rows(z, lab, mask, exp)
    pred = probe.predict(obs, pm, rm).cpu().numpy()
    assert pred.dtype == np.int64 and np.array_equal(pred.reshape(-1), host["pred"])
    c2 = Carver()
    rows = dict(logits=c2.carve("logits", shape + (64,)), loss_row=c2.carve("loss_row", shape), pred=_carve_int64(c2, "pred", shape))
    before = _state_bits(probe, OPTIMISER)
    ev = probe.evaluate([batch])  # one batch through gd_lp_eval_accumulate; it leaves the optimiser alone
    assert all(np.array_equal(v, before[k]) for k, v in _state_bits(probe, OPTIMISER).items())
    probe._acc.zero_()
    r = probe._rows(B, **rows)
    import ctypes as C
    probe._call(probe._L.gd_lp_eval_accumulate, "gd_lp_eval_accumulate", obs, pm, rm, B, batch[6].data_ptr(), batch[7].data_ptr(),
                C.byref(r), probe._acc.data_ptr())
    c2.assert_guards(what + " rows")
    assert np.array_equal(rows["logits"].cpu().numpy().view(np.int32), z.view(np.int32))
    assert np.array_equal(rows["pred"].cpu().numpy().reshape(-1), host["pred"])
    lr_ = rows["loss_row"].cpu().numpy().reshape(-1)
    bound = ULPS * EPS * (2 * np.abs(z.reshape(-1, 64)).max(-1) + np.log(64.0) + 1.0)
    assert (np.abs(lr_.astype(np.float64) - host["loss_row"]) <= bound).all()
    pi = probe._part_i.cpu().numpy()
    assert pi.shape == (7, PC.PART_INTS)
    assert np.array_equal(pi[:, PC.N_HEAD:].sum(0).reshape(6, 64), host["counters"])
    assert [int(v) for v in pi[:, :5].sum(0)] == [host["correct"], host["M"], host["bad"], host["ood_correct"], host["ood_rows"]]
    ref = PREF.batch(z64, x64, mask, lab, exp)
    assert host["M"] == ref["M"] and host["bad"] == ref["bad"] >= 1
    pd = probe._part_d.cpu().numpy()
    assert abs(pd[:, 0].sum() - host["loss_sum"]) <= 8 * EPS * max(host["M"], 1) * (np.abs(z).max() + 5)
    if ref["M"]:
        assert ev["batches"] == 1 and abs(ev["eval/pos_loss"] - ref["loss"]) <= 2 * K * np.abs(z32.reshape(z64.shape) - z64).max() + 8 * EPS * (abs(ref["loss"]) + 1)
        assert ev["bad_labels"] == ref["bad"]


# ---- 3. one update

@pytest.mark.parametrize("B,A,R,model,exp", [(17, 64, 5, "early_lp", "other"), (2, 128, 5, "late_lp", "other"), (17, 64, 5, "late_lp", "ego"),
                                            (3, 64, 1, "early_lp", "ego"), (1, 64, 5, "early_lp", "other"), (17, 64, 5, "baseline", "other"),
                                            (3, 64, 1, "baseline", "ego")], ids=lambda v: str(v))
def test_one_update(B, A, R, model, exp):
    what = "update %s %s B=%d A=%d R=%d" % (model, exp, B, A, R)
    P = 5
    bc, probe, hd = _probe(B, A, R, model, exp, partials=P)
    Kin = probe.in_features
    batch, mask, lab = _batch(B, A, R, exp, "plain")
    x64, x32 = _rows64_32(B, A, R, model, exp)
    ref = PREF.batch(PREF.logits(x64, hd), x64, mask, lab, exp)
    _, g32 = PC.float32_head(x32.reshape(-1, x32.shape[-1]), hd, mask, lab, exp)
    assert ref["M"] > 0
    start = _state_bits(probe)
    w0 = probe.flat.cpu().numpy()[:probe.G].copy()
    probe.update(*batch)       # the first call of the shape
    first = _state_bits(probe)
    grad = probe.grad.cpu().numpy()
    _ratio(what + " grad", float(np.abs(grad.astype(np.float64) - ref["grad"]).max()), float(np.abs(g32 - ref["grad"]).max()))
    st = dict(zip(PC.STATS, probe.stats.cpu().numpy().tolist()))
    assert st["rows"] == ref["M"] and st["bad_labels"] == 0 and st["ood_rows"] == ref["ood_rows"]
    assert abs(st["accuracy"] - ref["accuracy"]) <= 1.0 / ref["M"] + EPS and abs(st["loss"] - ref["loss"]) <= 1e-3 * (1 + abs(ref["loss"]))
    # the reduction and AdamW: the host program on the kernel's own partials and gradient, bit for bit
    M, hgrad, hstats = PC.host_reduce(probe._part_f.cpu().numpy(), probe._part_d.cpu().numpy(), probe._part_i.cpu().numpy(), Kin)
    assert M == ref["M"] and np.array_equal(hgrad.view(np.int32), grad.view(np.int32))
    assert np.array_equal(hstats.view(np.int32), probe.stats.cpu().numpy().view(np.int32))
    w, m, v, step, pw = PC.host_adamw(w0, np.zeros(probe.G), np.zeros(probe.G), 0, [1.0, 1.0], [(M, grad)], LR, ADAM_EPS, K=Kin)
    assert np.array_equal(w.view(np.int32), probe.flat.cpu().numpy()[:probe.G].view(np.int32)), what
    assert np.array_equal(m.view(np.int32), probe.exp_avg.cpu().numpy().view(np.int32))
    assert np.array_equal(v.view(np.int32), probe.exp_avg_sq.cpu().numpy().view(np.int32))
    assert int(probe._step.item()) == step == 1 and np.array_equal(pw, probe._beta_pow.cpu().numpy())
    assert float(probe.flat[-1].item()) == 0.0
    # the packed weights are the flat ones re-packed (the padding columns still zero)
    repacked = torch.index_select(probe.flat, 0, probe._index)
    assert torch.equal(repacked, probe.packed)
    assert not np.array_equal(first["flat"], start["flat"])
    # M = 0: every buffer's bits and the step count stay, `skipped` advances; no host synchronisation
    empty, _, _ = _batch(B, A, R, exp, "empty")
    _no_sync(lambda: probe.update(*empty))
    after = _state_bits(probe)
    assert all(np.array_equal(after[k], first[k]) for k in first), what + ": an empty batch moved something"
    counts = probe._counts.cpu().numpy().tolist()
    assert counts == [1, 1, 0]
    # a label out of range is counted and changes nothing else: the same step as with that row unselected
    bad, bmask, blab = _batch(B, A, R, exp, "bad")
    _, p2, _ = _probe(B, A, R, model, exp, partials=P)
    _, p3, _ = _probe(B, A, R, model, exp, partials=P)
    p2.update(*bad)
    drop = (blab < 0) | (blab > 63)
    m3 = bmask.copy()
    m3[drop] = exp == "other"
    l3 = np.where(drop, 0, blab)
    d_m3, d_l3 = _dev(m3, l3)
    p3.update(*(bad[:6] + (d_m3, d_l3)))
    s2, s3 = _state_bits(p2), _state_bits(p3)
    nbad = int((drop & PC.selected(bmask, exp)).sum())
    assert nbad >= 1 and p2._counts.cpu().numpy().tolist()[2] == nbad and p3._counts.cpu().numpy().tolist()[2] == 0
    for k in s2:
        if k != "stats":
            assert np.array_equal(s2[k], s3[k]), (what, k)
    assert np.array_equal(s2["stats"][:28], s3["stats"][:28])  # all but the bad-label count
    # the same call twice from the same state gives equal bits
    _, p4, _ = _probe(B, A, R, model, exp, partials=P)
    _no_sync(lambda: p4.update(*batch))
    s4 = _state_bits(p4)
    assert all(np.array_equal(s4[k], first[k]) for k in first), what + ": two runs differ"


def test_one_row_selected():
    B, A, R = 3, 64, 1
    for exp in PC.EXPS:
        bc, probe, hd = _probe(B, A, R, "early_lp", exp)
        batch, mask, lab = _batch(B, A, R, exp, "one")
        x64, _ = _rows64_32(B, A, R, "early_lp", exp)
        ref = PREF.batch(PREF.logits(x64, hd), x64, mask, lab, exp)
        probe.update(*batch)
        assert ref["M"] == 1 and probe.stats.cpu().numpy()[6] == 1.0
        g = probe.grad.cpu().numpy().astype(np.float64)
        assert np.abs(g - ref["grad"]).max() <= 1e-4 * (1 + np.abs(ref["grad"]).max())
        out = probe.losses()
        assert out["steps"] == 1 and out["skipped"] == 0 and out["pos_accuracy"] in (0.0, 1.0)
        assert abs(out["pos_loss"] - ref["loss"]) <= 1e-3 * (1 + ref["loss"])


# ---- 4. three updates against the float64 pipeline

@pytest.mark.parametrize("model,exp", [("early_lp", "other"), ("late_lp", "ego")])
def test_three_updates_against_the_float64_pipeline(model, exp):
    """loss, accuracy and F1 per step, twice.  (a) Against float64 on the weights the device itself holds before the step: the
    bound is the logits' own error K E (the loss is 2-Lipschitz in the logits); accuracy and F1 are exact unless a row's two
    largest float64 logits lie within twice that bound.  (b) Against an independent float64 pipeline (nn.Linear,
    cross_entropy, torch.optim.AdamW): on top of (a), what the gradient's error K E_grad does to the weights -- AdamW's
    normalised step lr g / (|g| + eps) moves by at most lr / eps per unit of gradient error -- through a row of 64 features
    and a bias.  That worst case is loose (every weight erring in the same direction); the bit-for-bit AdamW check of
    test_one_update is the tight one."""
    B, A, R = 17, 64, 5
    bc, probe, hd = _probe(B, A, R, model, exp)
    x64, x32 = _rows64_32(B, A, R, model, exp)
    lin = torch.nn.Linear(64, 64).double()
    lin.load_state_dict({"weight": hd["head.weight"].double(), "bias": hd["head.bias"].double()})
    opt = torch.optim.AdamW(lin.parameters(), lr=float(np.float32(LR)), eps=float(np.float32(ADAM_EPS)))
    xt = torch.from_numpy(x64.reshape(-1, 64))
    xmax = float(np.abs(x64).max())
    kinds = ("plain", "empty", "bad")
    made = 0
    for s, kind in enumerate(kinds):
        batch, mask, lab = _batch(B, A, R, exp, kind)
        z64 = lin(xt).detach().numpy()
        ref = PREF.batch(z64, x64.reshape(-1, 64), mask, lab, exp)
        z32, g32 = PC.float32_head(x32.reshape(-1, 64), {"head.weight": lin.weight.detach().float(), "head.bias": lin.bias.detach().float()},
                                   mask, lab, exp)
        own = {k: v.cpu() for k, v in probe.state_dict().items()}
        probe.update(*batch)
        if ref["M"] == 0:
            continue
        Ez = float(np.abs(z32 - z64).max())
        mine = PREF.batch(PREF.logits(x64.reshape(-1, 64), own), x64.reshape(-1, 64), mask, lab, exp)
        got = dict(zip(PC.STATS, probe.stats.cpu().numpy().tolist()))
        assert abs(got["loss"] - mine["loss"]) <= 2 * K * Ez + 8 * EPS * (abs(mine["loss"]) + 1)
        gap = np.sort(PREF.logits(x64.reshape(-1, 64), own)[mine["use"]], -1)
        if ((gap[:, -1] - gap[:, -2]) > 2 * K * Ez).all():
            assert abs(got["accuracy"] - mine["accuracy"]) <= 2 * EPS and abs(got["f1_macro"] - mine["f1"]) <= 2 * EPS
        Eg = float(np.abs(g32 - ref["grad"]).max())
        tol = K * Ez + made * 65 * xmax * (LR / ADAM_EPS) * K * Eg
        made += 1
        st = dict(zip(PC.STATS, probe.stats.cpu().numpy().tolist()))
        print("LP STEP %s %s step %d loss %.6f ref %.6f tol %.2e" % (model, exp, s, st["loss"], ref["loss"], 2 * tol))
        assert abs(st["loss"] - ref["loss"]) <= 2 * tol + 8 * EPS * (abs(ref["loss"]) + 1)
        top = np.sort(z64[ref["use"]], -1)
        near = int(((top[:, -1] - top[:, -2]) <= 2 * tol).sum())
        assert abs(st["accuracy"] - ref["accuracy"]) <= near / ref["M"] + 2 * EPS
        if near == 0:
            assert abs(st["f1_macro"] - ref["f1"]) <= 2 * EPS
        u = torch.from_numpy(ref["use"])
        opt.zero_grad()
        torch.nn.functional.cross_entropy(lin(xt)[u], torch.from_numpy(lab.reshape(-1))[u]).backward()
        opt.step()
    out = probe.losses()
    assert out["steps"] == 2 and out["skipped"] == 1 and out["bad_labels"] >= 1 and probe.host_reads == 1
    assert probe.losses()["steps"] == 0
    # the optimiser state loads into torch.optim.AdamW over an nn.Linear(64, 64) and back
    sd = probe.optimizer_state_dict()
    lin32 = torch.nn.Linear(64, 64).cuda()
    lin32.load_state_dict({"weight": probe.state_dict()["head.weight"], "bias": probe.state_dict()["head.bias"]})
    topt = torch.optim.AdamW(lin32.parameters(), lr=LR, eps=ADAM_EPS)
    topt.load_state_dict(sd)
    assert float(topt.state[lin32.weight]["step"]) == 2.0
    assert torch.equal(topt.state[lin32.bias]["exp_avg_sq"], probe._views(probe.exp_avg_sq)["head.bias"])
    before = _state_bits(probe)
    probe.load_optimizer_state_dict(topt.state_dict())
    after = _state_bits(probe)
    assert all(np.array_equal(after[k], before[k]) for k in before)
    with pytest.raises(ValueError, match="param group"):
        probe.load_optimizer_state_dict({"state": {}, "param_groups": [{"params": [0]}]})


# ---- 5. evaluate

@pytest.mark.parametrize("exp", PC.EXPS)
def test_evaluate_over_two_unequal_batches_and_an_empty_one(exp):
    B, A, R = 17, 64, 5
    model = "late_lp"
    bc, probe, hd = _probe(B, A, R, model, exp)
    batch, mask, lab = _batch(B, A, R, exp, "plain")
    empty, emask, _ = _batch(B, A, R, exp, "empty")
    cuts = ((0, 11), (11, 17))
    batches = [tuple(t[lo:hi] for t in batch) for lo, hi in cuts]
    batches.insert(1, tuple(t[:4] for t in empty))
    x64, x32 = _rows64_32(B, A, R, model, exp)
    z64 = PREF.logits(x64, hd)
    z32, _ = PC.float32_head(x32.reshape(-1, 64), hd, mask, lab, exp)
    E = float(np.abs(z32.reshape(z64.shape) - z64).max())
    refs = [PREF.batch(z64[lo:hi], x64[lo:hi], mask[lo:hi], lab[lo:hi], exp) for lo, hi in cuts]
    refs.insert(1, PREF.batch(z64[:4], x64[:4], emask[:4], lab[:4], exp))
    want = PREF.evaluate(refs)
    probe.evaluate(batches)  # the first call of these shapes
    torch.cuda.synchronize()
    reads, real = [], torch.Tensor.cpu

    def counted(t, *a, **k):
        torch.cuda.set_sync_debug_mode(0)
        reads.append(1)
        return real(t, *a, **k)

    torch.Tensor.cpu = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = probe.evaluate(batches)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        torch.Tensor.cpu = real
    assert len(reads) == 1
    assert got["batches"] == want["batches"] == 2 and got["skipped"] == want["skipped"] == 1
    top = np.sort(z64.reshape(-1, 64), -1)
    if ((top[:, -1] - top[:, -2]) > 2 * K * E).all():  # no prediction can differ, so the counts are exact
        for k in ("eval/pos_accuracy", "eval/pos_f1_macro", "eval/ood_accuracy", "eval/ood_f1_macro"):
            assert abs(got[k] - want[k]) <= 4 * EPS, (k, got[k], want[k])
    for k in ("eval/pos_loss", "eval/ood_loss"):
        assert abs(got[k] - want[k]) <= 2 * K * E + 8 * EPS * (abs(want[k]) + 1), (k, got[k], want[k])
    # a short batch weighs as much as a full one: not the mean over the rows
    whole = PREF.batch(z64, x64, mask, lab, exp)
    assert abs(want["eval/pos_loss"] - whole["loss"]) > 10 * (2 * K * E + 8 * EPS * (abs(want["eval/pos_loss"]) + 1))


# ---- 6. end to end on the committed scenes

def test_recorded_episode_to_future_dataset_to_fit():
    from gpudrive_lab_amd.recorder import ExpertRecorder
    from tests import parity as P
    A, R = 128, 5
    sim = P.make_gpu_sim([SCENE_407, SCENE_4], max_agents=A, knn_order=0, dynamicsModel=2, collisionBehaviour=1,
                         roadObservationAlgorithm=1, isStaticAgentControlled=0, polylineReductionThreshold=0.1,
                         observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0, initOnlyValidAgentsAtFirstStep=1,
                         IgnoreNonVehicles=1)
    try:
        episode = ExpertRecorder(sim).record()
        bc = _policy(A, R, BC.state_dict(R), chunk_rows=32)
        for exp in PC.EXPS:
            ds = episode.future_dataset(rollout_len=R, pred_len=1, future_step=5, exp=exp)
            n = len(ds)
            assert n > 100
            bs = n // 3 + 1
            hd = PC.head(64)
            fitted = LP.DeviceLinearProbe(bc, hd, model="early_lp", exp=exp, lr=LR, eps=ADAM_EPS)
            g = torch.Generator(device="cuda")
            g.manual_seed(3)
            evals = fitted.fit(ds, total_gradient_steps=3, batch_size=bs, eval_ds=ds, eval_freq=3, generator=g)
            assert len(evals) == 1 and evals[0][0] == 3 and np.isfinite(evals[0][1]["eval/pos_loss"])
            assert 0.0 <= evals[0][1]["eval/pos_accuracy"] <= 1.0 and evals[0][1]["batches"] >= 1
            # the same batches fed to update one by one
            manual = LP.DeviceLinearProbe(bc, hd, model="early_lp", exp=exp, lr=LR, eps=ADAM_EPS)
            g.manual_seed(3)
            for i, batch in enumerate(ds.batches(bs, shuffle=True, generator=g)):
                manual.update(*batch)
            keys = OPTIMISER + ("grad",)  # (`stats` is the evaluation's last batch after fit)
            a, b = _state_bits(fitted, keys), _state_bits(manual, keys)
            assert [k for k in a if not np.array_equal(a[k], b[k])] == [], exp
            best = fitted.best_state_dict()
            assert best is not None and all(torch.equal(best[k], fitted.state_dict()[k]) for k in best)  # the evaluated weights
            out = fitted.losses()
            assert out["steps"] == 3 and out["skipped"] == 0 and np.isfinite(out["pos_loss"]) and out["bad_labels"] == 0
            with pytest.raises(ValueError, match="exp"):
                fitted.fit(episode.future_dataset(rollout_len=R, pred_len=1, future_step=5, exp="ego" if exp == "other" else "other"), 1)
        with pytest.raises(ValueError, match="rollout_len"):
            fitted.fit(episode.future_dataset(rollout_len=3, pred_len=1, future_step=5, exp="ego"), 1)
    finally:
        sim.close()


class _Batches:
    """A stand-in dataset: the same batches every epoch."""

    def __init__(self, batches, exp, A, R):
        self._b, self.exp, self.max_agents, self.rollout_len = batches, exp, A, R

    def __len__(self):
        return len(self._b)

    def batches(self, batch_size, shuffle=True, generator=None, drop_last=False):
        return iter(self._b)


def test_fit_counts_no_step_for_a_batch_that_selects_nothing():
    """Epochs of (plain, empty, bad): three steps take four batches, the evaluation falls after the second STEP (the third batch),
    and fit stops in the middle of the second epoch.  The host never reads the device to decide a skip."""
    B, A, R, exp = 3, 64, 1, "other"
    bc, probe, hd = _probe(B, A, R, "early_lp", exp)
    bs = [_batch(B, A, R, exp, kind)[0] for kind in ("plain", "empty", "bad")]
    evals = probe.fit(_Batches(bs, exp, A, R), 3, batch_size=B, eval_ds=_Batches(bs, exp, A, R), eval_freq=2)
    assert [e[0] for e in evals] == [2] and evals[0][1]["batches"] == 2 and evals[0][1]["skipped"] == 1
    best = probe.best_state_dict()
    _, manual, _ = _probe(B, A, R, "early_lp", exp)
    for i in (0, 1, 2):
        manual.update(*bs[i])
    assert all(torch.equal(best[k], manual.state_dict()[k]) for k in best)  # the weights the evaluation saw, not the last ones
    manual.update(*bs[0])
    a, b = _state_bits(probe, OPTIMISER), _state_bits(manual, OPTIMISER)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    out = probe.losses()
    assert out["steps"] == 3 and out["skipped"] == 1 and out["bad_labels"] >= 1
    with pytest.raises(ValueError, match="selected no row"):
        probe.fit(_Batches(bs[1:2], exp, A, R), 1, batch_size=B)
    with pytest.raises(ValueError, match="max_agents|agents"):
        probe.fit(_Batches(bs, exp, 128, R), 1, batch_size=B)


# ---- 7. the input checks

def test_every_input_check_raises_before_a_launch():
    B, A, R = 3, 64, 1
    bc, probe, hd = _probe(B, A, R, "early_lp", "other")
    batch, mask, lab = _batch(B, A, R, "other")
    ego_batch, _, _ = _batch(B, A, R, "ego")
    obs, expert, valid, ego_mask, pm, rm, m, l_ = batch
    start = _state_bits(probe)
    carver = Carver()
    out = carver.carve("hidden", (B, A, 64))
    for kw in (dict(tap="rg_attn"), dict(out=out[:2]), dict(out=out.double()), dict(out=out.cpu())):
        with pytest.raises(ValueError):
            bc.hidden(obs, pm, rm, **dict(dict(out=out), **kw))
    for o, p_, r_ in ((obs[:, :, :-1].contiguous(), pm, rm), (obs.double(), pm, rm), (obs.cpu(), pm, rm), (obs, pm.int(), rm), (obs, pm, rm[:2])):
        with pytest.raises(ValueError):
            bc.hidden(o, p_, r_, out=out)
        with pytest.raises(ValueError):
            probe.update(o, expert, valid, ego_mask, p_, r_, m, l_)
        with pytest.raises(ValueError):
            probe.logits(o, p_, r_)
    carver.assert_guards("refused calls", written=False)
    bad = [dict(m=m.float()), dict(m=m[:, :-1].contiguous()), dict(l=l_.int()), dict(l=l_[:2]), dict(m=m.cpu()), dict(l=l_.t().contiguous().t())]
    for b in bad:
        with pytest.raises(ValueError):
            probe.update(obs, expert, valid, ego_mask, pm, rm, b.get("m", m), b.get("l", l_))
    with pytest.raises(ValueError, match="exp is 'other'"):  # an 'ego' batch into an 'other' probe
        probe.update(*ego_batch)
    with pytest.raises(ValueError):
        probe.update(*batch, logits=torch.empty((B, A - 1, 32), device="cuda"))
    with pytest.raises(ValueError):
        probe.predict(obs, pm, rm, out=torch.empty((B, A - 1), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="unexpected"):
        probe.load_state_dict(dict(hd, extra=hd["head.bias"]))
    with pytest.raises(ValueError, match="eval_freq"):
        probe.fit([batch], 1, eval_ds=[batch])
    assert all(np.array_equal(v, start[k]) for k, v in _state_bits(probe).items())
    assert probe._counts.cpu().numpy().tolist() == [0, 0, 0]
    # the probe follows the policy's blob: new backbone weights change the logits with no call on the probe
    z0 = probe.logits(obs, pm, rm).cpu().numpy()
    bc.load_state_dict({k: v.cuda() for k, v in BC.state_dict(R, seed=11).items()})
    assert np.abs(probe.logits(obs, pm, rm).cpu().numpy() - z0).max() > 0.1
