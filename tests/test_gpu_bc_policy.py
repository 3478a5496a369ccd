"""GPU suite: the device BC policy forward (gpudrive_lab_amd.bc_policy.DeviceBCPolicy; gd_bc_forward) against the float64
restatement (tests/bc_reference.py, itself pinned to the reference module by tests/test_bc_policy.py) on the shapes and
constructed samples of tests/bc_cases.py.

context, means, clamped raw covariances, weights and NLL: the yardstick E of a case and an output is the maximum absolute
error of torch's float32 CPU forward of the stand-in module (bc_cases.StandIn) against float64 on that case; the kernel's
error must be <= K E.  K was set from ratios measured ONCE on an MI355X (printed per case by this test with -s):
    (B, A, R)    context  means  log_covariances  weights  nll
    (1, 64, 5)   0.80     0.92   1.71             8.62     6.22
    (3, 64, 1)   0.95     1.17   1.28             1.02     3.43
    (17, 64, 5)  1.06     1.31   0.87             0.98     1.16
    (2, 128, 5)  1.22     1.41   1.51             0.79     0.83
The largest, 8.62, is the one-sample case, where the yardstick itself is one draw (its weights' E was 4.2e-8 against the
kernel's 3.6e-7, a few float32 ulps of a weight near 1; with 3 and 17 samples the ratios are about 1).  K is the next power
of two at or above twice the largest: 32.  A ratio above 16 would be a bug, not a bound to raise.  (The recorded-episode
batch, A = 128: 1.03, 1.23, 0.99, 1.05, 0.25.)
The configurations of bc_cases.EDGE_CASES (test_forward_at_the_edge_configurations; weights and inputs are the backward
tests', bc_grad_reference.case_inputs) under the same K, measured once:
    name (B, A, R)            context  means  log_covariances  weights  nll
    top (3, 64, 8)            0.89     1.61   1.90             1.56     2.52
    sweep (3, 64, 5)          1.08     1.24   0.60             1.48     0.31
    c9 (3, 64, 1)             1.56     1.47   1.75             2.85     1.84
    c10 (3, 64, 1)            1.56     1.71   1.53             0.72     0.50
    deep_branch (2, 128, 2)   1.08     0.75   0.74             1.28     0.49
    deep_fusion (3, 64, 2)    0.64     0.83   0.71             2.73     0.73
    defaults (130, 64, 1)     0.86     0.97   0.90             0 / 0    1.61
(`defaults` has one component: its weight is exactly 1 on both sides.)  Depth does not move the ratio: `top` sums over twelve
self-attention layers and stays where the three-row case of five layers is.  gd_bc_eval_accumulate called directly with 63,
64, 65, 130 and 513 rows stays within 0.02 of its bound (n + 8) 2^-24 max(1, |value|).
Actions, the component and ego_attn_score's normalisation are held to the rule in float64 on the kernel's OWN mixture
parameters: the deterministic action exactly, the draw where u falls to within 1e-5 of the running sum."""
import numpy as np
import pytest
import torch

from tests import bc_cases as BC
from tests import bc_reference as REF
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON
from tests.test_bc_policy import case

pytestmark = pytest.mark.gpu

K = 32
CANARY_BITS = 0x7FC0DEAD  # a NaN payload no kernel writes
GUARD = 64                # int32 words either side of every carved tensor
ALL = ("context", "means", "log_covariances", "covariances", "weights", "actions", "nll", "ego_attn_score", "component")
EPS = 2.0 ** -24


class Carver:
    """Tensors carved from canary-filled int32 buffers with GUARD words either side."""

    def __init__(self):
        self.whole = {}

    def carve(self, name, shape, dtype=torch.float32):
        words = int(np.prod(shape, dtype=np.int64))
        buf = torch.full((GUARD + words + GUARD,), CANARY_BITS, dtype=torch.int32, device="cuda")
        self.whole[name] = (buf, words)
        return buf[GUARD:GUARD + words].view(dtype).view(shape)

    def assert_guards(self, what, written=True):
        for name, (buf, words) in self.whole.items():
            h = buf.cpu().numpy()
            assert (h[:GUARD] == CANARY_BITS).all() and (h[GUARD + words:] == CANARY_BITS).all(), \
                "%s: bytes beside %s were written" % (what, name)
            if written:
                assert (h[GUARD:GUARD + words] != CANARY_BITS).all(), "%s: %s was not written whole" % (what, name)
            else:
                assert (h == CANARY_BITS).all(), "%s: %s was touched" % (what, name)


def _carved_outputs(bc, B):
    carver = Carver()
    out = {k: carver.carve(k, bc._OUT_SHAPES[k](bc, B), torch.int32 if k == "component" else torch.float32) for k in ALL}
    return carver, out


def _no_sync(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _host(res):
    return {k: v.cpu().numpy().copy() for k, v in res.items()}


def _same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), "%s: %s differs" % (what, k)


def _yardstick(c, A):
    if "E" not in c:
        ref = dict(c["ref"])
        ref["nll"] = REF.nll(ref["means"], ref["log_covariances"], ref["weights"], c["expert"][:, 0])
        c["ref_nll"] = ref["nll"]
        c["E"] = BC.yardstick(BC.standin_float32(c["sd"], c["obs"], c["pm"], c["rm"], A, c.get("cfg", BC.CFG), expert=c["expert"]), ref)
    return c["E"]


def _compare(what, got, c, A, keys=BC.COMPARED + ("nll",)):
    """The kernel's error against the restatement per output, as multiples of the case's yardstick; asserts <= K."""
    E = _yardstick(c, A)
    ratios = {}
    for k in keys:
        want = c["ref_nll"] if k == "nll" else c["ref"][k]
        err = float(np.abs(got[k].astype(np.float64).reshape(want.shape) - want).max())
        ratios[k] = err / E[k] if E[k] > 0 else (0.0 if err == 0 else np.inf)
        print("BC RATIO %s %s err %.3e E %.3e ratio %.2f" % (what, k, err, E[k], ratios[k]))
    assert max(ratios.values()) <= K, (what, ratios)
    return ratios


def _check_rule(what, got, u, z, det, A):
    """component, actions and ego_attn_score against the float64 rule on the kernel's own mixture parameters."""
    w = got["weights"][:, 0].astype(np.float64)
    means, cov = got["means"][:, 0].astype(np.float64), got["covariances"][:, 0].astype(np.float64)
    n, C_ = w.shape
    comp, r = got["component"].astype(np.int64), np.arange(n)
    assert (comp >= 0).all() and (comp < C_).all(), what
    assert (np.abs(cov - np.exp(got["log_covariances"][:, 0].astype(np.float64))) <= 4 * EPS * cov).all(), what
    if det:
        assert np.array_equal(comp, w.argmax(-1)), what + ": not the first component of maximal weight"
        assert np.array_equal(got["actions"][:, 0], got["means"][r, 0, comp]), what + ": the deterministic action is not that mean"
    else:
        run = REF.running_sums(w)
        lo, hi = np.where(comp > 0, run[r, np.maximum(comp - 1, 0)], 0.0), run[r, comp]
        u64 = u.astype(np.float64)
        last = comp == C_ - 1
        assert (lo - 1e-5 <= u64).all() and ((u64 < hi + 1e-5) | last).all(), what + ": the draw is not where u falls"
        want = means[r, comp] + np.sqrt(cov[r, comp]) * z.astype(np.float64)
        assert (np.abs(got["actions"][:, 0] - want) <= 8 * EPS * (np.abs(want) + np.abs(z) * np.sqrt(cov[r, comp]) + 1)).all(), what
    s = got["ego_attn_score"].astype(np.float64)
    assert (s >= 0).all() and (np.abs(s.sum(-1) - 1.0) <= (A + 8) * EPS).all(), what + ": ego_attn_score rows do not sum to 1"


def _policy(A, R, sd=None, cfg=BC.CFG, **kw):
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    return DeviceBCPolicy.from_state_dict(sd if sd is not None else BC.state_dict(R), max_agents=A, num_stack=R, **cfg, **kw)


def _forward_checks(B, A, R, cfg, what):
    """Everything the forward is held to at one case: K E on the compared outputs, nll and ego_attn_score; the float64 rule on the
    kernel's own mixture parameters for the deterministic action and the draws; canaries, every byte written, equal bits
    between calls.  Returns (case, the outputs on the host)."""
    c = case(B, A, R, cfg)
    C_, clip = cfg["n_components"], cfg["clip_value"]
    bc = _policy(A, R, c["sd"], cfg)
    obs, pm, rm, expert, u, z = _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["u"], c["z"])
    fresh = _host(bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert))
    assert fresh["actions"].shape == (B, 1, 3) and fresh["means"].shape == (B, 1, C_, 3) and fresh["weights"].shape == (B, 1, C_)
    carver, out = _carved_outputs(bc, B)
    # the second call of the shape: no host synchronisation, out= buffers, canaries either side, every byte written
    _no_sync(lambda: bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert, out=out))
    carver.assert_guards(what)
    got = _host(out)
    _same_bits(fresh, got, what + " out= against fresh tensors")
    _same_bits(got, _host(bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert)), what + " two calls")
    _compare(what, got, c, A)
    _check_rule(what + " deterministic", got, None, None, True, A)
    E = _yardstick(c, A)
    serr = np.abs(got["ego_attn_score"].astype(np.float64) - c["ref"]["ego_attn_score"]).max()
    print("BC RATIO %s ego_attn_score err %.3e E %.3e" % (what, serr, E["ego_attn_score"]))  # (E is 0 where one key is left)
    assert serr <= K * E["ego_attn_score"]
    for i, kind in enumerate(c["kinds"]):
        if "a" in kind:  # every partner masked: the row is uniform over all A - 1 keys, as the reference's is
            assert np.abs(got["ego_attn_score"][i] - 1.0 / (A - 1)).max() <= 4 * EPS
    # the public methods are views of the same call
    assert np.array_equal(bc(obs, pm, rm, deterministic=True).cpu().numpy(), got["actions"])
    assert np.array_equal(bc.context(obs, pm, rm).cpu().numpy(), got["context"])
    m, cv, w = bc.gmm_params(obs, pm, rm)
    assert np.array_equal(m.cpu().numpy(), got["means"]) and np.array_equal(cv.cpu().numpy(), got["covariances"])
    assert np.array_equal(w.cpu().numpy(), got["weights"]) and np.array_equal(bc.nll(obs, pm, rm, expert).cpu().numpy(), got["nll"])
    # the draw: seeded uniforms, then u = 0 and u just below 1 (g)
    for uu in (c["u"], BC.edge_uniforms(B)):
        d_u, = _dev(uu)
        drawn = _host(bc.forward(obs, pm, rm, ALL, deterministic=False, u=d_u, z=z, expert_actions=expert))
        _same_bits({k: got[k] for k in ("context", "means", "weights", "nll")}, {k: drawn[k] for k in ("context", "means", "weights", "nll")},
                   what + " drawn against deterministic")
        _check_rule(what + " drawn", drawn, uu, c["z"], False, A)
        assert np.array_equal(bc(obs, pm, rm, u=d_u, z=z).cpu().numpy(), drawn["actions"])
    own = drawn["weights"][:, 0]
    assert np.array_equal(drawn["component"][0::2], np.argmax(own > 0, axis=-1)[0::2])  # u = 0: the first component with any mass
    reached = np.cumsum(own.astype(np.float64), -1)[:, :-1].max(-1, initial=0.0) > BC.edge_uniforms(2)[1] - 1e-5
    assert (drawn["component"][1::2] == C_ - 1)[~reached[1::2]].all()  # u just below 1: the last, unless the sum is there before
    # (f): raw covariances below clip_value and above 3.58352 are clamped exactly (pushed there where the mixture has room)
    lc = got["log_covariances"][:, 0].reshape(B, -1)
    if cfg is BC.CFG:
        assert (lc[:, 1] == np.float32(-20.0)).all() and (lc[:, 5] == np.float32(3.58352)).all()
    # and wherever the float64 raw value lies outside a bound by more than the clamp margin, whatever pushed it there
    raw = c["ref"]["raw"][:, 3 * C_:6 * C_]
    below, above = raw < clip - 1e-3, raw > REF.COV_MAX + 1e-3
    assert (lc[below] == np.float32(clip)).all() and (lc[above] == np.float32(3.58352)).all()
    assert C_ < 2 or (below.any() and above.any()), what + ": the case has no covariance outside the clamp"
    return c, got


@pytest.mark.parametrize("B,A,R", BC.SHAPES, ids=lambda v: str(v))
def test_forward_against_the_float64_restatement(B, A, R):
    _forward_checks(B, A, R, BC.CFG, "B=%d A=%d R=%d" % (B, A, R))


@pytest.mark.parametrize("name", [c[0] for c in BC.EDGE_CASES])
def test_forward_at_the_edge_configurations(name):
    """bc_cases.EDGE_CASES through the same checks.  Ratios measured once on an MI355X: the table in DESIGN section 2."""
    B, A, R, cfg = BC.EDGE[name]
    c, got = _forward_checks(B, A, R, cfg, "%s B=%d A=%d R=%d" % (name, B, A, R))
    if name == "deep_fusion":  # a floor above 0: it cuts through the raw covariances, and the device's equal it exactly below
        raw = c["ref"]["raw"][:, 3 * cfg["n_components"]:6 * cfg["n_components"]]
        below, above = raw < cfg["clip_value"] - 1e-3, (raw > cfg["clip_value"] + 1e-3) & (raw < REF.COV_MAX - 1e-3)
        assert below.any() and above.any()
        lc = got["log_covariances"][:, 0].reshape(B, -1)
        assert (lc[below] == np.float32(cfg["clip_value"])).all() and (lc[above] > np.float32(cfg["clip_value"])).all()


@pytest.mark.parametrize("n", [63, 64, 65, 130, 513])
def test_eval_accumulate_past_one_row_per_lane(n):
    """gd_bc_eval_accumulate called directly, two batches of n rows into one accumulator between canaries, against
    bc_reference.evaluate's sums in float64: (n + 8) 2^-24 max(1, |value|) per mean and per sum, the counts and the number of
    batches exact, and the eight numbers of evaluate() from them."""
    from gpudrive_lab_amd import _capi
    from tests.test_bc_edge_cases import eval_batches, eval_bound
    batches = eval_batches(n)
    want = REF.evaluate_sums(batches)
    carver = Carver()
    acc = carver.carve("acc", (11,))
    acc.zero_()
    L = _capi.lib()
    for nll, pred, ex in batches:
        d_nll, d_pred, d_ex = _dev(nll, pred, ex)
        _no_sync(lambda: _capi.check(L.gd_bc_eval_accumulate(n, d_nll.data_ptr(), d_pred.data_ptr(), d_ex.data_ptr(), acc.data_ptr(), None)))
        torch.cuda.synchronize()
    carver.assert_guards("gd_bc_eval_accumulate n = %d" % n)
    got = acc.cpu().numpy().astype(np.float64)
    bound = eval_bound(n, want)
    print("BC EVAL n=%d err/bound %s" % (n, " ".join("%.2f" % v for v in (np.abs(got - want) / bound)[:7])))
    assert (np.abs(got - want)[:7] <= bound[:7]).all(), (n, got, want)
    assert np.array_equal(got[7:], want[7:]) and got[10] == 2, (n, got[7:], want[7:])
    assert (want[7:10] > 0).all() and (want[7:10] < 2 * n).all(), "experts on both sides of every threshold"
    eight = np.array(REF.evaluate(batches)[:7])
    mine = np.concatenate([got[:4] / got[10], got[4:7] / got[7:10]])
    assert (np.abs(mine - eight) <= eval_bound(n, eight)).all()


def test_masked_features_do_not_reach_the_context_and_all_masked_rows_are_uniform():
    B, A, R = 17, 64, 5
    c = case(B, A, R)
    bc = _policy(A, R, c["sd"])
    obs, pm, rm = _dev(c["obs"], c["pm"], c["rm"])
    obs2, = _dev(BC.overwrite_masked(c["obs"], c["pm"], c["rm"], A))
    assert not torch.equal(obs, obs2)
    a, b = bc.context(obs, pm, rm).cpu().numpy(), bc.context(obs2, pm, rm).cpu().numpy()
    some = np.array([not ("a" in k or "b" in k) for k in c["kinds"]])  # a key left in every attention
    assert some.sum() >= 12 and np.array_equal(a[some].view(np.int32), b[some].view(np.int32))
    # (a), (b): the kernel matches the restatement's uniform attention, which the -inf variant is far from
    E = _yardstick(c, A)["context"]
    inf = REF.forward(c["sd"], c["obs"], c["pm"], c["rm"], A, **BC.CFG, wrong="inf_fill")["context"]
    full = ~some
    assert full.sum() == 3
    assert (np.abs(inf[full] - c["ref"]["context"][full]).max(-1) > 1000 * K * E).all()
    assert np.abs(a[full].astype(np.float64) - c["ref"]["context"][full]).max() <= K * E


def test_rows_above_the_chunk_equal_the_concatenation_of_the_chunks():
    B, A, R = 17, 64, 5
    c = case(B, A, R)
    obs, pm, rm, expert, u, z = _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["u"], c["z"])
    small, whole = _policy(A, R, c["sd"], chunk_rows=5), _policy(A, R, c["sd"])
    assert small.nbytes(B) < whole.nbytes(B) and whole.nbytes(B) == whole.nbytes(1) + 16 * (whole.nbytes(2) - whole.nbytes(1))
    got = _host(small.forward(obs, pm, rm, ALL, deterministic=False, u=u, z=z, expert_actions=expert))
    parts = [_host(whole.forward(obs[i:i + 5], pm[i:i + 5], rm[i:i + 5], ALL, deterministic=False, u=u[i:i + 5], z=z[i:i + 5],
                                 expert_actions=expert[i:i + 5])) for i in range(0, B, 5)]
    _same_bits(got, {k: np.concatenate([p[k] for p in parts]) for k in ALL}, "chunk 5 against slices")
    _same_bits(got, _host(whole.forward(obs, pm, rm, ALL, deterministic=False, u=u, z=z, expert_actions=expert)), "chunk 5 against one chunk")


def test_evaluate_over_two_unequal_batches():
    B, A, R = 17, 64, 5
    c = case(B, A, R)
    bc = _policy(A, R, c["sd"])
    obs, pm, rm, expert = _dev(c["obs"], c["pm"], c["rm"], c["expert"])
    cuts = ((0, 11), (11, 17))
    batches = [(obs[lo:hi], expert[lo:hi], pm[lo:hi], rm[lo:hi], None) for lo, hi in cuts]
    stats = _no_sync_but_the_last_read(bc, batches)
    from gpudrive_lab_amd.bc_policy import EVAL_NAMES
    assert tuple(stats) == EVAL_NAMES and stats["tom_loss"] == 0.0
    got = np.array([stats[k] for k in EVAL_NAMES])
    # (1) the accumulation itself: the reference's averaging on the kernel's OWN rows, within float32 summation
    own = _host(bc.forward(obs, pm, rm, ("nll", "actions"), deterministic=True, expert_actions=expert))
    mine = REF.evaluate([(own["nll"][lo:hi], own["actions"][lo:hi, 0], c["expert"][lo:hi, 0]) for lo, hi in cuts])
    assert (np.abs(got - mine) <= (B + 8) * EPS * np.maximum(1.0, np.abs(mine))).all(), (got, mine)
    # (2) and the restatement's eight numbers: the rows' own error on top
    E = _yardstick(c, A)
    _, act = REF.deterministic_action(c["ref"]["means"], c["ref"]["weights"])
    want = np.array(REF.evaluate([(c["ref_nll"][lo:hi], act[lo:hi], c["expert"][lo:hi, 0]) for lo, hi in cuts]))
    rows = np.array([E["nll"]] + [E["means"]] * 6 + [0.0])
    assert np.isfinite(want).all() and (np.abs(got - want) <= K * rows + (B + 8) * EPS * np.maximum(1.0, np.abs(want))).all(), (got, want)
    # a short last batch weighs as much as a full one: the mean of the two batch means, not the mean over the rows
    assert abs(want[0] - c["ref_nll"].mean()) > 100 * (K * E["nll"] + B * EPS * abs(want[0]))


def _no_sync_but_the_last_read(bc, batches):
    """evaluate() reads the device once, at the end: every launch before it runs under the sync-debug mode 'error'."""
    bc.evaluate(batches)  # the first call of these shapes allocates
    torch.cuda.synchronize()
    reads = []
    real = torch.Tensor.cpu

    def counted(t, *a, **k):
        torch.cuda.set_sync_debug_mode(0)
        reads.append(1)
        return real(t, *a, **k)

    torch.Tensor.cpu = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats = bc.evaluate(batches)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        torch.Tensor.cpu = real
    assert len(reads) == 1
    return stats


def test_load_state_dict_changes_the_outputs_to_the_new_reference():
    B, A, R = 3, 64, 1
    c = case(B, A, R)
    bc = _policy(A, R, c["sd"])
    obs, pm, rm = _dev(c["obs"], c["pm"], c["rm"])
    before = bc.context(obs, pm, rm).cpu().numpy()
    sd2 = BC.state_dict(R, seed=11)
    bc.load_state_dict({k: v.cuda() for k, v in sd2.items()})
    ref2 = REF.forward(sd2, c["obs"], c["pm"], c["rm"], A, **BC.CFG)
    E2 = BC.yardstick(BC.standin_float32(sd2, c["obs"], c["pm"], c["rm"], A), ref2)
    got = _host(bc.forward(obs, pm, rm, BC.COMPARED))
    for k in BC.COMPARED:
        assert np.abs(got[k].astype(np.float64).reshape(ref2[k].shape) - ref2[k]).max() <= K * E2[k], k
    assert np.abs(got["context"] - before).max() > 0.1
    with pytest.raises(ValueError, match="shape"):
        bc.load_state_dict(BC.state_dict(2))


def test_tied_mixture_weights_take_the_first_index():
    B, A, R = 3, 64, 1
    c = case(B, A, R)
    bc = _policy(A, R, BC.with_tied_weights(c["sd"]))
    obs, pm, rm = _dev(c["obs"], c["pm"], c["rm"])
    got = _host(bc.forward(obs, pm, rm, ("weights", "component", "actions", "means")))
    w = got["weights"][:, 0]
    assert np.array_equal(w[:, 1].view(np.int32), w[:, 3].view(np.int32)) and (w[:, 1] > 0.49).all()  # (e) an exact tie at the top
    assert (got["component"] == 1).all() and np.array_equal(got["actions"][:, 0], got["means"][:, 0, 1])


def test_input_checks_raise_before_anything_is_launched():
    B, A, R = 3, 64, 1
    c = case(B, A, R)
    bc = _policy(A, R, c["sd"])
    obs, pm, rm, expert, u, z = _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["u"], c["z"])
    carver = Carver()
    out = carver.carve("actions", (B, 1, 3))
    bad = [
        dict(obs=obs[:, :, :-1].contiguous()), dict(obs=obs.double()), dict(obs=obs.cpu()), dict(obs=obs[:, 0]),
        dict(obs=torch.cat([obs, obs], 1)[:, ::2]),  # not contiguous
        dict(pm=pm.int()), dict(pm=pm[:, :, :-1].contiguous()), dict(rm=rm.float()), dict(rm=rm[:2]), dict(rm=rm.cpu()),
        dict(kw=dict(deterministic=False)), dict(kw=dict(deterministic=False, u=u)), dict(kw=dict(u=u[:2], z=z)),
        dict(kw=dict(u=u, z=z.double())), dict(kw=dict(deterministic=True, out=out[:2])), dict(kw=dict(deterministic=True, out=out.double())),
    ]
    for b in bad:
        kw = dict(deterministic=True, out=out)
        kw.update(b.get("kw", {}))
        with pytest.raises(ValueError):
            bc(b.get("obs", obs), b.get("pm", pm), b.get("rm", rm), **kw)
    with pytest.raises(ValueError, match="expert_actions"):
        bc.forward(obs, pm, rm, ("nll",))
    with pytest.raises(ValueError, match="expert_actions"):
        bc.nll(obs, pm, rm, expert[:, 0, :2].contiguous())
    with pytest.raises(ValueError, match="unknown output"):
        bc.forward(obs, pm, rm, ("logits",))
    with pytest.raises(ValueError, match="three tensors"):
        bc.gmm_params(obs, pm, rm, out=(out,))
    carver.assert_guards("refused calls", written=False)
    uint8 = bc(obs, pm.to(torch.uint8), rm.to(torch.uint8), deterministic=True, out=out)  # the masks may be uint8
    carver.assert_guards("uint8 masks")
    assert np.array_equal(uint8.cpu().numpy(), bc(obs, pm, rm, deterministic=True).cpu().numpy())


def test_recorded_episode_to_batch_to_policy():
    """ExpertRecorder.record() -> dataset() -> batch(sel) -> bc(...) with the dataset's own mask tensors, against the
    restatement on the same batch copied to the host."""
    from gpudrive_lab_amd.recorder import ExpertRecorder
    from tests import parity as P
    A, R = 128, 5
    sim = P.make_gpu_sim([TEST_JSON, SCENE_407, SCENE_4], max_agents=A, knn_order=0, dynamicsModel=2, collisionBehaviour=1,
                         roadObservationAlgorithm=1, isStaticAgentControlled=0, polylineReductionThreshold=0.1,
                         observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0, initOnlyValidAgentsAtFirstStep=1,
                         IgnoreNonVehicles=1)
    try:
        ds = ExpertRecorder(sim).record().dataset(rollout_len=R, pred_len=1)
        M = len(ds)
        assert M > 100
        sel = torch.tensor([0, 1, 3, M // 3, M // 2, M - 2, M - 1], dtype=torch.int64, device="cuda")  # windows with and without a prefix
        obs, expert, pm, rm, _ = ds.batch(sel)
        assert pm.dtype == torch.bool and rm.dtype == torch.bool and pm.shape[2] == A - 1  # an odd byte pitch
        sd = BC.state_dict(R)
        bc = _policy(A, R, sd)
        got = _host(bc.forward(obs, pm, rm, ALL, deterministic=True, expert_actions=expert))
        h = dict(sd=sd, obs=obs.cpu().numpy(), pm=pm.cpu().numpy(), rm=rm.cpu().numpy(), expert=expert.cpu().numpy())
        assert np.isfinite(h["obs"]).all() and h["pm"][:, -1].any() and not h["pm"][:, -1].all()
        h["ref"] = REF.forward(sd, h["obs"], h["pm"], h["rm"], A, **BC.CFG)
        _compare("recorded A=128 R=5", got, h, A)
        _check_rule("recorded", got, None, None, True, A)
        stats = bc.evaluate(ds, batch_size=M // 2 + 1)
        assert all(np.isfinite(stats[k]) for k in ("test_loss", "dx_loss", "dy_loss", "dyaw_loss"))
    finally:
        sim.close()
