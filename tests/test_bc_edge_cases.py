"""The configurations of bc_cases.EDGE_CASES without a GPU: the host-side layouts at every one of them (the blob's index, the
flat gradient, the optimiser's tensor table, the C side's tensor count), the float32 yardsticks of the forward and the
backward there, and five wrong rules -- each the RIGHT rule at bc_cases.CFG, which is why the suite at CFG alone could not
see it -- shown to leave the GPU tests' bound K E on the edge case named for it and to stay inside it on bc_cases.SHAPES."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_opt as BO
from gpudrive_lab_amd import bc_policy as BP
from gpudrive_lab_amd import bc_train as BT

from . import bc_cases as BC
from . import bc_grad_reference as GR
from . import bc_reference as REF
from . import bc_update_reference as UR
from .test_bc_policy import case
from .test_bc_update import C_ADAMW, OK, _structs

K = 32  # the bound of the GPU tests: error <= K E
NAMES = [c[0] for c in BC.EDGE_CASES]
_E = {}


def cfg_of(name):
    return BC.EDGE[name][3]


def _lay(R, cfg):
    return R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"]


def _yardstick(name):
    """The case, with its float32 stand-in's error against the float64 restatement per output (nll too)."""
    if not isinstance(name, str):
        B, A, R, cfg = name
        name = repr(GR.case_key(B, A, R, cfg))
    else:
        B, A, R, cfg = BC.EDGE[name]
    if name not in _E:
        c = case(B, A, R, cfg)
        ref = dict(c["ref"])
        ref["nll"] = REF.nll(ref["means"], ref["log_covariances"], ref["weights"], c["expert"][:, 0])
        _E[name] = (c, ref, BC.yardstick(BC.standin_float32(c["sd"], c["obs"], c["pm"], c["rm"], A, cfg, expert=c["expert"]), ref))
    return _E[name]


def _forward_ratios(c, ref, E, A, wrong):
    """What the GPU forward test measures, with the wrong rule in the kernel's place: error / E per compared output."""
    bad = REF.forward(c["sd"], c["obs"], c["pm"], c["rm"], A, **c["cfg"], wrong=wrong)
    bad["nll"] = REF.nll(bad["means"], bad["log_covariances"], bad["weights"], c["expert"][:, 0])
    return {k: float(np.abs(bad[k] - ref[k]).max()) / E[k] for k in BC.COMPARED + ("nll",)}


# ---- the table itself

def test_the_table_reaches_what_it_is_named_for():
    e = BC.EDGE
    assert NAMES == ["top", "sweep", "c9", "c10", "deep_branch", "deep_fusion", "defaults"]
    tensors = {n: len(BP.expected_shapes(*_lay(e[n][2], e[n][3]))) for n in NAMES}
    assert tensors["top"] == 288 and tensors["sweep"] == 252 and len(BP.expected_shapes(*_lay(1, BC.CFG))) == 204
    assert [7 * e[n][3]["n_components"] for n in ("c9", "c10", "top")] == [63, 70, 112]
    assert 13 * e["top"][2] == 104 and e["top"][3]["head_num_layers"] == 4
    f, b = e["deep_branch"][3]["num_layer"]
    assert b > f and e["deep_branch"][1] == 128 and (6 * e["deep_branch"][2]) % 2 == 0 and (13 * e["deep_branch"][2]) % 2 == 0
    f, b = e["deep_fusion"][3]["num_layer"]
    assert f > b and 0 < e["deep_fusion"][3]["clip_value"] < REF.COV_MAX
    assert e["defaults"][0] == BP.DEFAULT_CHUNK + 2
    for name in NAMES:
        B, A, R, cfg = e[name]
        assert GR.case_key(B, A, R, cfg) in GR.INPUT_SEEDS and GR.case_key(B, A, R, cfg)[-1] == cfg["clip_value"]
        sd = GR.state_dict(R, cfg)
        assert list(BP.check_bc_args(sd, max_agents=A, num_stack=R, **cfg)) == list(sd)  # the host checks accept every one
    # two cases differ from another key in the clamp alone: the key tells them apart
    assert GR.case_key(3, 64, 5, e["sweep"][3]) != GR.case_key(3, 64, 5, dict(e["sweep"][3], clip_value=-20.0))


# ---- the host-side layouts

@pytest.mark.parametrize("name", NAMES)
def test_layouts_at_every_edge_configuration(name):
    _, A, R, cfg = BC.EDGE[name]
    lay = _lay(R, cfg)
    f, b = cfg["num_layer"]
    shapes = BP.expected_shapes(*lay)
    index, G, end = BP.pack_index(*lay), BT.grad_floats(*lay), BO.tensor_end(shapes)
    # the blob's index: every parameter exactly once, nothing outside flat + its one zero
    real = index[index != G]
    assert index.min() >= 0 and index.max() <= G and np.array_equal(np.sort(real), np.arange(G))
    assert index.size - real.size == 64 * sum((k * R) % 2 for k in BP.NET_K)
    # the tensor table
    T = 48 + 16 * (f + 2 * b) + 36 + 2 * (cfg["head_num_layers"] + 2)
    assert len(shapes) == len(end) == T and end[-1] == G and (np.diff(end) > 0).all() and (T == 288) == (name == "top")
    assert T <= 288, "bc_opt_rule::MAX_TENSORS"
    # the C side counts the same tensors: one off is refused by name, the right count passes on to the last check
    L = _capi.lib()
    for t, word in ((T - 1, b"num_tensors"), (T + 1, b"num_tensors"), (T, b"aligned")):
        o = _structs(A, R, cfg, num_tensors=t)[2]
        assert L.gd_bc_adamw(C.byref(o), OK + 2, None) == _capi.GD_ERR_INVALID and word in L.gd_last_error(), (t, L.gd_last_error())
    # the flat layout round-trips a state dict, through the blob and back
    sd = GR.state_dict(R, cfg)
    flat = np.concatenate([sd[k].numpy().reshape(-1) for k in shapes])
    assert flat.size == G
    back = {k: a.reshape(shapes[k]) for k, a in zip(shapes, np.split(flat, end[:-1]))}
    assert all(np.array_equal(back[k], sd[k].numpy()) for k in shapes)
    blob = np.concatenate([flat, [np.float32(0)]])[index]
    assert np.array_equal(blob[BO.blob_of(*lay)], flat)
    assert BT.grad_scratch_floats(A, 2, cfg["num_layer"], index.size) > index.size


# ---- the yardsticks

@pytest.mark.parametrize("name", NAMES)
def test_forward_yardsticks_are_float32_errors(name):
    c, ref, E = _yardstick(name)
    for k, v in E.items():
        print("BC EDGE E %s %s %.3e" % (name, k, v))
        if k == "weights" and cfg_of(name)["n_components"] == 1:
            assert v == 0  # one component: its weight is exactly 1 in either precision
            continue
        size = max(1.0, float(np.abs(ref[k]).max()))
        assert np.isfinite(v) and 0 < v < 1e-5 * size, (name, k, v, size)  # an error of float32: not zero, no loose bound
    B, A, R, cfg = BC.EDGE[name]
    assert ref["means"].shape == (B, cfg["n_components"], 3) and np.isfinite(ref["nll"]).all()
    raw = ref["raw"][:, 3 * cfg["n_components"]:6 * cfg["n_components"]]
    if name == "deep_fusion":  # a floor above 0 cuts through the raw covariances: some below it, some above
        assert (raw < cfg["clip_value"]).any() and (raw > cfg["clip_value"]).any()
        assert (ref["log_covariances"].reshape(B, -1)[raw < cfg["clip_value"]] == cfg["clip_value"]).all()
    if name == "sweep":        # only a raw value in (-20, -10) tells the clip10 floor from -20
        assert ((raw > -20) & (raw < -10)).any()


def test_backward_yardstick_at_the_largest_model():
    B, A, R, cfg = BC.EDGE["top"]
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R, cfg)
    w = GR.grad_weights(B, "mean")
    g64, _, margins = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg)
    g32, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, dtype=torch.float32)
    assert min(margins.values()) > GR.MARGIN and len(g64) == 288
    E = GR.yardstick(g32, g64)
    rel = [E[k] / np.abs(g64[k]).max() for k in E if not k.endswith("k_proj.bias")]
    assert 2.0 ** -23 <= min(rel) and max(rel) < 1e-2
    assert np.abs(g64["head.head.weight"][64:]).max() > 0, "the head's outputs past lane 63 carry gradient"


# ---- wrong rules that are right at CFG

@pytest.mark.parametrize("wrong,names", [("head_one_trip", ("c10", "top")), ("rg_at_ro", ("deep_branch",)),
                                         ("floor_m20", ("sweep", "deep_fusion"))])
def test_a_rule_that_is_right_at_cfg_is_caught_at_its_edge_case(wrong, names):
    for name in names:
        c, ref, E = _yardstick(name)
        ratios = _forward_ratios(c, ref, E, BC.EDGE[name][1], wrong)
        print("BC EDGE WRONG %s %s %s" % (wrong, name, {k: "%.3g" % v for k, v in ratios.items()}))
        assert max(ratios.values()) > 4 * K, (wrong, name, ratios)
    for B, A, R in BC.SHAPES:
        c, ref, E = _yardstick((B, A, R, BC.CFG))
        ratios = _forward_ratios(c, ref, E, A, wrong)
        assert max(ratios.values()) == 0.0, (wrong, (B, A, R), ratios)  # the same rule there: not one bit moves


def test_rg_at_ro_cannot_show_with_one_branch_layer():
    """deep_fusion has ONE branch layer, index 0 < min(fusion, branch): the rule leaves it alone.  What deep_fusion adds for the
    layer offsets is fusion > branch, which the backward's and the taps' comparisons run at; a layer index at or above the
    other block's depth exists only with branch > fusion (deep_branch)."""
    c, ref, E = _yardstick("deep_fusion")
    assert max(_forward_ratios(c, ref, E, 64, "rg_at_ro").values()) == 0.0


def test_c9_ends_one_lane_short_of_the_second_trip():
    c, ref, E = _yardstick("c9")
    assert max(_forward_ratios(c, ref, E, 64, "head_one_trip").values()) == 0.0


@pytest.mark.parametrize("wrong,name,tensor", [("head_one_trip", "c10", "head.head.weight"), ("rg_at_ro", "deep_branch", "rg_attn.1.1.module.3.weight"),
                                               ("floor_m20", "deep_fusion", "head.head.bias")])
def test_a_backward_rule_that_is_right_at_cfg_is_caught_at_its_edge_case(wrong, name, tensor):
    B, A, R, cfg = BC.EDGE[name]
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R, cfg)
    w = GR.grad_weights(B, "mean")
    g64, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg)
    g32, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, dtype=torch.float32)
    bad, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, wrong=wrong)
    E = GR.yardstick(g32, g64)
    assert float(np.abs(bad[tensor] - g64[tensor]).max()) / E[tensor] > 4 * K
    # and at CFG it is the right rule
    sd, obs, pm, rm, expert, _ = GR.case_inputs(3, 64, 1)
    w = GR.grad_weights(3, "mean")
    g64, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, 64)
    bad, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, 64, wrong=wrong)
    assert all(np.array_equal(bad[k], g64[k]) for k in g64)


def test_tensors_past_the_first_trip_left_out_of_the_norms_are_caught():
    """Against the host program of csrc/bc_opt_rule.hpp at `top`'s 288 tensors, with the gradients the GPU test uploads: the
    rule that sees tensors 0 .. 255 only gives another clip norm, another largest tensor and other parameters; at CFG's 204
    tensors it is the right rule."""
    R, cfg = BC.EDGE["top"][2], BC.EDGE["top"][3]
    _, end, G = UR.layout(R, cfg)
    grads, zt, largest = UR.top_gradients(end)
    assert len(end) == 288 and zt >= 256 and largest >= 256
    for g in grads:
        n64 = UR.tensor_norms64(g, end)
        top = np.sort(n64)[-2:]
        assert int(np.argmax(n64)) == largest and top[1] - top[0] > 1e-3 * top[1]  # no float32 rounding changes the largest
    p0 = np.random.default_rng(5).normal(0.0, 0.1, G).astype(np.float32)
    z = np.zeros(G, np.float32)
    host = UR.run_adamw_host(p0, z, z, grads, end, **UR.ADAMW)
    r64 = UR.adamw_reference(p0, grads, end, torch.float64, **UR.ADAMW)
    r32 = UR.adamw_reference(p0, grads, end, torch.float32, **UR.ADAMW)
    bad = UR.adamw_reference(p0, grads, end, torch.float64, **UR.ADAMW, wrong="first_256")
    assert host[0]["tensor_norms"][zt] == 0 and (host[0]["tensor_norms"][256:] > 0).sum() == 288 - 256 - 1
    for s in range(3):
        for k in ("params", "exp_avg", "exp_avg_sq"):
            err, E = UR.error_floor(host[s][k], r64[s][k], r32[s][k])
            assert err <= C_ADAMW * E, (s, k, err, E)
        assert abs(float(host[s]["total"]) - r64[s]["total"]) <= 2.0 ** -22 * r64[s]["total"]
        assert host[s]["max_grad_tensor"] == largest == r64[s]["max_grad_tensor"]
        assert abs(float(host[s]["max_grad_norm"]) - r64[s]["max_grad_norm"]) <= 2.0 ** -21 * r64[s]["max_grad_norm"]
        # the wrong rule
        assert bad[s]["max_grad_tensor"] < 256
        assert abs(float(host[s]["total"]) - bad[s]["total"]) > 1e3 * 2.0 ** -22 * r64[s]["total"]
        assert abs(float(host[s]["max_grad_norm"]) - bad[s]["max_grad_norm"]) > 1e3 * 2.0 ** -21 * r64[s]["max_grad_norm"]
    _, E = UR.error_floor(host[0]["exp_avg"], r64[0]["exp_avg"], r32[0]["exp_avg"])
    err = float(np.abs(host[0]["exp_avg"] - bad[0]["exp_avg"]).max())
    print("BC EDGE WRONG first_256 exp_avg err %.3e E %.3e" % (err, E))
    assert err > 4 * K * C_ADAMW * E, "the first step's clip coefficient is another"
    _, end, G = UR.layout(1)
    p0, grads = p0[:G], UR.gradients(end)
    a, b = (UR.adamw_reference(p0, grads, end, torch.float64, **UR.ADAMW, wrong=w) for w in (None, "first_256"))
    for s in range(3):
        assert a[s]["max_grad_tensor"] == b[s]["max_grad_tensor"] and abs(a[s]["total"] - b[s]["total"]) <= 1e-12 * a[s]["total"]
        assert np.abs(a[s]["params"] - b[s]["params"]).max() <= 1e-12


# ---- the evaluation's sums

def eval_batches(n):
    """Two batches of n rows for one accumulator, seeded as bc_update_reference.row_inputs: experts on both sides of the three
    thresholds (2, 0.035, 0.023) in either."""
    out = [UR.row_inputs(n, seed=s) for s in (3, 4)]
    for _, _, ex in out:
        big = np.abs(ex) > np.array([2.0, 0.035, 0.023], dtype=np.float32)
        assert n < 8 or (big.any(0).all() and (~big).any(0).all())
    return out


def eval_bound(n, want):
    return (n + 8) * 2.0 ** -24 * np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("n", [63, 64, 65, 130, 513])
def test_an_evaluation_of_the_first_64_rows_is_caught_from_65(n):
    """The float32 wave's own order (lane i sums rows i, i + 64, ..; then a tree) stays inside the GPU test's bound; the rule
    that stops after one trip is the same rule up to n = 64 and leaves the bound from n = 65."""
    batches = eval_batches(n)
    want = REF.evaluate_sums(batches)
    bad = REF.evaluate_sums(batches, wrong="eval_one_trip")
    bound = eval_bound(n, want)[:10]
    if n <= 64:
        assert np.array_equal(bad, want)
    else:
        assert (np.abs(bad - want)[:4] > 4 * K * bound[:4]).all()  # the four means lose a row each, whatever the row holds
    acc = np.zeros(11, np.float32)
    thr = np.array([2.0, 0.035, 0.023], dtype=np.float32)
    for nll, pred, ex in batches:
        d = np.abs(pred - ex)
        big = np.abs(ex) > thr
        cols = np.concatenate([nll[:, None], d, np.where(big, d, np.float32(0)), big.astype(np.float32)], 1)
        lanes = np.zeros((64, 10), np.float32)
        for r in range(n):
            lanes[r % 64] += cols[r]
        while len(lanes) > 1:
            lanes = lanes[:len(lanes) // 2] + lanes[len(lanes) // 2:]
        acc[:4] += lanes[0, :4] / np.float32(n)
        acc[4:10] += lanes[0, 4:]
        acc[10] += 1
    assert (np.abs(acc.astype(np.float64) - want)[:10] <= bound).all(), (np.abs(acc - want)[:10] / bound)
    assert np.array_equal(acc[7:], want[7:])
