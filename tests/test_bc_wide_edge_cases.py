"""The configurations of bc_wide_cases.EDGE_CASES without a GPU, as tests/test_bc_edge_cases.py has bc_cases.EDGE_CASES at 64: the
table itself, the host-side layouts at width 128 at every one of them (the blob's index and its inverse, the flat gradient and
the backward's scratch, the optimiser's tensor table, the C side's tensor count), the float32 yardsticks and the head margins
there, and the wrong rules -- each the RIGHT rule at the four cases of bc_wide_cases.CASES, or at 64, which is why the wide suite
could not see it -- shown to leave the GPU tests' bounds K E and K E_p on the edge case named for it and to change no bit where
they are the right rule.

Measured here (error of the wrong rule / yardstick, the worst output or tensor; the GPU tests accept at most K = 32):
    forward    head_one_trip wide_c10 2.2e6 (weights; 1.4e6 on nll), wide_top 7.0e5 (log_covariances), wide_c9 no bit;
               rg_at_ro wide_deep_branch 4.7e5 (context), wide_deep_fusion no bit; floor_m20 wide_clip10 3.7e5 (log_covariances
               alone), wide_deep_fusion 8.7e6 (nll); kin_three_tiles wide_top 2.6e5 (weights), top at 64 5.6e5 (context);
               scale16 wide_top 1.5e5 (nll), ln64 wide_top 3.7e5 (weights), ctx192 wide_top 4.9e5 (log_covariances; the
               context does not move), heads_of_16 wide_deep_branch 6.0e5 (context)
    backward   head_one_trip wide_c10 4.2e5, wide_top 2.4e5, wide_c9 no bit; rg_at_ro wide_deep_branch 1.7e6, wide_deep_fusion
               no bit; floor_m20 wide_deep_fusion 1.7e7, wide_clip10 no bit of any gradient; kin_three_tiles wide_top 2.2e5
               (1.5e5 on road_graph_net.0.weight), top at 64 1.8e5 on that tensor; quarter_scale wide_deep_fusion 3.1e5
    evaluate   eval_one_trip on wide_defaults' 130 rows: 2.0e3, 7.8e3, 2.5e3 and 1.2e3 times the bound on the four means"""
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
from . import bc_wide_cases as WC
from . import bc_wide_grad_reference as WGR
from . import bc_wide_update_reference as WUR

K = 32  # the bound of the GPU tests: error <= K E (forward), K E_p (backward)
NAMES = list(WC.EDGE_NAMES)
DIM = WC.DIM
KEYS = BC.COMPARED + ("nll",)


def _lay(R, cfg):
    return R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"]


def _forward_ratios(c, wrong):
    """What the GPU forward test measures, with the wrong rule in the kernel's place: error / E per compared output."""
    bad = REF.forward(c["sd"], c["obs"], c["pm"], c["rm"], c["A"], **c["cfg"], wrong=wrong)
    bad["nll"] = REF.nll(bad["means"], bad["log_covariances"], bad["weights"], c["expert"][:, 0])
    return {k: (float(np.abs(bad[k] - c["ref"][k]).max()) / c["E"][k] if c["E"][k] > 0 else
                float(np.abs(bad[k] - c["ref"][k]).max())) for k in KEYS}


def _backward_ratios(c, wrong):
    """The same for the backward: error / E_p per parameter tensor, and the wrong rule's gradients."""
    bad, _, _ = WGR.gradients(c["sd"], c["obs"], c["pm"], c["rm"], c["expert"], c["w"], c["A"], c["cfg"], wrong=wrong)
    return {k: float(np.abs(bad[k] - c["g64"][k]).max()) / c["E"][k] for k in bad if c["E"][k] > 0}, bad


def _worst(ratios):
    k = max(ratios, key=ratios.get)
    return "%.3g at %s" % (ratios[k], k)


# ---- the table itself

def test_the_table_reaches_what_it_is_named_for():
    e = WC.EDGE
    assert NAMES == ["wide_top", "wide_clip10", "wide_c9", "wide_c10", "wide_deep_branch", "wide_deep_fusion", "wide_defaults"]
    for name, narrow, seed in WC.EDGE_CASES:
        assert e[name] is BC.EDGE[narrow] and WC.lookup(name) is e[name] and WC.SEEDS[name] == seed  # taken, not copied
    assert all(WC.SEEDS[n] == 1 for n in WC.CASES) and all(WC.lookup(n) is WC.CASES[n] for n in WC.CASES)
    tensors = {n: len(WC.shapes(e[n][2], e[n][3])) for n in NAMES}
    assert tensors["wide_top"] == 288 and tensors["wide_clip10"] == 252 == len(WC.shapes(*WC.CASES["wide_sweep"][2:]))
    assert [7 * e[n][3]["n_components"] for n in ("wide_c9", "wide_c10", "wide_top")] == [63, 70, 112]
    assert 13 * e["wide_top"][2] == 104 and e["wide_top"][3]["head_num_layers"] == 4 and e["wide_top"][3]["num_layer"] == (4, 4)
    assert e["wide_deep_fusion"][3]["head_num_layers"] == 3
    f, b = e["wide_deep_branch"][3]["num_layer"]
    assert (f, b) == (1, 4) and b > f and e["wide_deep_branch"][1] == 128
    assert (6 * e["wide_deep_branch"][2], 13 * e["wide_deep_branch"][2]) == (12, 26)  # even first-layer kin
    f, b = e["wide_deep_fusion"][3]["num_layer"]
    assert (f, b) == (4, 1) and f > b and 0 < e["wide_deep_fusion"][3]["clip_value"] < REF.COV_MAX == 3.58352
    assert e["wide_clip10"][3]["clip_value"] == -10.0 and dict(e["wide_clip10"][3], clip_value=-20.0) == WC.CASES["wide_sweep"][3]
    assert e["wide_defaults"][0] == BP.DEFAULT_CHUNK + 2 == 130
    # what the four cases of bc_wide_cases.CASES stop at
    assert max(7 * c[3]["n_components"] for c in WC.CASES.values()) == 42 and max(c[3]["head_num_layers"] for c in WC.CASES.values()) == 2
    assert max(c[2] for c in WC.CASES.values()) == 5 and {c[3]["clip_value"] for c in WC.CASES.values()} == {-20.0}
    assert max(c[0] for c in WC.CASES.values()) == 5 and max(tensors.values()) > max(len(WC.shapes(c[2], c[3])) for c in WC.CASES.values())
    for name in NAMES:
        B, A, R, cfg = e[name]
        sd = BC.state_dict(R, cfg, network_dim=DIM)
        got = BP.check_bc_args(sd, max_agents=A, num_stack=R, network_dim=DIM, network_dims=(64, DIM), **cfg)
        assert list(got) == list(sd) == list(WC.shapes(R, cfg))  # the host checks accept every one


# ---- the host-side layouts at width 128

@pytest.mark.parametrize("name", NAMES)
def test_layouts_at_every_edge_configuration_at_128(name):
    _, A, R, cfg = WC.EDGE[name]
    lay = _lay(R, cfg)
    f, b = cfg["num_layer"]
    shapes = WC.shapes(R, cfg)
    index, G, end = BP.pack_index(*lay, network_dim=DIM), BT.grad_floats(*lay, network_dim=DIM), BO.tensor_end(shapes)
    assert G == sum(int(np.prod(s)) for s in shapes.values())
    if name == "wide_top":
        assert G == 1620912
    if name == "wide_clip10":
        assert G == WUR.SWEEP_G
    # the blob's index: every parameter exactly once, nothing outside flat + its one zero; 128 padding places per odd kin
    real = index != G
    assert index.min() >= 0 and index.max() <= G and np.array_equal(np.sort(index[real]), np.arange(G))
    assert index.size - int(real.sum()) == DIM * sum((k * R) % 2 for k in BP.NET_K)
    # ... and blob_of is its inverse onto the places that are no padding
    inv = BO.blob_of(*lay, network_dim=DIM)
    assert inv.shape == (G,) and inv.dtype == np.int32
    assert np.array_equal(index[inv], np.arange(G)) and np.array_equal(np.sort(inv), np.flatnonzero(real))
    assert np.array_equal(inv[index[real]], np.flatnonzero(real))
    # the tensor table
    T = 48 + 16 * (f + 2 * b) + 36 + 2 * (cfg["head_num_layers"] + 2)
    assert len(shapes) == len(end) == T and end[-1] == G and (np.diff(end) > 0).all() and (T == 288) == (name == "wide_top")
    assert T <= 288, "bc_opt_rule::MAX_TENSORS"
    # the C side counts the same tensors at 128: one off is refused by name, the right count passes on to the last check
    L = _capi.lib()
    for t, word in ((T - 1, b"num_tensors"), (T + 1, b"num_tensors"), (T, b"aligned")):
        o = WUR.structs(DIM, name, num_tensors=t)[2]
        assert o.grad_floats == G and o.blob_floats == index.size
        assert L.gd_bc_adamw_dim(C.byref(o), DIM, WUR.OK + 2, None) == _capi.GD_ERR_INVALID and word in L.gd_last_error(), (t, L.gd_last_error())
    # the flat layout round-trips a state dict, through the blob and back
    sd = BC.state_dict(R, cfg, network_dim=DIM)
    flat = np.concatenate([sd[k].numpy().reshape(-1) for k in shapes])
    assert flat.size == G
    back = {k: a.reshape(shapes[k]) for k, a in zip(shapes, np.split(flat, end[:-1]))}
    assert all(np.array_equal(back[k], sd[k].numpy()) for k in shapes)
    blob = np.concatenate([flat, [np.float32(0)]])[index]
    assert np.array_equal(blob[inv], flat) and (blob[~real] == 0).all()
    # the backward's scratch: the transposed weights, then per row and token f + b + 5 buffers of 128 and 16 statistics
    for chunk in (2, BP.DEFAULT_CHUNK):
        want = (index.size + 63) // 64 * 64 + chunk * (A + 200) * (DIM * (f + b + 5) + 16)
        assert BT.grad_scratch_floats(A, chunk, cfg["num_layer"], index.size, network_dim=DIM) == want
    assert BP.scratch_floats(A, BP.DEFAULT_CHUNK, DIM) == BP.DEFAULT_CHUNK * 3 * (A + 200) * DIM


# ---- the yardsticks and the margins

@pytest.mark.parametrize("name", NAMES)
def test_forward_yardsticks_are_float32_errors_at_128(name):
    c = WC.case(name)
    B, cfg, ref = c["B"], c["cfg"], c["ref"]
    for k, v in c["E"].items():
        print("BC WIDE EDGE E %s %s %.3e" % (name, k, v))
        if k == "weights" and cfg["n_components"] == 1:
            assert v == 0  # one component: its weight is exactly 1 in either precision
            continue
        size = max(1.0, float(np.abs(ref[k]).max()))
        assert np.isfinite(v) and 0 < v < 1e-5 * size, (name, k, v, size)  # an error of float32: not zero, no loose bound
    assert ref["means"].shape == (B, cfg["n_components"], 3) and ref["context"].shape == (B, 3 * DIM) and np.isfinite(ref["nll"]).all()
    raw = ref["raw"][:, 3 * cfg["n_components"]:6 * cfg["n_components"]]
    assert (raw < cfg["clip_value"] - 1e-3).any() and (raw > REF.COV_MAX + 1e-3).any()  # the exact-clamp check has rows on both sides
    if name == "wide_deep_fusion":  # a floor above 0 cuts through the raw covariances: some below it, some above
        assert (raw < cfg["clip_value"]).any() and ((raw > cfg["clip_value"]) & (raw < REF.COV_MAX)).any()
    if name == "wide_clip10":       # only a raw value in (-20, -10) tells the clip10 floor from -20
        assert ((raw > -20) & (raw < -10)).any()


@pytest.mark.parametrize("name", NAMES)
def test_the_margins_hold_and_the_backward_shares_the_forwards_inputs(name):
    """Both head margins of the float64 restatement exceed bc_grad_reference.MARGIN with the table's seed, so no clamp and no
    ReLU of the head can flip between float32 and float64; the backward's case is the forward's, row for row."""
    c, f = WGR.case(name, "mean"), WC.case(name)
    print("BC WIDE EDGE MARGINS %s clamp %.3g relu %.3g" % (name, c["margins"]["clamp"], c["margins"]["relu"]))
    assert c["margins"]["clamp"] > GR.MARGIN and c["margins"]["relu"] > GR.MARGIN, c["margins"]
    assert np.array_equal(c["obs"], f["obs"]) and np.array_equal(c["pm"], f["pm"]) and np.array_equal(c["rm"], f["rm"])
    assert np.array_equal(c["expert"], f["expert"][:, 0]) and len(c["obs"]) == WC.EDGE[name][0]
    assert np.abs(c["nll"] - f["ref"]["nll"]).max() <= 1e-12 * (1 + np.abs(c["nll"]).max())
    assert list(c["g64"]) == list(WC.shapes(c["R"], c["cfg"]))
    rel = [c["E"][k] / np.abs(c["g64"][k]).max() for k in c["E"] if not k.endswith("k_proj.bias") and np.abs(c["g64"][k]).max() > 0]
    assert 2.0 ** -23 <= min(rel) and max(rel) < 1e-2  # E_p is an error of float32
    if name == "wide_defaults":
        with torch.no_grad():  # the default seed would not do
            net = WGR.Net(c["sd"], c["A"], c["cfg"])
            obs, pm, rm, expert, _, _, _ = BC.inputs(*WC.EDGE[name][:3], seed=1)
            net.nll(obs, pm, rm, expert[:, 0])
        assert min(net.margins.values()) < GR.MARGIN
    if name in ("wide_c10", "wide_top"):
        C_ = c["cfg"]["n_components"]  # (rows 3 C .. 6 C of a covariance outside the clamp are exact zeros; the weights' rows never)
        live = np.abs(c["g64"]["head.head.weight"][64:]).max(1) > 0
        assert live[max(6 * C_ - 64, 0):].all() and live.sum() >= 6 and (c["g64"]["head.head.bias"][64:][live] != 0).all(), \
            "the head's outputs past lane 63 carry gradient"


# ---- wrong rules that are right at the four wide cases

FORWARD_RULES = [("head_one_trip", ("wide_c10", "wide_top")), ("rg_at_ro", ("wide_deep_branch",)),
                 ("floor_m20", ("wide_clip10", "wide_deep_fusion")), ("kin_three_tiles", ("wide_top",))]


@pytest.mark.parametrize("wrong,names", FORWARD_RULES)
def test_a_forward_rule_that_is_right_at_the_wide_cases_is_caught_at_its_edge_case(wrong, names):
    for name in names:
        ratios = _forward_ratios(WC.case(name), wrong)
        print("BC WIDE EDGE WRONG %s %s %s" % (wrong, name, {k: "%.3g" % v for k, v in ratios.items()}))
        assert max(ratios.values()) > 4 * K, (wrong, name, ratios)
    for name in WC.CASES:
        ratios = _forward_ratios(WC.case(name), wrong)
        if (wrong, name) == ("rg_at_ro", "wide_a128"):  # (1, 2): the one layer of the four cases the rule is wrong at
            assert max(ratios.values()) > 4 * K
            continue
        assert max(ratios.values()) == 0.0, (wrong, name, ratios)  # the same rule there: not one bit moves


def test_the_two_rules_that_show_on_one_output_show_there():
    """head_one_trip moves wide_c10's nll and floor_m20 wide_clip10's log_covariances by about 1e6 and 4e5 yardsticks."""
    assert _forward_ratios(WC.case("wide_c10"), "head_one_trip")["nll"] > 1e5
    assert _forward_ratios(WC.case("wide_clip10"), "floor_m20")["log_covariances"] > 1e5


def test_kin_three_tiles_is_caught_on_top_at_64():
    """The rule at the 64-wide `top` (R = 8: kin 104), and the right rule on every other case of bc_cases.EDGE_CASES (R <= 5)."""
    from .test_bc_edge_cases import _forward_ratios as narrow_ratios
    from .test_bc_edge_cases import _yardstick
    c, ref, E = _yardstick("top")
    ratios = narrow_ratios(c, ref, E, BC.EDGE["top"][1], "kin_three_tiles")
    print("BC EDGE WRONG kin_three_tiles top %s" % {k: "%.3g" % v for k, v in ratios.items()})
    assert max(ratios.values()) > 4 * K
    for name in ("sweep", "deep_branch"):
        c, ref, E = _yardstick(name)
        assert max(narrow_ratios(c, ref, E, BC.EDGE[name][1], "kin_three_tiles").values()) == 0.0


def test_c9_ends_one_lane_short_of_the_second_trip_at_128():
    assert max(_forward_ratios(WC.case("wide_c9"), "head_one_trip").values()) == 0.0
    ratios, bad = _backward_ratios(WGR.case("wide_c9", "mean"), "head_one_trip")
    assert max(ratios.values()) == 0.0 and all(np.array_equal(bad[k], WGR.case("wide_c9", "mean")["g64"][k]) for k in bad)


def test_rg_at_ro_cannot_show_with_one_branch_layer_at_128():
    """wide_deep_fusion has ONE branch layer, index 0 < min(fusion, branch): the rule leaves it alone, forward and backward.
    What wide_deep_fusion adds for the layer offsets is fusion > branch, which the backward's comparison runs at; a layer index
    at or above the other block's depth exists only with branch > fusion (wide_deep_branch, where three such layers exist)."""
    assert max(_forward_ratios(WC.case("wide_deep_fusion"), "rg_at_ro").values()) == 0.0
    c = WGR.case("wide_deep_fusion", "mean")
    ratios, bad = _backward_ratios(c, "rg_at_ro")
    assert all(np.array_equal(bad[k], c["g64"][k]) for k in bad)


@pytest.mark.parametrize("wrong,name,output", [("scale16", "wide_top", "context"), ("ln64", "wide_top", "context"),
                                               ("ctx192", "wide_top", "means"), ("heads_of_16", "wide_deep_branch", "context")])
def test_the_mistakes_the_width_invites_are_caught_at_the_edge_cases(wrong, name, output):
    """The four rules of the 64-wide kernels kept at 128 (tests/test_bc_wide.py shows them on bc_wide_cases.CASES): caught on the
    edge cases too, and the right rule at 64 -- no bit moves on a 64-wide state dict."""
    c = WC.case(name)
    ratios = _forward_ratios(c, wrong)
    print("BC WIDE EDGE WRONG %s %s %s" % (wrong, name, {k: "%.3g" % v for k, v in ratios.items()}))
    assert ratios[output] > 4 * K
    B, A, R, cfg = BC.EDGE["c10"]
    sd = BC.state_dict(R, cfg)
    obs, pm, rm, _, _, _, _ = BC.inputs(B, A, R)
    a, b = REF.forward(sd, obs, pm, rm, A, **cfg), REF.forward(sd, obs, pm, rm, A, **cfg, wrong=wrong)
    assert all(np.array_equal(a[k], b[k]) for k in a)


BACKWARD_RULES = [("head_one_trip", "wide_c10", "head.head.weight"), ("head_one_trip", "wide_top", "head.head.weight"),
                  ("rg_at_ro", "wide_deep_branch", "rg_attn.1.1.module.3.weight"), ("floor_m20", "wide_deep_fusion", "head.head.bias"),
                  ("kin_three_tiles", "wide_top", "road_graph_net.0.weight"), ("quarter_scale", "wide_deep_fusion", "fusion_attn.3.0.module.attention.q_proj.weight")]


@pytest.mark.parametrize("wrong,name,tensor", BACKWARD_RULES)
def test_a_backward_rule_that_is_right_at_the_wide_cases_is_caught_at_its_edge_case(wrong, name, tensor):
    c = WGR.case(name, "mean")
    ratios, bad = _backward_ratios(c, wrong)
    print("BC WIDE EDGE WRONG backward %s %s %s worst %s" % (wrong, name, "%.3g at %s" % (ratios[tensor], tensor), _worst(ratios)))
    assert ratios[tensor] > 4 * K
    if wrong == "kin_three_tiles":  # the fourth tile's columns get nothing
        assert (bad[tensor][:, 96:] == 0).all() and (c["g64"][tensor][:, 96:] != 0).any()
    if wrong == "head_one_trip":    # the second trip's rows get nothing
        assert (bad[tensor][64:] == 0).all() and (c["g64"][tensor][64:] != 0).any()
    if wrong == "quarter_scale":
        return  # wrong at every 128-wide case (tests/test_bc_wide_grad.py); the right rule at 64, below
    # and on the four wide cases it is the right rule: no bit of any gradient moves
    for other in ("wide_min", "wide_chunks"):  # (wide_sweep: the test below; rg_at_ro is wrong at wide_a128's second layer)
        o = WGR.case(other, "mean")
        bad, _, _ = WGR.gradients(o["sd"], o["obs"], o["pm"], o["rm"], o["expert"], o["w"], o["A"], o["cfg"], wrong=wrong)
        assert all(np.array_equal(bad[k], o["g64"][k]) for k in bad), (wrong, other)


def test_every_backward_rule_is_the_right_rule_at_the_sweeps_model():
    """wide_sweep, the largest of bc_wide_cases.CASES (42 head outputs, (4, 3), R = 5, clamp -20): none of the four rules moves
    a bit there."""
    o = WGR.case("wide_sweep", "mean")
    for wrong in ("head_one_trip", "rg_at_ro", "floor_m20", "kin_three_tiles"):
        bad, _, _ = WGR.gradients(o["sd"], o["obs"], o["pm"], o["rm"], o["expert"], o["w"], o["A"], o["cfg"], wrong=wrong)
        assert all(np.array_equal(bad[k], o["g64"][k]) for k in bad), wrong


def test_quarter_scale_is_the_right_rule_at_64():
    B, A, R, cfg = BC.EDGE["c10"]
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R, cfg)
    w = GR.grad_weights(B, "mean")
    a, _, _ = WGR.gradients(sd, obs, pm, rm, expert, w, A, cfg)
    b, _, _ = WGR.gradients(sd, obs, pm, rm, expert, w, A, cfg, wrong="quarter_scale")
    for k in a:
        assert np.abs(a[k] - b[k]).max() <= 1e-14 * max(np.abs(a[k]).max(), 1e-300), k  # 16^-1/2 is 0.25


def test_kin_three_tiles_backward_is_caught_on_top_at_64():
    B, A, R, cfg = BC.EDGE["top"]
    sd, obs, pm, rm, expert, _ = GR.case_inputs(B, A, R, cfg)
    w = GR.grad_weights(B, "mean")
    g64, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg)
    g32, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, dtype=torch.float32)
    bad, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, A, cfg, wrong="kin_three_tiles")
    E, t = GR.yardstick(g32, g64), "road_graph_net.0.weight"
    print("BC EDGE WRONG backward kin_three_tiles top %.3g" % (float(np.abs(bad[t] - g64[t]).max()) / E[t]))
    assert float(np.abs(bad[t] - g64[t]).max()) / E[t] > 4 * K and (bad[t][:, 96:] == 0).all()
    sd, obs, pm, rm, expert, _ = GR.case_inputs(3, 64, 1)  # and at CFG it is the right rule
    w = GR.grad_weights(3, "mean")
    g64, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, 64)
    bad, _, _ = GR.gradients(sd, obs, pm, rm, expert, w, 64, wrong="kin_three_tiles")
    assert all(np.array_equal(bad[k], g64[k]) for k in g64)


def test_floor_m20_moves_no_gradient_at_clip10():
    """wide_clip10's forward tells the two floors apart (log_covariances, above); its gradients do not.  The raw covariances
    between -20 and -10 belong to components whose covariance, at exp(-10) or exp(-20), puts the expert's action so far out
    that the component's responsibility is exactly 0 in float64: every gradient through it is an exact zero under either
    floor, and the nll does not move.  The floor's gradient is held at wide_deep_fusion, whose 2.0 cuts through live
    components."""
    c = WGR.case("wide_clip10", "mean")
    bad, nll, _ = WGR.gradients(c["sd"], c["obs"], c["pm"], c["rm"], c["expert"], c["w"], c["A"], c["cfg"], wrong="floor_m20")
    assert all(np.array_equal(bad[k], c["g64"][k]) for k in bad) and np.array_equal(nll, c["nll"])


def test_an_evaluation_of_the_first_64_rows_is_caught_at_wide_defaults():
    """`evaluate` on wide_defaults' 130 rows, from the float64 restatement's own nll and deterministic actions: the rule that sums
    one trip of 64 lanes leaves the GPU test's bound, K E per row plus (B + 8) 2^-24 for the sum; on the rows of every case of
    bc_wide_cases.CASES (at most 5) it is the same rule."""
    c = WC.case("wide_defaults")
    B = c["B"]
    _, act = REF.deterministic_action(c["ref"]["means"], c["ref"]["weights"])
    batches = [(c["ref"]["nll"], act, c["expert"][:, 0])]
    want, bad = REF.evaluate_sums(batches), REF.evaluate_sums(batches, wrong="eval_one_trip")
    rows = np.array([c["E"]["nll"]] + [c["E"]["means"]] * 3)
    bound = K * rows + (B + 8) * 2.0 ** -24 * np.maximum(1.0, np.abs(want[:4]))
    print("BC WIDE EDGE WRONG eval_one_trip wide_defaults %s" % (np.abs(bad - want)[:4] / bound))
    assert (np.abs(bad - want)[:4] > 4 * bound).all()
    for name in WC.CASES:
        o = WC.case(name)
        _, act = REF.deterministic_action(o["ref"]["means"], o["ref"]["weights"])
        batches = [(o["ref"]["nll"], act, o["expert"][:, 0])]
        assert np.array_equal(REF.evaluate_sums(batches), REF.evaluate_sums(batches, wrong="eval_one_trip"))
