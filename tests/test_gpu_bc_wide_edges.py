"""GPU suite: the BC policy at network_dim = 128 on the edge configurations of bc_wide_cases.EDGE_CASES -- forward, row lists,
backward, update and evaluate -- through the checks the wide suite already has (the helpers of tests/test_gpu_bc_wide.py,
test_gpu_bc_wide_grad.py, test_gpu_bc_wide_update.py and test_gpu_bc_live_rows.py), under the same bounds: K = 32 E per output
for the forward, K = 32 E_p per parameter tensor for the backward, the yardsticks being the float32 CPU run of the same
restatement against float64, never the kernel.  A ratio above 16 would be a finding to explain, not a bound to raise.
tests/test_bc_wide_edge_cases.py shows, without a GPU, the wrong rules these cases exist to catch.

What each case reaches in the kernels at T = 4 (csrc/bc_policy.hip, csrc/bc_grad.hip): wide_top the second trip of the head's
64-lane loops over 112 outputs, hin / pre at head depth 4, road kin 104 (kpad 128), 288 tensors in the optimiser; wide_c9 /
wide_c10 63 and 70 head outputs; wide_deep_branch rg_attn's layers past ro_attn's, A 128, even kin; wide_deep_fusion fusion >
branch, head depth 3, a clamp floor of 2.0; wide_clip10 the sweep's model at its own clamp; wide_defaults 130 rows under the
default chunk_rows = partials = 128: a full chunk of 128 rows and a short second chunk of 2 adding into the same 128 slices, and
the tile kernels' `id += gridDim.x` loops.  k_bcg_head_block is launched once per chunk on `partials` workgroups, so at the
defaults no workgroup takes a second row of its loop `b += gridDim.x` (a barrier at its head); `test_a_second_row_per_workgroup`
runs wide_top, wide_c10 and wide_deep_fusion with two partials for their three rows, where workgroup 0 takes rows 0 and 2.

Ratios measured once on an MI355X (printed per case and output or tensor with -s); the backward's is the worst tensor's:
    name (B, A, R)                context  means  log_covariances  weights  nll    ego_attn_score  backward (upstream)
    wide_top (3, 64, 8)           0.81     1.39   1.25             4.55     1.15   2.07            3.08 (seeded)
    wide_clip10 (3, 64, 5)        1.30     1.55   0.98             4.29     0.49   1.59            2.85 (mean)
    wide_c9 (3, 64, 1)            1.17     1.53   1.59             0.73     2.23   3.11            5.66 (seeded)
    wide_c10 (3, 64, 1)           1.17     1.57   1.26             0.48     1.59   3.11            6.07 (mean)
    wide_deep_branch (2, 128, 2)  1.02     1.52   0.89             0.93     0.73   0.70            5.75 (seeded)
    wide_deep_fusion (3, 64, 2)   1.38     1.24   0.61             1.09     0.43   2.56            2.68 (mean)
    wide_defaults (130, 64, 1)    1.23     1.04   1.06             0 / 0    0.90   0.91            2.30 (mean)
(`wide_defaults` has one component: its weight is exactly 1 on both sides.)  The largest of the forward, 4.55 and 4.29, are the
weights of three rows at E = 3.1e-7 and 4.3e-7, a few float32 ulps of a weight near 1, as wide_sweep's 4.29 is.  The backward's
worst tensors are k_proj biases (zero in exact arithmetic: rounding residue on both sides) at wide_top, wide_clip10,
wide_deep_branch and wide_deep_fusion, ego_ro_attn's k_proj weight at wide_c9 and its MLP's first weight at wide_c10.  One update at
wide_top: at most 0.11 of the step's bound per tensor, the four statistics within 0.012 of theirs; `evaluate` on wide_defaults'
130 + 65 rows within 0.002 of its bound.  With two partials (a second row in workgroup 0): wide_top 3.17, wide_c10
6.07, wide_deep_fusion 2.67."""
import numpy as np
import pytest
import torch

from gpudrive_lab_amd import bc_policy as BP
from tests import bc_grad_reference as GR
from tests import bc_reference as REF
from tests import bc_wide_cases as WC
from tests import bc_wide_grad_reference as WGR
from tests.test_gpu_bc_grad import K, _ratios
from tests.test_gpu_bc_live_rows import F_CANARY, I_CANARY, OUTPUTS, _Guarded, _row_lists_at_an_edge_configuration
from tests.test_gpu_bc_policy import EPS, _dev, _host
from tests.test_gpu_bc_wide import K as K_FORWARD
from tests.test_gpu_bc_wide import _forward_checks, _policy
from tests.test_gpu_bc_wide_grad import _device, _same_bits
from tests.test_gpu_bc_wide_update import _bits, _one_update_against_the_float64_pipeline, _train, _trainer, _update_against_its_parts

pytestmark = pytest.mark.gpu

NAMES = list(WC.EDGE_NAMES)


# ---- forward

@pytest.mark.parametrize("name", NAMES)
def test_forward_at_the_wide_edge_configurations(name):
    """test_gpu_bc_wide.test_forward_against_the_float64_restatement's body: context, means, clamped raw covariances, weights,
    nll and ego_attn_score within K E of float64; the rule on the kernel's own mixture for the deterministic action and both
    draws; raw covariances outside the clamp clamped exactly to the case's own clip_value; guard words on out=, two calls and
    uint8 masks bit for bit."""
    c, got, _ = _forward_checks(name)
    B, cfg = c["B"], c["cfg"]
    C_, clip = cfg["n_components"], cfg["clip_value"]
    assert got["means"].shape == (B, 1, C_, 3) and got["weights"].shape == (B, 1, C_)
    raw = c["ref"]["raw"][:, 3 * C_:6 * C_]
    lc = got["log_covariances"][:, 0].reshape(B, -1)
    inside = (raw > clip + 1e-3) & (raw < REF.COV_MAX - 1e-3)
    assert inside.any() and (lc[inside] > np.float32(clip)).all() and (lc[inside] < np.float32(3.58352)).all()
    if name == "wide_deep_fusion":  # a floor above 0 cuts through the raw covariances: more below it than the pushed one
        assert (raw < clip - 1e-3).sum() > B
    if name == "wide_clip10":       # a raw value between -20 and -10 is at -10 exactly, not passed through
        between = (raw > -20 + 1e-3) & (raw < -10 - 1e-3)
        assert between.any() and (lc[between] == np.float32(-10.0)).all()


# ---- row lists

@pytest.mark.parametrize("name", ["wide_top", "wide_c10"])
def test_forward_on_a_row_list_at_the_wide_edge_configurations(name):
    """test_gpu_bc_live_rows.test_forward_on_a_row_list_at_the_edge_configurations' lists (empty, last, first5, eight_permuted,
    all, no_middle_chunk; 11 rows in chunks of 4) on the wide policy: listed rows have the full forward's bits in every output,
    nothing else is written."""
    _row_lists_at_an_edge_configuration(name, *WC.EDGE[name][1:], network_dim=WC.DIM)


def test_a_list_of_most_rows_at_the_default_chunk():
    """wide_defaults: 97 of its 130 rows, permuted, at the default chunk_rows = 128 -- more listed rows than one wave has lanes,
    in one chunk."""
    from gpudrive_lab_amd.policy import LiveRows
    c = WC.case("wide_defaults")
    B = c["B"]
    bc = _policy(c)
    assert bc.chunk_rows == BP.DEFAULT_CHUNK == 128 < B
    obs, pm, rm, expert, u, z = _dev(c["obs"], c["pm"], c["rm"], c["expert"], c["u"], c["z"])
    kw = dict(deterministic=False, u=u, z=z, expert_actions=expert)
    full = bc.forward(obs, pm, rm, OUTPUTS, **kw)
    rows = np.random.default_rng(9).permutation(B)[:97]
    assert len(set(rows.tolist())) == 97 > 64 and (rows >= 128).any()
    made = {}

    def new(name, shape, dtype, fill, device):
        made[name] = g = _Guarded(shape, dtype, I_CANARY)
        return g.view

    lr = LiveRows(B, torch.device("cuda", torch.cuda.current_device()), new=new)
    lr.rows[:len(rows)] = torch.from_numpy(rows.astype(np.int32)).cuda()
    lr.count.fill_(len(rows))
    outs = {k: _Guarded(bc._OUT_SHAPES[k](bc, B), torch.int32 if k == "component" else torch.float32,
                        I_CANARY if k == "component" else F_CANARY) for k in OUTPUTS}
    bc.forward(obs, pm, rm, OUTPUTS, out={k: g.view for k, g in outs.items()}, rows=lr, **kw)
    listed = torch.zeros(B, dtype=torch.bool, device="cuda")
    listed[torch.from_numpy(rows).cuda()] = True
    for k, g in outs.items():
        g.check("wide_defaults list " + k)
        got, want = g.bits(), full[k].view(torch.int32)
        assert torch.equal(got[listed], want[listed]), k + " of a listed row differs from the full forward"
        assert bool((got[~listed] == g.canary).all()), k + " of a row that is not listed was written"
    for k, g in made.items():
        g.check("wide_defaults list " + k)
    assert int(lr.count) == 97 and lr.rows[:97].tolist() == rows.tolist()


# ---- backward

# the upstream gradients alternate; wide_top and wide_clip10 pass three partials (at the default 128 wide_top's partial slices
# alone would be 830 MB); the others take every default, chunk_rows = partials = 128
BACKWARD = dict(wide_top=("seeded", dict(partials=3)), wide_clip10=("mean", dict(partials=3)), wide_c9=("seeded", {}),
                wide_c10=("mean", {}), wide_deep_branch=("seeded", {}), wide_deep_fusion=("mean", {}), wide_defaults=("mean", {}))


@pytest.mark.parametrize("name", NAMES)
def test_every_parameter_gradient_at_the_wide_edge_configurations(name):
    """test_gpu_bc_wide_grad.test_every_parameter_gradient_against_float64's comparison on every row of every edge case, twice
    with equal bits; the rows of head.head the second 64-lane trip writes; exact zeros for the covariances outside the
    clamp."""
    kind, kw = BACKWARD[name]
    c = WGR.case(name, kind)
    assert min(c["margins"].values()) > GR.MARGIN, c["margins"]
    assert len(c["obs"]) == WC.EDGE[name][0]  # no row is left out
    got, nll = _device(c, **kw)
    assert list(got) == list(c["g64"])
    worst, at = _ratios("%s %s" % (name, kind), got, c)
    assert worst <= K, (worst, at)
    assert np.abs(nll - c["nll"]).max() <= 1e-3 * (1 + np.abs(c["nll"]).max())
    again, _ = _device(c, **kw)
    _same_bits(got, again)
    C_ = c["cfg"]["n_components"]
    w64, b64 = c["g64"]["head.head.weight"], c["g64"]["head.head.bias"]
    if name in ("wide_c10", "wide_top"):
        # rows 64 .. of head.head: what the second trip of the 64-lane loops writes.  The rows whose float64 gradient is above
        # the bound itself (a row left at zero would be outside it; wide_top has rows of 1e-144 too, zero in float32) are not
        # zero, and every row is within the bound
        Ew, Eb = c["E"]["head.head.weight"], c["E"]["head.head.bias"]
        live = np.flatnonzero((np.abs(w64[64:]).max(1) > K * Ew) & (np.abs(b64[64:]) > K * Eb)) + 64
        assert len(live) >= 6, live
        assert (np.abs(got["head.head.weight"][live]).max(1) > 0).all() and (got["head.head.bias"][live] != 0).all()
        for k, E in (("head.head.weight", Ew), ("head.head.bias", Eb)):
            assert np.abs(got[k][64:].astype(np.float64) - c["g64"][k][64:]).max() <= K * E, k
    if name == "wide_defaults":
        from gpudrive_lab_amd import TrainableBCPolicyDim
        assert TrainableBCPolicyDim.from_state_dict(c["sd"], max_agents=c["A"], num_stack=c["R"], device="cuda", network_dim=WC.DIM,
                                                    **c["cfg"]).partials == BP.DEFAULT_CHUNK == 128 < len(c["obs"])
    # the covariances every row has outside the clamp (the two bc_cases.state_dict pushes there among them) get exactly zero
    # rows of head.head, as float64 gives them -- at the floors -10 and 2.0 too; a covariance inside it in some row does not
    raw = WC.case(name)["ref"]["raw"][:, 3 * C_:6 * C_]
    clip = c["cfg"]["clip_value"]
    dead = np.flatnonzero(((raw < clip - 1e-3) | (raw > REF.COV_MAX + 1e-3)).all(0))
    assert 1 in dead and 2 <= len(dead) < 3 * C_, dead  # (1: the covariance pushed below the floor; wide_top's head, four
    # residual layers deep, brings the one pushed above 3.58352 back under it in one row, and has ten others outside)
    if name == "wide_deep_fusion":
        assert len(dead) > 2
    for r in dead + 3 * C_:
        assert (w64[r] == 0).all() and b64[r] == 0 and (got["head.head.weight"][r] == 0.0).all() and got["head.head.bias"][r] == 0.0, r
    live = np.flatnonzero(np.abs(w64[3 * C_:6 * C_]).max(1) > K * c["E"]["head.head.weight"]) + 3 * C_  # (above the bound itself)
    assert (len(live) or C_ == 1) and (np.abs(got["head.head.weight"][live]).max(1) > 0).all()  # (wide_defaults' one free covariance
    # has E_p of 1e3, under an nll of 1e9)


@pytest.mark.parametrize("name", ["wide_top", "wide_c10", "wide_deep_fusion"])
def test_a_second_row_per_workgroup(name):
    """k_bcg_head_block's row loop `for (b = blockIdx.x; b < rows; b += gridDim.x)` with fewer workgroups than rows in the chunk:
    two partials for three rows in one chunk, so workgroup 0 passes the barrier at the loop's head a second time and adds row 2
    into the slice that holds row 0 -- at head depth 4 and 112 outputs (wide_top), 70 outputs (wide_c10) and head depth 3
    (wide_deep_fusion).  Every gradient within K E_p of float64, twice with equal bits."""
    kind, _ = BACKWARD[name]
    c = WGR.case(name, kind)
    B = len(c["obs"])
    assert B == 3 and B <= BP.DEFAULT_CHUNK  # one chunk: rows 0 and 2 in workgroup 0, row 1 in workgroup 1
    got, nll = _device(c, partials=2)
    worst, at = _ratios("%s %s partials 2" % (name, kind), got, c)
    assert worst <= K, (worst, at)
    assert np.abs(nll - c["nll"]).max() <= 1e-3 * (1 + np.abs(c["nll"]).max())
    again, _ = _device(c, partials=2)
    _same_bits(got, again)


# ---- update and evaluate

def test_one_update_at_288_tensors_against_the_float64_pipeline():
    """test_gpu_bc_wide_update.test_one_update_against_the_float64_pipeline's body on wide_top: 288 tensors at the wide sizes, the
    optimiser's kernels past their first 256."""
    _one_update_against_the_float64_pipeline("wide_top", chunk_rows=2, partials=3)


def test_update_is_its_four_parts_bit_for_bit_on_wide_top():
    _update_against_its_parts("wide_top", chunk_rows=2, partials=3)


def test_defaults_through_the_wide_trainer_and_evaluate():
    """wide_defaults through `DeviceBCDim` with every default (chunk_rows = partials = 128, 130 rows): the update's gradient is
    `TrainableBCPolicyDim`'s with every default, bit for bit; `evaluate` on its 130 rows and a short batch of 65 -- more than one
    row per lane of gd_bc_eval_accumulate through the wide class -- against the reference's averaging on the kernel's own rows
    within float32 summation, and against the float64 restatement with the rows' own error on top."""
    name = "wide_defaults"
    c, f = WGR.case(name, "mean"), WC.case(name)
    B, A = len(c["obs"]), c["A"]
    obs, expert, pm, rm = _dev(c["obs"], c["expert"], c["pm"], c["rm"])
    bc = _trainer(c, batch_size=B)
    assert bc.policy.chunk_rows == BP.DEFAULT_CHUNK == 128 < B and bc._g.num_partials == 128 and bc.network_dim == 128
    # evaluate, on the weights before the step
    cuts = ((0, B), (0, 65))
    stats = bc.evaluate([(obs[lo:hi], expert[lo:hi], pm[lo:hi], rm[lo:hi], None) for lo, hi in cuts])
    assert tuple(stats) == BP.EVAL_NAMES and stats["tom_loss"] == 0.0
    got = np.array([stats[k] for k in BP.EVAL_NAMES])
    own = _host(bc.policy.forward(obs, pm, rm, ("nll", "actions"), deterministic=True, expert_actions=expert))
    mine = np.array(REF.evaluate([(own["nll"][lo:hi], own["actions"][lo:hi, 0], c["expert"][lo:hi]) for lo, hi in cuts]))
    assert np.isfinite(mine[:7]).all() and (np.abs(got - mine) <= (B + 8) * EPS * np.maximum(1.0, np.abs(mine))).all(), (got, mine)
    _, act = REF.deterministic_action(f["ref"]["means"], f["ref"]["weights"])
    want = np.array(REF.evaluate([(f["ref"]["nll"][lo:hi], act[lo:hi], c["expert"][lo:hi]) for lo, hi in cuts]))
    rows = np.array([f["E"]["nll"]] + [f["E"]["means"]] * 6 + [0.0])
    bound = K_FORWARD * rows + (B + 8) * EPS * np.maximum(1.0, np.abs(want))
    print("BC WIDE EDGE EVAL err/bound %s" % " ".join("%.3f" % v for v in (np.abs(got - want) / bound)[:7]))
    assert np.isfinite(want).all() and (np.abs(got - want) <= bound).all(), (got, want)
    one_trip = np.array(REF.evaluate([(f["ref"]["nll"][lo:hi], act[lo:hi], c["expert"][lo:hi]) for lo, hi in cuts], wrong="eval_one_trip"))
    assert (np.abs(one_trip - want)[:4] > 4 * bound[:4]).all()  # the rule that sums one row per lane is outside this bound
    # the update's gradient
    tbp = _train(c)
    assert tbp.chunk_rows == 128 and tbp.partials == 128
    bc.update(obs, expert, pm, rm)
    tbp(obs, pm, rm, expert).mean().backward()
    flat = torch.cat([p.grad.reshape(-1) for p in tbp.parameters()])
    assert [k for k, _ in tbp.named_parameters()] == list(bc._names)
    assert np.array_equal(_bits(bc.grad), _bits(flat)) and np.abs(bc.grad.cpu().numpy()).max() > 0
    worst, at = _ratios("wide_defaults update", dict(zip(c["g64"], (p.grad.cpu().numpy() for p in tbp.parameters()))), c)
    assert worst <= K, (worst, at)
    assert int(bc._step.item()) == 1 and np.isfinite(bc.flat.cpu().numpy()).all()
    assert bc.losses()["loss"] == pytest.approx(float(c["nll"].mean()), rel=1e-3)
