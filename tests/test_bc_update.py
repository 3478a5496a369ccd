"""CPU suite of the device BC update: the C interface and its argument checks, `blob_of`, the host-side refusals of `DeviceBC`,
and the rule's header (csrc/bc_opt_rule.hpp) run on the host against torch in float64.  The kernels themselves are tested in
test_gpu_bc_update.py.

The yardstick is the project's: E of a quantity is the error of the same lines in torch float32 on the CPU against float64,
floored at 2^-23 max |float64|; the host program must stay within C E.  C_ROWS and C_ADAMW are the next power of two at or
above twice the largest ratio measured over all cases below (DESIGN.md section 5 tabulates them):
  rows   largest ratio 0.35 (dyaw_loss, n = 3)                                            -> C_ROWS = 1
  adamw  largest ratio 1.00 (the parameters after the second and third step, weight_decay 0.01: the
         host program's error there IS float32 torch's)                                   -> C_ADAMW = 2"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from tests import bc_cases as BC
from tests import bc_grad_reference as GR
from tests import bc_update_reference as UR
from tests import ppo_update_reference as PR
from tests.conftest import ROOT

C_ROWS = 1
C_ADAMW = 2
# (R, cfg): both stack depths, whose first embedder layers have odd widths at R = 1 and R = 5 (6, 13, 30, 65 columns: the odd
# ones carry a padding column in the blob), the smallest head, the largest model
LAYOUTS = ((1, BC.CFG), (5, BC.CFG), (3, BC.CFG), (1, GR.MINIMAL), (5, dict(GR.MINIMAL, n_components=16)),
           (8, dict(num_layer=(4, 4), head_num_layers=4, n_components=16, clip_value=-20.0)))


def _layout_args(R, cfg):
    return R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"]


# ---- the C interface

def test_the_header_declares_the_entry_points_and_null_is_refused():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert "int gd_bc_train_rows(const gd_bc_opt *opt, int32_t n, " in header
    assert "int gd_bc_adamw(const gd_bc_opt *opt, const float *grad, void *stream);" in header
    assert "int gd_bc_update(const gd_bc_policy *p, const gd_bc_grad *g, const gd_bc_opt *opt, " in header
    assert "typedef struct gd_bc_opt {" in header and "csrc/bc_opt_rule.hpp" in header
    csrc = os.path.join(ROOT, "gpudrive_lab_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "bc_opt_rule.hpp")) and os.path.exists(os.path.join(csrc, "bc_opt.hip"))
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "bc_opt_rule.hpp" in make and "bc_opt.hip" in make and "-ffp-contract=off" in make
    names = {"gd_bc_train_rows", "gd_bc_adamw", "gd_bc_update"}
    assert names <= set(_capi.SYMBOLS)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_bc_train_rows.argtypes) == 7 and len(L.gd_bc_adamw.argtypes) == 3 and len(L.gd_bc_update.argtypes) == 9
    assert C.sizeof(_capi.GdBCOpt) == 4 * 4 + 2 * 8 + 2 * 8 + 8 * 4 + 18 * 8 and _capi.GdBCOpt.beta1.offset == 16
    assert _capi.GdBCOpt.tensor_end.offset == 80
    assert _capi.BC_STATS == UR.STATS + ("grad_norm", "max_grad_norm")
    assert L.gd_bc_train_rows(None, 1, *[None] * 5) == _capi.GD_ERR_INVALID and b"gd_bc_train_rows" in L.gd_last_error()
    assert L.gd_bc_adamw(None, None, None) == _capi.GD_ERR_INVALID and b"gd_bc_adamw" in L.gd_last_error()
    assert L.gd_bc_update(None, None, None, None, None, None, 1, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_bc_update" in L.gd_last_error()


OK = 0x1000


def _structs(A=64, R=1, cfg=BC.CFG, max_rows=8, chunk=2, **kw):
    from gpudrive_lab_amd import bc_train as BT
    lay = _layout_args(R, cfg)
    G, blob = BT.grad_floats(*lay), len(BP.pack_index(*lay))
    p, g, o = _capi.GdBCPolicy(), _capi.GdBCGrad(), _capi.GdBCOpt()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers = A, R, *cfg["num_layer"]
    p.head_layers, p.n_components, p.clip_value, p.chunk_rows = cfg["head_num_layers"], cfg["n_components"], -20.0, chunk
    p.blob, p.blob_floats, p.scratch, p.scratch_floats = OK, blob, OK, BP.scratch_floats(A, chunk)
    g.scratch, g.scratch_floats = OK, BT.grad_scratch_floats(A, chunk, cfg["num_layer"], blob)
    g.partials, g.grad_floats, g.num_partials = OK, G, 4
    o.max_grad_norm, o.eps, o.weight_decay, o.stats_scale, o.beta1, o.beta2 = 20.0, 1e-4, 0.01, 1.0, 0.9, 0.999
    o.grad_floats, o.blob_floats = G, blob
    o.num_stack, o.fusion_layers, o.branch_layers = R, *cfg["num_layer"]
    o.head_layers, o.n_components, o.max_rows = cfg["head_num_layers"], cfg["n_components"], max_rows
    o.num_tensors = len(BP.expected_shapes(*lay))
    for name, _ in _capi.GdBCOpt._fields_[16:]:
        setattr(o, name, OK)
    for k, v in kw.items():
        setattr(o, k, v)
    return p, g, o


def test_the_entry_points_check_their_arguments_without_a_device():
    """Nothing is launched: every call below stops at a check (the last one of each group at a pointer's alignment, which is
    checked after everything else)."""
    L = _capi.lib()

    def rows(o, n=3, args=(OK,) * 4):
        return L.gd_bc_train_rows(C.byref(o), n, *args, None), L.gd_last_error()

    for n in (0, -1, (1 << 20) + 1):
        rc, err = rows(_structs()[2], n)
        assert rc == _capi.GD_ERR_INVALID and b"n must be" in err, (n, err)
    for kw, msg in ((dict(stats=None), b"stats"), (dict(stats_sum=None), b"stats"), (dict(stats=OK + 2), b"aligned")):
        rc, err = rows(_structs(**kw)[2])
        assert rc == _capi.GD_ERR_INVALID and msg in err, (kw, err)
    for i in range(4):
        rc, err = rows(_structs()[2], args=[None if j == i else OK for j in range(4)])
        assert rc == _capi.GD_ERR_INVALID and b"null" in err
        rc, err = rows(_structs()[2], args=[OK + 2 if j == i else OK for j in range(4)])
        assert rc == _capi.GD_ERR_INVALID and b"aligned" in err

    def adamw(o, grad=OK):
        return L.gd_bc_adamw(C.byref(o), grad, None), L.gd_last_error()

    bad = [(dict(num_stack=0), b"num_stack"), (dict(num_stack=9), b"num_stack"), (dict(fusion_layers=5), b"fusion_layers"),
           (dict(branch_layers=0), b"branch_layers"), (dict(head_layers=5), b"head_layers"), (dict(n_components=17), b"n_components"),
           (dict(reserved=1), b"reserved"), (dict(grad_floats=5), b"grad_floats"), (dict(blob_floats=5), b"blob_floats"),
           (dict(num_tensors=203), b"num_tensors"), (dict(num_tensors=0), b"num_tensors"), (dict(beta1=1.0), b"betas"),
           (dict(beta2=-0.1), b"betas"), (dict(beta1=float("nan")), b"betas"), (dict(eps=0.0), b"eps"),
           (dict(max_grad_norm=0.0), b"max_grad_norm"), (dict(max_grad_norm=float("nan")), b"max_grad_norm"),
           (dict(weight_decay=-0.01), b"weight_decay"), (dict(weight_decay=float("inf")), b"weight_decay"),
           (dict(weight_decay=float("nan")), b"weight_decay"), (dict(beta_pow=OK + 4), b"aligned"), (dict(scal=OK + 4), b"aligned"),
           (dict(blob_of=OK + 2), b"aligned"), (dict(tensor_end=OK + 2), b"aligned")]
    bad += [({name: None}, b"required") for name in ("tensor_end", "lr", "step", "beta_pow", "params", "exp_avg", "exp_avg_sq", "blob",
                                                      "blob_of", "stats", "stats_sum", "max_grad_tensor", "tensor_norms", "scal")]
    for kw, msg in bad:
        rc, err = adamw(_structs(**kw)[2])
        assert rc == _capi.GD_ERR_INVALID and msg in err and b"gd_bc_adamw" in err, (kw, err)
    rc, err = adamw(_structs()[2], None)
    assert rc == _capi.GD_ERR_INVALID and b"null" in err
    rc, err = adamw(_structs()[2], OK + 2)
    assert rc == _capi.GD_ERR_INVALID and b"aligned" in err
    # a layout of another configuration is another G, blob and T
    other = _structs(R=5)[2]
    rc, err = adamw(_structs(grad_floats=other.grad_floats)[2])
    assert rc == _capi.GD_ERR_INVALID and b"grad_floats" in err

    def update(p, g, o, n=3, args=(OK,) * 3, expert=OK):
        return L.gd_bc_update(C.byref(p), C.byref(g), C.byref(o), *args, n, expert, None), L.gd_last_error()

    for kw in bad:
        rc, err = update(*_structs(**kw[0]))
        assert rc == _capi.GD_ERR_INVALID and b"gd_bc_update" in err, (kw, err)
    for name in ("actions", "nll", "grad_nll", "grad"):
        rc, err = update(*_structs(**{name: None}))
        assert rc == _capi.GD_ERR_INVALID and b"null" in err, (name, err)
    rc, err = update(*_structs(grad=OK + 4))
    assert rc == _capi.GD_ERR_INVALID and b"aligned" in err
    for n, msg in ((0, b"n must be"), (9, b"max_rows"), (-3, b"n must be")):
        rc, err = update(*_structs(), n=n)
        assert rc == _capi.GD_ERR_INVALID and msg in err, (n, err)
    rc, err = update(*_structs(max_rows=0), n=1)
    assert rc == _capi.GD_ERR_INVALID and b"max_rows" in err
    rc, err = update(*_structs(blob=OK + 64))
    assert rc == _capi.GD_ERR_INVALID and b"must be opt's" in err
    # p of one configuration, opt of another (each consistent in itself)
    p, g, _ = _structs(R=1)
    rc, err = update(p, g, _structs(R=5)[2])
    assert rc == _capi.GD_ERR_INVALID and b"differ" in err
    p, g, o = _structs()
    g.num_partials = 0
    rc, err = update(p, g, o)
    assert rc == _capi.GD_ERR_INVALID and b"num_partials" in err
    p, g, o = _structs()
    p.chunk_rows = 0
    rc, err = update(p, g, o)
    assert rc == _capi.GD_ERR_INVALID and b"chunk_rows" in err
    for i in range(3):
        rc, err = update(*_structs(), args=[None if j == i else OK for j in range(3)])
        assert rc == _capi.GD_ERR_INVALID and b"null" in err
    rc, err = update(*_structs(), expert=None)
    assert rc == _capi.GD_ERR_INVALID and b"null" in err
    # everything in order up to the alignment of obs, which is checked last
    rc, err = update(*_structs(), args=(OK + 2, OK, OK))
    assert rc == _capi.GD_ERR_INVALID and b"aligned" in err


def test_blob_of_inverts_pack_index():
    from gpudrive_lab_amd.bc_opt import blob_of, tensor_end
    from gpudrive_lab_amd.bc_train import grad_floats
    padded = 0
    for R, cfg in LAYOUTS:
        lay = _layout_args(R, cfg)
        index, inv, G = BP.pack_index(*lay), blob_of(*lay), grad_floats(*lay)
        assert inv.dtype == np.int32 and inv.shape == (G,)
        assert (np.bincount(index, minlength=G + 1)[:G] == 1).all()
        assert np.array_equal(index[inv], np.arange(G)) and len(set(inv.tolist())) == G
        pad = int((index == G).sum())
        assert pad == len(index) - G
        # one padding column of 64 rows per first layer of odd width (6 R for ego and partners, 13 R for roads)
        assert pad == 64 * sum(k % 2 for k in (6 * R, 6 * R, 13 * R))
        padded += pad > 0
        end = tensor_end(BP.expected_shapes(*lay))
        assert end.dtype == np.int32 and end[-1] == G and (np.diff(end) > 0).all()
        assert len(end) == 48 + 16 * (cfg["num_layer"][0] + 2 * cfg["num_layer"][1]) + 36 + 2 * (cfg["head_num_layers"] + 2)
    assert padded >= 2 and len(BP.expected_shapes(*_layout_args(*LAYOUTS[-1]))) == 288
    assert any(cfg["head_num_layers"] == 0 for _, cfg in LAYOUTS)


def test_blob_of_refuses_a_layout_that_is_no_permutation(monkeypatch):
    from gpudrive_lab_amd import bc_opt
    lay = _layout_args(1, GR.MINIMAL)
    index = BP.pack_index(*lay)
    twice = index.copy()
    twice[np.flatnonzero(index == 7)[0]] = 8       # parameter 7 has no place, parameter 8 two
    monkeypatch.setattr(bc_opt.BP, "pack_index", lambda *a: twice)
    with pytest.raises(ValueError, match="exactly one place"):
        bc_opt.blob_of(*lay)
    monkeypatch.setattr(bc_opt.BP, "pack_index", lambda *a: np.concatenate([index, [3]]))
    with pytest.raises(ValueError, match="exactly one place"):
        bc_opt.blob_of(*lay)


# ---- the host-side refusals

def test_the_constructor_refuses_on_the_host(monkeypatch):
    from gpudrive_lab_amd import DeviceBC
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library is not needed for a refusal"))
    sd = BC.state_dict(1)
    base = dict(max_agents=64, num_stack=1, batch_size=8, **BC.CFG)
    for kw in (dict(dropout=0.1), dict(dropout=True), dict(use_tom="guide_weighted"), dict(act_func="selu"), dict(network_dim=128),
               dict(max_agents=100), dict(num_stack=0), dict(num_layer=(3,)), dict(n_components=0), dict(chunk_rows=0),
               dict(batch_size=0), dict(batch_size=(1 << 20) + 1), dict(batch_size=8.0), dict(batch_size=True),
               dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(0.9,)), dict(betas=0.9), dict(betas=(0.9, float("nan"))),
               dict(eps=0.0), dict(eps=-1e-4), dict(eps=None), dict(learning_rate=0.0), dict(learning_rate=float("inf")),
               dict(max_grad_norm=0.0), dict(max_grad_norm=-20.0), dict(weight_decay=-0.01), dict(weight_decay=float("nan")),
               dict(weight_decay=None), dict(partials=0), dict(partials=4097), dict(partials=2.0), dict(amsgrad=True),
               dict(device="cpu"), dict(device="no such device")):
        with pytest.raises(ValueError):
            DeviceBC(sd, **dict(base, **kw))
    for bad in ({k: v for k, v in sd.items() if k != "head.head.bias"}, dict(sd, extra=torch.zeros(1)),
                dict(sd, **{"head.head.bias": sd["head.head.bias"].double()}), BC.state_dict(5)):
        with pytest.raises(ValueError):
            DeviceBC(bad, **base)
    with pytest.raises(ValueError, match="GPU"):
        DeviceBC(sd, **dict(base, device="cpu"))   # everything else in order: the refusal is the device's


def _hollow(A=64, R=1, cfg=BC.CFG, batch_size=4):
    """A DeviceBC with no device behind it: what the host-side checks of update and of the state dicts read."""
    from gpudrive_lab_amd.bc_opt import DeviceBC
    bc, pol = object.__new__(DeviceBC), object.__new__(BP.DeviceBCPolicy)
    pol.num_stack, pol.max_agents, pol.obs_width, pol.device = R, A, BP.obs_width(A), torch.device("cpu")
    bc.policy, bc.batch_size, bc.device = pol, batch_size, pol.device
    bc._shapes = BP.expected_shapes(*_layout_args(R, cfg))
    bc._names = tuple(bc._shapes)
    bc.betas, bc.eps, bc.weight_decay, bc.learning_rate = (0.9, 0.999), 1e-4, 0.01, 5e-4
    bc._L = bc._p = bc._g = bc._o = None   # a check that lets a call through fails on these
    return bc


def test_update_and_fit_refuse_on_the_host():
    bc = _hollow()
    A, R, D = 64, 1, BP.obs_width(64)

    def args(B=3, **kw):
        a = dict(obs=torch.zeros(B, R, D), expert_actions=torch.zeros(B, 1, 3), partner_mask=torch.zeros(B, R, A - 1, dtype=torch.bool),
                 road_mask=torch.zeros(B, R, 200, dtype=torch.bool))
        a.update(kw)
        return a

    for kw in (dict(B=5), dict(B=0), dict(obs=torch.zeros(3, R, D + 1)), dict(obs=torch.zeros(3, R + 1, D)),
               dict(obs=torch.zeros(3, R, D, dtype=torch.float64)), dict(obs=torch.zeros(3, D, R).transpose(1, 2)), dict(obs=None),
               dict(expert_actions=torch.zeros(3, 2)), dict(expert_actions=torch.zeros(4, 1, 3)), dict(expert_actions=torch.zeros(3, 3).double()),
               dict(expert_actions=np.zeros((3, 3), np.float32)), dict(partner_mask=torch.zeros(3, R, A, dtype=torch.bool)),
               dict(partner_mask=torch.zeros(3, R, A - 1)), dict(road_mask=torch.zeros(3, R, 199, dtype=torch.bool)), dict(road_mask=None)):
        with pytest.raises(ValueError):
            bc.update(**args(**kw))
    with pytest.raises(ValueError, match="batch_size"):
        bc.update(**args(B=5))
    with pytest.raises(ValueError):
        cuda = _hollow()
        cuda.policy.device = cuda.device = torch.device("cuda", 0)
        cuda.update(**args())                      # tensors on another device
    ok = args()
    assert bc.policy._inputs(ok["obs"], ok["partner_mask"], ok["road_mask"]) == 3 and bc.policy._expert(ok["expert_actions"], 3).shape == (3, 3)

    class DS:
        def __len__(self):
            return 0

        def batches(self, *a, **k):
            pytest.fail("nothing is gathered for a refusal")

    for ds, steps in (("a dataset", 3), (DS(), 3), (DS(), -1), (DS(), 2.0), (DS(), True)):
        with pytest.raises(ValueError):
            bc.fit(ds, steps)
    for x in (0.0, -1.0, None, float("nan"), True):
        with pytest.raises(ValueError):
            bc.set_learning_rate(x)


def test_load_optimizer_state_dict_refuses_on_the_host():
    bc = _hollow(cfg=GR.MINIMAL)
    ps = [torch.nn.Parameter(torch.zeros(s)) for s in bc._shapes.values()]
    n = len(ps)

    def good(**kw):
        opt = torch.optim.AdamW(ps, lr=5e-4, eps=1e-4, weight_decay=0.01, **kw)
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt.step()
        return opt.state_dict()

    def variant(f):
        sd = good()
        f(sd)
        return sd

    bad = [None, {}, {"state": {}}, dict(good(), param_groups=[]), dict(good(), param_groups=good()["param_groups"] * 2),
           good(amsgrad=True), good(maximize=True), good(betas=(0.8, 0.999)),
           variant(lambda sd: sd["param_groups"][0].update(params=list(range(n - 1)))),
           variant(lambda sd: sd["param_groups"][0].update(eps=1e-8)),
           variant(lambda sd: sd["param_groups"][0].update(weight_decay=-1.0)),
           variant(lambda sd: sd["param_groups"][0].update(weight_decay=float("nan"))),
           variant(lambda sd: sd["param_groups"][0].update(lr=0.0)),
           variant(lambda sd: sd["state"].pop(0)),
           variant(lambda sd: sd["state"][1].update(step=torch.tensor(2.0))),
           variant(lambda sd: [st.update(step=torch.tensor(-1.0)) for st in sd["state"].values()]),
           variant(lambda sd: sd["state"][2].pop("exp_avg")),
           variant(lambda sd: sd["state"][2].update(exp_avg=sd["state"][2]["exp_avg"].double())),
           variant(lambda sd: sd["state"][0].update(exp_avg_sq=sd["state"][0]["exp_avg_sq"].reshape(-1)[:-1]))]
    for sd in bad:
        with pytest.raises(ValueError):
            bc.load_optimizer_state_dict(sd)
    with pytest.raises(AttributeError):
        bc.load_optimizer_state_dict(good())       # (the checks pass: the load reaches the missing device buffers)


# ---- the rule on the host

@pytest.mark.parametrize("n", UR.ROWS)
def test_the_row_rule_against_float64(n):
    x = UR.row_inputs(n)
    got, w = UR.run_rows_host(*x)
    r64, w64 = UR.rows_reference(*x, torch.float64)
    r32, w32 = UR.rows_reference(*x, torch.float32)
    worst = 0.0
    for k, name in enumerate(UR.STATS):
        assert np.isfinite(got[k]), name
        err, E = UR.error_floor(got[k], r64[k], r32[k])
        worst = max(worst, UR.ratio_of(err, E))
        print("BCOPT RATIO rows n=%d %s err %.3e E %.3e ratio %.2f" % (n, name, err, E, UR.ratio_of(err, E)))
        assert err <= C_ROWS * E, (n, name, "error %.3g above %d E = %.3g" % (err, C_ROWS, C_ROWS * E))
    assert w.shape == (n,) and (w == np.float32(1.0) / np.float32(n)).all()
    assert np.abs(w - w64).max() <= 2.0 ** -24 / n and np.array_equal(w.astype(np.float64), w32), "torch's own 1 / n"
    print("BCOPT WORST rows n=%d %.2f" % (n, worst))


@pytest.mark.parametrize("weight_decay", [0.01, 0.0])
def test_the_adamw_rule_against_float64(weight_decay):
    names, end, G = UR.layout(1)
    assert G % 256 and any((e - b) % 256 for b, e in zip(np.concatenate([[0], end[:-1]]), end)), "short last partial sums"
    ad = dict(UR.ADAMW, weight_decay=weight_decay)
    p0 = np.random.default_rng(5).normal(0.0, 0.1, G).astype(np.float32)
    grads = UR.gradients(end)
    norms = [float(np.linalg.norm(g.astype(np.float64))) for g in grads]
    assert norms[0] > 20 + 1 and norms[1] < 20 - 1 and norms[2] > 20 + 1
    zt = UR.zero_tensor(end)
    zeros = slice(int(end[zt - 1]), int(end[zt]))
    assert (grads[0][zeros] == 0).all() and zeros.stop - zeros.start == 4096
    for g in grads:   # the condition on the inputs: no float32 rounding can change which tensor is the largest
        top = np.sort(UR.tensor_norms64(g, end))[-2:]
        assert top[1] - top[0] > 1e-3 * top[1], top
    z = np.zeros(G, np.float32)
    host = UR.run_adamw_host(p0, z, z, grads, end, **ad)
    r64 = UR.adamw_reference(p0, grads, end, torch.float64, **ad)
    r32 = UR.adamw_reference(p0, grads, end, torch.float32, **ad)
    worst = 0.0
    for s in range(3):
        what = "step %d wd %g" % (s + 1, weight_decay)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            err, E = UR.error_floor(host[s][k], r64[s][k], r32[s][k])
            ratio = UR.ratio_of(err, E)
            worst = max(worst, ratio)
            print("BCOPT RATIO adamw %s %s err %.3e E %.3e ratio %.2f" % (what, k, err, E, ratio))
            assert err <= C_ADAMW * E, (what, k, "error %.3g above %d E = %.3g" % (err, C_ADAMW, C_ADAMW * E))
        n64 = UR.tensor_norms64(grads[s], end)
        coef = min(1.0, 20.0 / (norms[s] + 1e-6))
        assert (np.abs(host[s]["tensor_norms"] - n64) <= 2.0 ** -22 * n64).all(), what
        assert abs(float(host[s]["total"]) - r64[s]["total"]) <= 2.0 ** -22 * r64[s]["total"], what
        assert abs(float(host[s]["total"]) - norms[s]) <= 2.0 ** -22 * norms[s], what
        assert abs(float(host[s]["max_grad_norm"]) - r64[s]["max_grad_norm"]) <= 2.0 ** -21 * r64[s]["max_grad_norm"], what
        assert abs(r64[s]["max_grad_norm"] - coef * n64.max()) <= 1e-12 * n64.max(), "the restated get_grad_norm"
        assert host[s]["max_grad_tensor"] == int(np.argmax(n64)) == r64[s]["max_grad_tensor"], what
        assert host[s]["step"] == s + 1
        assert host[s]["beta_pow"][0] == pytest.approx(0.9 ** (s + 1), rel=1e-15)
        assert host[s]["beta_pow"][1] == pytest.approx(0.999 ** (s + 1), rel=1e-15)
    print("BCOPT WORST adamw wd %g %.2f" % (weight_decay, worst))
    assert host[0]["tensor_norms"][zt] == 0
    # exact zeros of the first gradient: the first step only decays those weights, and leaves their moments at zero
    decay = np.float32(1.0 - float(np.float32(ad["lr"])) * float(np.float32(weight_decay)))
    assert np.array_equal(host[0]["params"][zeros], p0[zeros] * decay)
    assert (host[0]["exp_avg"][zeros] == 0).all() and (host[0]["exp_avg_sq"][zeros] == 0).all()
    if weight_decay == 0:
        assert decay == 1 and np.array_equal(host[0]["params"][zeros], p0[zeros])
    # below max_grad_norm the coefficient is exactly 1: the second step's moments from the first step's, gradient unscaled
    m1, v1, g = host[0]["exp_avg"], host[0]["exp_avg_sq"], grads[1]
    omb1, b2, omb2 = np.float32(1.0 - 0.9), np.float32(0.999), np.float32(1.0 - 0.999)
    assert np.array_equal(host[1]["exp_avg"], m1 + (g - m1) * omb1)
    assert np.array_equal(host[1]["exp_avg_sq"], v1 * b2 + omb2 * (g * g))
    # the state carries over: steps two and three from the first step's state give the same bits
    again = UR.run_adamw_host(host[0]["params"], host[0]["exp_avg"], host[0]["exp_avg_sq"], grads[1:], end, step=1,
                              beta_pow=host[0]["beta_pow"], **ad)
    for s in (0, 1):
        for k in ("params", "exp_avg", "exp_avg_sq", "beta_pow", "tensor_norms"):
            assert np.array_equal(again[s][k], host[s + 1][k])
        assert again[s]["step"] == s + 2 and again[s]["total"] == host[s + 1]["total"]


def test_without_weight_decay_the_step_is_the_ppo_rules_adam_bit_for_bit():
    """The same inputs through both host programs.  With the gradient taken as ONE tensor the sum of squares has the PPO
    rule's order, so everything agrees by construction; in the real layout the per-tensor sums add up to a float64 that
    rounds to the same float32 norm on these inputs, and everything agrees again."""
    _, end, G = UR.layout(1)
    p0 = np.random.default_rng(5).normal(0.0, 0.1, G).astype(np.float32)
    grads = UR.gradients(end)
    z = np.zeros(G, np.float32)
    ad = dict(UR.ADAMW, weight_decay=0.0)
    ppo = PR.run_adam_host(p0, z, z, grads, lr=ad["lr"], betas=ad["betas"], eps=ad["eps"], max_norm=ad["max_norm"])
    one = UR.run_adamw_host(p0, z, z, grads, np.array([G], np.int32), **ad)
    for s in range(3):
        for k in ("params", "exp_avg", "exp_avg_sq", "beta_pow"):
            assert np.array_equal(one[s][k].view(np.int32), ppo[s][k].view(np.int32)), (s, k)
        assert one[s]["total"] == ppo[s]["total"] == one[s]["tensor_norms"][0] and one[s]["step"] == ppo[s]["step"]
        assert one[s]["max_grad_tensor"] == 0
    real = UR.run_adamw_host(p0, z, z, grads, end, **ad)
    for s in range(3):
        assert real[s]["total"] == ppo[s]["total"], "the float32 norm of these inputs does not depend on the cut"
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(real[s][k].view(np.int32), ppo[s][k].view(np.int32)), (s, k)
    # and weight decay is what makes the difference
    wd = UR.run_adamw_host(p0, z, z, grads[:1], end, **UR.ADAMW)
    assert not np.array_equal(wd[0]["params"], real[0]["params"]) and np.array_equal(wd[0]["exp_avg"], real[0]["exp_avg"])
