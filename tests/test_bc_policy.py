"""The device BC policy forward without a GPU: the float64 restatement (bc_reference.py) pinned to the reference module's own
outputs (tests/golden/bc_forward_*.npz, written by tools/bc_reference_golden.py from the reference's EarlyFusionAttnBCNet in
float64 on the seeded weights and inputs of bc_cases.py), the blob's pack index, every refusal, the rule header on the host,
and four wrong rules shown caught."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP

from . import bc_cases as BC
from . import bc_grad_reference as GR
from . import bc_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_CACHE = {}


def case(B, A, R, cfg=BC.CFG):
    """The seeded case and its float64 restatement, computed once and shared (nobody writes into it).  At BC.CFG the weights
    and inputs are bc_cases' own (seed 1); at any other configuration (bc_cases.EDGE_CASES) they are the backward tests'
    (bc_grad_reference.state_dict and the input seed that keeps its margins), so that both suites share one case."""
    key = GR.case_key(B, A, R, cfg)
    if key not in _CACHE:
        if cfg is BC.CFG:
            sd, seed = BC.state_dict(R), 1
        else:
            sd, seed = GR.state_dict(R, cfg), GR.INPUT_SEEDS[key]
        obs, pm, rm, expert, u, z, kinds = BC.inputs(B, A, R, seed=seed)
        ref = REF.forward(sd, obs, pm, rm, A, **cfg)
        _CACHE[key] = dict(sd=sd, obs=obs, pm=pm, rm=rm, expert=expert, u=u, z=z, kinds=kinds, ref=ref, cfg=cfg)
    return _CACHE[key]


# ---- the surface

def test_symbols_header_and_structs():
    names = {"gd_bc_forward", "gd_bc_eval_accumulate"}
    assert names <= set(_capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    for n in names:
        assert re.search(r"\bint %s\(" % n, header)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_bc_forward.argtypes) == 11 and len(L.gd_bc_eval_accumulate.argtypes) == 6
    assert C.sizeof(_capi.GdBCPolicy) == 8 * 4 + 4 * 8 and _capi.GdBCPolicy.blob.offset == 32
    assert C.sizeof(_capi.GdBCOutputs) == 9 * 8
    rule = open(os.path.join(ROOT, "gpudrive_lab_amd", "csrc", "bc_rule.hpp")).read()
    assert "cannot be reproduced" in rule and "3.58352" in rule


def test_c_entry_refuses_before_the_device():
    """gd_bc_forward's checker returns a message for a bad struct; the pointers are never read (they are junk here)."""
    L = _capi.lib()
    p, o = _capi.GdBCPolicy(), _capi.GdBCOutputs()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers, p.head_layers, p.n_components = 64, 5, 3, 2, 2, 6
    p.clip_value, p.chunk_rows, p.blob, p.scratch = -20.0, 8, 4096, 4096
    p.blob_floats = int(BP.pack_index(5, (3, 2), 2, 6).size)
    p.scratch_floats = BP.scratch_floats(64, 8)

    def call(n=4, det=1, u=None, z=None, expert=None):
        return L.gd_bc_forward(C.byref(p), 4096, 4096, 4096, n, det, u, z, expert, C.byref(o), None)

    for field, bad, word in (("max_agents", 96, "max_agents"), ("num_stack", 9, "num_stack"), ("fusion_layers", 0, "fusion_layers"),
                             ("branch_layers", 5, "branch_layers"), ("head_layers", 5, "head_layers"),
                             ("n_components", 17, "n_components"), ("chunk_rows", 0, "chunk_rows"),
                             ("blob_floats", 7, "blob_floats"), ("scratch_floats", 7, "scratch_floats"), ("blob", 4100, "aligned"),
                             ("scratch", 4100 + 12, "aligned")):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert call() == _capi.GD_ERR_INVALID
        assert word in L.gd_last_error().decode(), (field, L.gd_last_error())
        setattr(p, field, keep)
    assert call(n=0) == _capi.GD_ERR_INVALID and call(det=0) == _capi.GD_ERR_INVALID
    assert "u and z" in L.gd_last_error().decode()
    o.nll = 4096
    assert call() == _capi.GD_ERR_INVALID and "expert_actions" in L.gd_last_error().decode()
    assert L.gd_bc_eval_accumulate(0, 4096, 4096, 4096, 4096, None) == _capi.GD_ERR_INVALID
    assert L.gd_bc_eval_accumulate(4, None, 4096, 4096, 4096, None) == _capi.GD_ERR_INVALID


# ---- the pin to the reference module

@pytest.mark.parametrize("B,A,R", BC.SHAPES)
def test_restatement_equals_the_reference_module(B, A, R):
    g = np.load(os.path.join(GOLDEN, "bc_forward_%d_%d_%d.npz" % (B, A, R)))
    want = BP.expected_shapes(R, BC.CFG["num_layer"], BC.CFG["head_num_layers"], BC.CFG["n_components"])
    assert [str(n) for n in g["names"]] == list(want)  # the reference module's own names, in its own order
    assert [tuple(int(v) for v in str(s).split(",")) for s in g["shapes"]] == list(want.values())
    c = case(B, A, R)
    ref = c["ref"]
    comp, act = REF.deterministic_action(ref["means"], ref["weights"])
    got = dict(context=ref["context"], means=ref["means"][:, None], covariances=ref["covariances"][:, None],
               weights=ref["weights"][:, None], action=act[:, None], ego_attn_score=ref["ego_attn_score"],
               nll=REF.nll(ref["means"], ref["log_covariances"], ref["weights"], c["expert"][:, 0])[:, None])
    for k, v in got.items():
        assert g[k].shape == v.shape, k
        assert np.abs(g[k] - v).max() <= 1e-12 * np.abs(g[k]).max(), k


# ---- the blob

@pytest.mark.parametrize("R,num_layer,hl,C_", [(5, (3, 2), 2, 6), (1, (1, 1), 0, 1), (8, (4, 4), 4, 16), (3, (2, 1), 1, 5)])
def test_pack_index_is_a_permutation(R, num_layer, hl, C_):
    idx = BP.pack_index(R, num_layer, hl, C_)
    total = sum(int(np.prod(s)) for s in BP.expected_shapes(R, num_layer, hl, C_).values())
    real = idx[idx != total]
    assert np.array_equal(np.sort(real), np.arange(total))  # every parameter lands exactly once
    odd = sum(64 for k in BP.NET_K if (k * R) % 2)  # one zero column per odd first layer
    assert idx.size - real.size == odd and idx.max() <= total
    p = _capi.GdBCPolicy()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers, p.head_layers, p.n_components = 64, R, *num_layer, hl, C_
    p.clip_value, p.chunk_rows, p.blob, p.scratch, p.scratch_floats = -1.0, 1, 4096, 4096, BP.scratch_floats(64, 1)
    o = _capi.GdBCOutputs()
    L = _capi.lib()
    p.blob_floats = idx.size + 1  # the C side computes the same size: one off is refused with that message
    assert L.gd_bc_forward(C.byref(p), 4096, 4096, 4096, 1, 1, None, None, None, C.byref(o), None) == _capi.GD_ERR_INVALID
    assert "blob_floats" in L.gd_last_error().decode()
    p.blob_floats, p.max_agents = idx.size, 65  # and with the right size the NEXT check speaks
    assert L.gd_bc_forward(C.byref(p), 4096, 4096, 4096, 1, 1, None, None, None, C.byref(o), None) == _capi.GD_ERR_INVALID
    assert "max_agents" in L.gd_last_error().decode()


# ---- the refusals

def test_every_refusal():
    sd = BC.state_dict(5)
    ok = dict(max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2, n_components=6, clip_value=-20.0)
    assert list(BP.check_bc_args(sd, **ok)) == list(sd)
    for name, bad in (("network_dim", 128), ("head_dim", 32), ("num_head", 8), ("network_num_layers", 3), ("act_func", "selu"),
                      ("dropout", 0.1), ("action_dim", 2), ("time_dim", 2), ("use_tom", "guide"), ("max_agents", 96),
                      ("max_agents", True), ("num_stack", 0), ("num_stack", 9), ("num_layer", (0, 2)), ("num_layer", (3, 5)),
                      ("num_layer", 3), ("head_num_layers", -1), ("head_num_layers", 5), ("n_components", 0),
                      ("n_components", 17), ("clip_value", float("nan")), ("clip_value", "low"), ("chunk_rows", 0),
                      ("chunk_rows", 5000)):
        with pytest.raises(ValueError, match=name):
            BP.check_bc_args(sd, **dict(ok, **{name: bad}))
    with pytest.raises(ValueError, match="mapping"):
        BP.check_bc_args([1, 2], **ok)
    some = "fusion_attn.1.0.module.attention.k_proj.weight"
    with pytest.raises(ValueError, match="missing"):
        BP.check_bc_args({k: v for k, v in sd.items() if k != some}, **ok)
    with pytest.raises(ValueError, match="unexpected"):
        BP.check_bc_args(dict(sd, **{"aux_head.0.weight": torch.zeros(64, 64)}), **ok)
    with pytest.raises(ValueError, match="shape"):
        BP.check_bc_args(dict(sd, **{some: torch.zeros(64, 32)}), **ok)
    with pytest.raises(ValueError, match="float32"):
        BP.check_bc_args(dict(sd, **{some: sd[some].double()}), **ok)
    with pytest.raises(ValueError, match="contiguous"):
        BP.check_bc_args(dict(sd, **{some: sd[some].t().contiguous().t()}), **ok)
    with pytest.raises(ValueError, match="missing"):  # another num_stack, layer count or mixture size is another state dict
        BP.check_bc_args(sd, **dict(ok, num_layer=(4, 2)))
    with pytest.raises(ValueError, match="shape"):
        BP.check_bc_args(sd, **dict(ok, num_stack=4))
    with pytest.raises(ValueError, match="shape"):
        BP.check_bc_args(sd, **dict(ok, n_components=5))
    with pytest.raises(ValueError, match="GPU"):
        BP.DeviceBCPolicy(sd, device="cpu", **ok)
    with pytest.raises(ValueError, match="unknown argument"):
        BP.DeviceBCPolicy(sd, device="cpu", rotary=True, **ok)


# ---- the rule header on the host

def _raws(C_, n=64, seed=3):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, 7 * C_)).astype(np.float32) * 2
    raw[:, 3 * C_:6 * C_] *= 6  # covariances on both sides of both clamps (-20 .. 3.58352 against clip -5)
    if C_ > 3:
        raw[0, 6 * C_ + 1] = raw[0, 6 * C_ + 3] = 9.0  # a tie at the top: the first index wins
    return raw


@pytest.mark.parametrize("C_", [1, 6, 16])
def test_rule_header_on_the_host_equals_the_float64_rule(C_):
    raw = _raws(C_)
    n, clip = raw.shape[0], -5.0
    rng = np.random.default_rng(5)
    z = rng.standard_normal((n, 3)).astype(np.float32)
    expert = rng.standard_normal((n, 3)).astype(np.float32) * 2
    mix = REF.mixture(raw, C_, clip)
    eps = 2.0 ** -24
    for u, det in ((rng.random(n).astype(np.float32), False), (BC.edge_uniforms(n), False), (np.zeros(n, np.float32), True)):
        got = BC.run_rule_host(raw, clip, u, z, expert, det)
        assert np.array_equal(got["log_covariances"], mix["log_covariances"].astype(np.float32))  # a clamp is exact
        assert (np.abs(got["covariances"] - mix["covariances"]) <= 4 * eps * mix["covariances"]).all()
        assert (np.abs(got["weights"] - mix["weights"]) <= (C_ + 4) * eps).all()
        if det:
            comp, act = REF.deterministic_action(mix["means"], got["weights"].astype(np.float64))
            assert np.array_equal(got["component"], comp) and np.array_equal(got["actions"], act.astype(np.float32))
            if C_ > 3:
                assert got["component"][0] == 1
        else:
            # the draw on the program's OWN weights: exact away from the running sums, either neighbour within 1e-5 of one
            w = got["weights"].astype(np.float64)
            comp, _ = REF.sampled_action(mix["means"], mix["covariances"], w, u, z)
            near = np.abs(REF.running_sums(w) - u[:, None].astype(np.float64)).min(-1) <= 1e-5
            assert (np.abs(got["component"] - comp) <= near).all() and not near.all()
            r = np.arange(n)
            want = mix["means"][r, got["component"]] + np.sqrt(mix["covariances"][r, got["component"]]) * z
            assert (np.abs(got["actions"] - want) <= 8 * eps * (np.abs(want) + np.abs(z) * 6 + 1)).all()
        nll = REF.nll(mix["means"], mix["log_covariances"], mix["weights"], expert)
        # the quadratic form is a sum of three terms of magnitude up to q; everything after it is O(1) operations
        q = ((expert[:, None] - mix["means"]) ** 2 / mix["covariances"]).sum(-1).min(-1)
        assert (np.abs(got["nll"] - nll) <= 16 * eps * (np.abs(nll) + q + 1)).all()
    got = BC.run_rule_host(raw, clip, BC.edge_uniforms(n), z, expert, False)
    assert (got["component"][1::2] == C_ - 1).all()  # u just below 1 takes the last component unless the sum reaches 1 early
    first = np.argmax(got["weights"] > 0, axis=-1)
    assert np.array_equal(got["component"][0::2], first[0::2])  # u = 0 takes the first component with any mass


# ---- wrong rules are caught

@pytest.mark.parametrize("wrong", ["inf_fill", "normed_residual", "entity_major", "tanh_gelu"])
def test_a_wrong_rule_is_caught(wrong):
    """On the B = 17 case the comparison the GPU test makes (error <= k E; a ratio above 16 is a bug, so k is 32 at the most)
    tells each wrong rule from the right one, with a factor 4 to spare.  The tanh form of GELU is the closest of the four
    (about 2.6e-3 against E of 7.6e-6).  The -inf fill can differ only where a row has every key masked: samples a, b, ab."""
    B, A, R = 17, 64, 5
    c = case(B, A, R)
    E = BC.yardstick(BC.standin_float32(c["sd"], c["obs"], c["pm"], c["rm"], A), c["ref"])
    bad = REF.forward(c["sd"], c["obs"], c["pm"], c["rm"], A, **BC.CFG, wrong=wrong)
    err = np.abs(bad["context"] - c["ref"]["context"]).max(-1)
    assert err.max() > 4 * 32 * E["context"]
    if wrong == "inf_fill":
        full = np.array(["a" in k or "b" in k for k in c["kinds"]])
        assert (err[full] > 4 * 32 * E["context"]).all() and (err[~full] == 0).all()
    assert 1e-7 < E["context"] < 1e-4  # the yardstick is a float32 forward's error, not zero and not a loose bound
