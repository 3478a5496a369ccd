"""The BC policy at network_dim = 128 without a GPU: the restatement at that width against the reference module, the wide layout of
the blob against an emulation of the wide kernels' lane maps, the unchanged 64-wide results, every refusal, the new struct
and the C entry points' checks."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP
from tests import bc_cases as BC
from tests import bc_reference as REF
from tests import bc_wide_cases as WC
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 32  # the project's bound: an error of at most K E against the float64 restatement


# ---- the pin to the reference module

@pytest.mark.parametrize("name", WC.GOLDEN_CASES + WC.EDGE_GOLDEN_CASES)
def test_expected_shapes_are_the_reference_modules(name):
    B, A, R, cfg = WC.lookup(name)
    g = np.load(os.path.join(GOLDEN, "bc_wide_forward_%s.npz" % name))
    want = WC.shapes(R, cfg)
    assert [str(n) for n in g["names"]] == list(want)  # the reference module's own names, in its own order
    assert [tuple(int(v) for v in str(s).split(",")) for s in g["shapes"]] == list(want.values())
    assert want["head.input_layer.0.weight"] == (64, 384) and want["fusion_attn.0.0.module.attention.q_proj.weight"] == (128, 128)
    assert want["head.head.weight"] == (7 * cfg["n_components"], 64)


@pytest.mark.parametrize("name", WC.GOLDEN_CASES + WC.EDGE_GOLDEN_CASES)
def test_restatement_equals_the_reference_module(name):
    g = np.load(os.path.join(GOLDEN, "bc_wide_forward_%s.npz" % name))
    c = WC.case(name)
    ref = c["ref"]
    comp, act = REF.deterministic_action(ref["means"], ref["weights"])
    got = dict(context=ref["context"], means=ref["means"][:, None], covariances=ref["covariances"][:, None],
               weights=ref["weights"][:, None], action=act[:, None], ego_attn_score=ref["ego_attn_score"],
               nll=ref["nll"][:, None])
    assert got["context"].shape == (c["B"], 384) and got["ego_attn_score"].shape == (c["B"], 4, c["A"] - 1)
    for k, v in got.items():
        assert g[k].shape == v.shape, k
        assert np.abs(g[k] - v).max() <= 1e-12 * np.abs(g[k]).max(), k


# (wrong, case, output): the encoder's mistakes move the context; "ctx192" is a mistake of the head, which reads the context and
# cannot move it, so it is held to the same bound on the means
@pytest.mark.parametrize("wrong,name,output", [("scale16", "wide_min", "context"), ("heads_of_16", "wide_a128", "context"),
                                               ("ctx192", "wide_sweep", "means"), ("ln64", "wide_sweep", "context")])
def test_the_comparison_catches_each_wide_mistake(wrong, name, output):
    c = WC.case(name)
    bad = REF.forward(c["sd"], c["obs"], c["pm"], c["rm"], c["A"], wrong=wrong, **c["cfg"])
    moved = np.abs(bad[output] - c["ref"][output]).max()
    print("%s on %s: %s moves by %.3g = %.3g E" % (wrong, name, output, moved, moved / c["E"][output]))
    assert moved >= 4 * K * c["E"][output]
    if wrong == "ctx192":
        assert np.array_equal(bad["context"], c["ref"]["context"])


# ---- the blob at 128: an emulation of what the kernels read at T = 4 (csrc/bc_tile.hpp), written out again here

FW, T, F = 128, 4, 64
LANE = np.arange(64)
COL, HALF = LANE & 31, LANE >> 5


def _acc(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


class Blob:
    """Reads a blob front to back in the order the wide kernels' offsets state."""

    def __init__(self, blob):
        self.b, self.o = blob, 0

    def nat(self, n):
        v = self.b[self.o:self.o + n]
        self.o += n
        return v

    def first(self, kin):
        """embed_first128: the A operand of k-step s for output tile t is w0[(t ks + s) 64 + lane] = W[32 t + c][2 s + h]."""
        ks = (kin + 1) // 2
        w0 = self.nat(T * ks * 64)
        W = np.zeros((FW, 2 * ks))
        for t in range(T):
            for s in range(ks):
                W[32 * t + COL, 2 * s + HALF] = w0[(t * ks + s) * 64 + LANE]
        assert not W[:, kin:].any()  # the kernel feeds x = 0 there; the weight it reads must be the padding zero
        return W[:, :kin]

    def mfma(self):
        """linear at T = 4: the A operand of k-step (t, r) for output tile t2 is w[((t2 4 + t) 16 + r) 64 + lane]."""
        w = self.nat(FW * FW)
        W = np.full((FW, FW), np.nan)
        for t2 in range(T):
            for t in range(T):
                for r in range(16):
                    W[32 * t2 + COL, 32 * t + _acc(r, HALF)] = w[((t2 * T + t) * 16 + r) * 64 + LANE]
        return W

    def trans(self, out, inp):
        """block_matvec128 and the head's loops: wt[k * out + o] = W[o][k]."""
        return self.nat(inp * out).reshape(inp, out).T


def unpack_wide(blob, R, num_layer, head_layers, C_):
    """The state dict the wide kernels see in `blob`, by the reference's names."""
    rd, sd = Blob(blob), {}

    def put(name, w):
        sd[name + ".weight"] = w
        sd[name + ".bias"] = rd.nat(w.shape[0])

    def norm(name):
        sd[name + ".weight"], sd[name + ".bias"] = rd.nat(FW), rd.nat(FW)

    for net, k in zip(BP.NETS, BP.NET_K):
        put(net + ".0", rd.first(k * R))
        norm(net + ".2")
        for i in range(1, 4):
            put("%s.%d" % (net, 4 * i), rd.mfma())
            norm("%s.%d" % (net, 4 * i + 2))
    for blk, n in zip(BP.SELF_BLOCKS, (num_layer[0], num_layer[1], num_layer[1])):
        for i in range(n):
            p = "%s.%d" % (blk, i)
            norm(p + ".0.module.norm")
            for proj in "qkvo":
                put(p + ".0.module.attention.%s_proj" % proj, rd.mfma())
            norm(p + ".1.module.0")
            put(p + ".1.module.1", rd.mfma())
            put(p + ".1.module.3", rd.mfma())
    for p in BP.CROSS_LAYERS:
        norm(p + ".0.module.q_norm")
        norm(p + ".0.module.kv_norm")
        put(p + ".0.module.attention.q_proj", rd.trans(FW, FW))
        put(p + ".0.module.attention.k_proj", rd.mfma())
        put(p + ".0.module.attention.v_proj", rd.mfma())
        put(p + ".0.module.attention.o_proj", rd.trans(FW, FW))
        norm(p + ".1.module.0")
        put(p + ".1.module.1", rd.trans(FW, FW))
        put(p + ".1.module.3", rd.trans(FW, FW))
    put("head.input_layer.0", rd.trans(F, 3 * FW))
    for i in range(head_layers):
        put("head.residual_block.%d.0" % i, rd.trans(F, F))
    put("head.head", rd.trans(7 * C_, F))
    assert rd.o == blob.size
    return sd


def test_pack_index_at_128_is_what_the_wide_kernels_read():
    c = WC.case("wide_min")
    R, cfg = c["R"], c["cfg"]
    idx = BP.pack_index(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], network_dim=128)
    names = list(WC.shapes(R, cfg))
    flat = np.concatenate([c["sd"][k].numpy().astype(np.float64).reshape(-1) for k in names] + [np.zeros(1)])
    total = flat.size - 1
    real = idx[idx != total]
    assert np.array_equal(np.sort(real), np.arange(total))  # every parameter lands exactly once
    odd = sum(128 for k in BP.NET_K if (k * R) % 2)  # one zero column per odd first layer, and nothing else points at the zero
    assert idx.size - real.size == odd == 128
    seen = unpack_wide(flat[idx], R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"])
    assert list(seen) == names
    for k in names:  # exact: a gather moves bits
        assert np.array_equal(seen[k], c["sd"][k].numpy().astype(np.float64)), k
    # and the forward on what the kernels see is the reference's: embedders, the self layers, the cross layers and the head
    got = REF.forward(seen, c["obs"], c["pm"], c["rm"], c["A"], **cfg)
    for k in ("context", "raw", "ego_attn_score"):  # (the same float64 values through other strides: BLAS may round otherwise)
        assert np.abs(got[k] - c["ref"][k]).max() <= 1e-12 * np.abs(c["ref"][k]).max(), k


@pytest.mark.parametrize("R,num_layer,hl,C_", [(5, (4, 3), 2, 6), (2, (1, 2), 1, 2), (8, (4, 4), 4, 16)])
def test_pack_index_at_128_is_a_permutation_and_the_library_agrees_on_its_size(R, num_layer, hl, C_):
    idx = BP.pack_index(R, num_layer, hl, C_, network_dim=128)
    total = sum(int(np.prod(s)) for s in BP.expected_shapes(R, num_layer, hl, C_, network_dim=128).values())
    real = idx[idx != total]
    assert np.array_equal(np.sort(real), np.arange(total))
    assert idx.size - real.size == sum(128 for k in BP.NET_K if (k * R) % 2) and idx.max() <= total
    unpack_wide(np.arange(idx.size, dtype=np.float64) * 0.0, R, num_layer, hl, C_)  # the walk ends at the blob's end
    p, o = _dim_struct(R, num_layer, hl, C_, 128)
    L = _capi.lib()
    p.base.blob_floats = idx.size + 1
    assert _call(L, p, o) == _capi.GD_ERR_INVALID and "blob_floats" in L.gd_last_error().decode()
    p.base.blob_floats, p.base.max_agents = idx.size, 65  # with the right size the NEXT check speaks
    assert _call(L, p, o) == _capi.GD_ERR_INVALID and "max_agents" in L.gd_last_error().decode()
    p.base.max_agents, p.base.blob = 64, 4100
    assert _call(L, p, o) == _capi.GD_ERR_INVALID and "aligned" in L.gd_last_error().decode()


@pytest.mark.parametrize("R,num_layer,hl,C_", [(5, (3, 2), 2, 6), (1, (1, 1), 0, 1), (8, (4, 4), 4, 16)])
def test_the_64_wide_layout_is_unchanged(R, num_layer, hl, C_):
    assert np.array_equal(BP.pack_index(R, num_layer, hl, C_), BP.pack_index(R, num_layer, hl, C_, network_dim=64))
    a, b = BP.expected_shapes(R, num_layer, hl, C_), BP.expected_shapes(R, num_layer, hl, C_, network_dim=64)
    assert a == b and list(a) == list(b)
    assert a["head.input_layer.0.weight"] == (64, 192)
    assert BP.scratch_floats(128, 128) == BP.scratch_floats(128, 128, 64) == 128 * 3 * 328 * 64
    assert BP.scratch_floats(128, 128, 128) * 4 == 64487424  # 64.5 MB


# ---- the refusals

def test_every_refusal_at_128():
    B, A, R, cfg = WC.CASES["wide_min"]
    wide, narrow = BC.state_dict(R, cfg, network_dim=WC.DIM), BC.state_dict(R, cfg, network_dim=64)
    ok = dict(max_agents=A, num_stack=R, num_head=4, **cfg)
    both = dict(network_dims=(64, 128))
    assert list(BP.check_bc_args(wide, network_dim=128, **both, **ok)) == list(wide)
    assert list(BP.check_bc_args(narrow, network_dim=64, **both, **ok)) == list(narrow)
    for bad in (96, 256, 128.0, True):
        with pytest.raises(ValueError, match="network_dim"):
            BP.check_bc_args(wide, network_dim=bad, **both, **ok)
    with pytest.raises(ValueError, match="network_dim must be 64 \\(nothing else is built\\)"):
        BP.check_bc_args(wide, network_dim=128, **ok)  # by default only 64: what the backward and the optimiser pass
    for bad in (128, 96):
        with pytest.raises(ValueError, match="head_dim"):
            BP.check_bc_args(wide, network_dim=128, head_dim=bad, **both, **ok)
    with pytest.raises(ValueError, match="shape \\(128, 6\\)"):
        BP.check_bc_args(narrow, network_dim=128, **both, **ok)
    with pytest.raises(ValueError, match="shape"):
        BP.check_bc_args(wide, network_dim=64, **both, **ok)
    with pytest.raises(ValueError, match="shape \\(128, 6\\)"):
        BP.DeviceBCPolicy(narrow, device="cpu", network_dim=128, **ok)
    with pytest.raises(ValueError, match="GPU"):  # a wide state dict passes every host check
        BP.DeviceBCPolicy(wide, device="cpu", network_dim=128, **ok)
    with pytest.raises(ValueError, match="network_dim"):
        BP.DeviceBCPolicy(wide, device="cpu", network_dim=96, **ok)


def test_training_refuses_128():
    from gpudrive_lab_amd.bc_opt import DeviceBC
    from gpudrive_lab_amd.bc_train import TrainableBCPolicy
    B, A, R, cfg = WC.CASES["wide_min"]
    wide = BC.state_dict(R, cfg, network_dim=WC.DIM)
    ok = dict(max_agents=A, num_stack=R, num_head=4, **cfg)
    with pytest.raises(ValueError, match="TrainableBCPolicy: network_dim must be 64"):
        TrainableBCPolicy(wide, network_dim=128, **ok)
    with pytest.raises(ValueError, match="DeviceBC: network_dim must be 64"):
        DeviceBC(wide, network_dim=128, **ok)


def _stub_policy(network_dim):
    p = object.__new__(BP.DeviceBCPolicy)
    p.max_agents, p.num_stack, p.num_layer, p.network_dim = 64, 1, (1, 1), network_dim
    return p


def test_what_reads_64_wide_tokens_refuses_a_wide_policy_before_the_device():
    from gpudrive_lab_amd.bc_readout import ProbeReadout
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    from gpudrive_lab_amd.lp_probe import DeviceLinearProbe
    pol = _stub_policy(128)  # (no device, no blob: anything past the check would raise AttributeError)
    assert object.__new__(BP.DeviceBCPolicy).network_dim == 64
    with pytest.raises(ValueError, match="network_dim"):
        pol.hidden(None, None, None)
    with pytest.raises(ValueError, match="network_dim"):
        pol.read(None, None, None, readout=object())
    with pytest.raises(ValueError, match="network_dim"):
        pol.forward(None, None, None, ("actions",), readout=object())
    with pytest.raises(ValueError, match="network_dim"):
        ProbeReadout(pol, "ro_attn", 0, ego=[])
    with pytest.raises(ValueError, match="network_dim"):
        DeviceLinearProbe(pol, {}, model="early_lp", exp="ego")
    loop = object.__new__(ClosedLoopBC)
    loop.policy = pol
    with pytest.raises(ValueError, match="network_dim"):
        loop.run(readout=object())


# ---- the C surface

def test_struct_matches_the_header():
    hdr = os.path.join(ROOT, "include")
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "gpudrive_amd.h"\nint main() { printf("%zu %zu %zu %zu\\n", '
           "sizeof(gd_bc_policy_dim), offsetof(gd_bc_policy_dim, base), offsetof(gd_bc_policy_dim, network_dim), "
           "offsetof(gd_bc_policy_dim, reserved)); return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", hdr, "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        want = [int(v) for v in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout.split()]
    S = _capi.GdBCPolicyDim
    assert [C.sizeof(S), S.base.offset, S.network_dim.offset, S.reserved.offset] == want == [72, 0, 64, 68]
    assert C.sizeof(_capi.GdBCPolicy) == 64  # gd_bc_policy has not grown


def test_symbols_are_declared_exported_and_bound():
    names = {"gd_bc_forward_dim", "gd_bc_forward_rows_dim", "gd_bc_rollout_dim"}
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
    assert len(L.gd_bc_forward_dim.argtypes) == 11 and len(L.gd_bc_forward_rows_dim.argtypes) == 13
    assert len(L.gd_bc_rollout_dim.argtypes) == 6


def _dim_struct(R, num_layer, hl, C_, dim, A=64, chunk=8):
    p, o = _capi.GdBCPolicyDim(), _capi.GdBCOutputs()
    b = p.base
    b.max_agents, b.num_stack, b.fusion_layers, b.branch_layers, b.head_layers, b.n_components = A, R, *num_layer, hl, C_
    b.clip_value, b.chunk_rows, b.blob, b.scratch = -20.0, chunk, 4096, 4096
    b.blob_floats = int(BP.pack_index(R, num_layer, hl, C_, network_dim=dim).size)
    b.scratch_floats = BP.scratch_floats(A, chunk, dim)
    p.network_dim, p.reserved = dim, 0
    return p, o


def _call(L, p, o, n=4):
    return L.gd_bc_forward_dim(C.byref(p), 4096, 4096, 4096, n, 1, None, None, None, C.byref(o), None)


def test_c_entries_refuse_before_the_device():
    """The checkers return a message for a bad struct; the pointers are junk and are never read."""
    L = _capi.lib()
    args = (5, (4, 3), 2, 6)
    p, o = _dim_struct(*args, 128)
    for field, bad, word in (("network_dim", 96, "network_dim"), ("network_dim", 0, "network_dim"), ("reserved", 1, "reserved")):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert _call(L, p, o) == _capi.GD_ERR_INVALID
        assert word in L.gd_last_error().decode(), (field, L.gd_last_error())
        setattr(p, field, keep)
    narrow, _ = _dim_struct(*args, 64)
    for field, word in (("scratch_floats", "scratch_floats"), ("blob_floats", "blob_floats")):  # sized for 64
        keep = getattr(p.base, field)
        setattr(p.base, field, getattr(narrow.base, field))
        assert _call(L, p, o) == _capi.GD_ERR_INVALID
        assert word in L.gd_last_error().decode() and "128" in L.gd_last_error().decode(), (field, L.gd_last_error())
        setattr(p.base, field, keep)
    p.network_dim = 64  # ... and a blob sized for 128 is not the 64-wide layout's
    assert _call(L, p, o) == _capi.GD_ERR_INVALID and "blob_floats" in L.gd_last_error().decode()
    p.network_dim = 128
    assert _call(L, p, o, n=0) == _capi.GD_ERR_INVALID and "n must be" in L.gd_last_error().decode()
    assert L.gd_bc_forward_dim(None, 4096, 4096, 4096, 4, 1, None, None, None, C.byref(o), None) == _capi.GD_ERR_INVALID
    assert L.gd_bc_forward_rows_dim(C.byref(p), 4096, 4096, 4096, 4, 1, None, None, None, C.byref(o), None, 4096, None) \
        == _capi.GD_ERR_INVALID
    p.reserved = 3
    assert L.gd_bc_forward_rows_dim(C.byref(p), 4096, 4096, 4096, 4, 1, None, None, None, C.byref(o), 4096, 4096, None) \
        == _capi.GD_ERR_INVALID and "reserved" in L.gd_last_error().decode()
    b, x = _capi.GdBCRolloutBuffers(), _capi.GdBCRolloutReads()
    assert L.gd_bc_rollout_dim(None, C.byref(p), C.byref(b), None, None, 91) == _capi.GD_ERR_INVALID
    assert L.gd_bc_rollout_dim(4096, C.byref(p), C.byref(b), None, None, 91) == _capi.GD_ERR_INVALID
    assert "reserved" in L.gd_last_error().decode()
    p.reserved = 0
    ro = _capi.GdBCReadout()
    x.readout = C.pointer(ro)
    assert L.gd_bc_rollout_dim(4096, C.byref(p), C.byref(b), None, C.byref(x), 91) == _capi.GD_ERR_INVALID
    assert "readout must be NULL" in L.gd_last_error().decode()
