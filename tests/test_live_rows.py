"""CPU tests of the live-row policy forward (gd_live_rows, gd_policy_forward_rows, gd_policy_rollout_compact;
gpudrive_lab_amd.policy.live_rows / LiveRows, DevicePolicy(rows=), ClosedLoopPPO.run(compact=True)): the surface, the struct,
the refusals -- every one before anything is launched or any simulator touched -- and the byte count."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from gpudrive_lab_amd import _capi
from tests.conftest import ROOT
from tests.test_ppo_rollout import _StubSim, _stub_policy

HEADER = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
NAMES = ("gd_live_rows", "gd_policy_forward_rows", "gd_policy_rollout_compact")


def _declared_args(name):
    decl = re.search(r"^int %s\((.*?)\);" % name, HEADER, flags=re.S | re.M).group(1)
    return [a.strip() for a in decl.split(",")]


def test_the_symbols_are_declared_exported_and_bound():
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    for name, n_args in zip(NAMES, (6, 13, 5)):
        args = _declared_args(name)
        assert len(args) == n_args, (name, args)
        assert name in _capi.SYMBOLS and name in exported
        assert len(getattr(L, name).argtypes) == n_args, name
    assert _declared_args("gd_live_rows") == ["const uint8_t *mask", "int32_t n", "int32_t *rows", "int32_t *count",
                                              "int32_t *scratch", "void *stream"]
    # gd_policy_forward's ten arguments, plus d, rows and count
    fwd = _declared_args("gd_policy_forward")
    assert _declared_args("gd_policy_forward_rows") == (fwd[:1] + ["const gd_dropout *d"] + fwd[1:-1]
                                                        + ["const int32_t *rows", "const int32_t *count"] + fwd[-1:])
    at = L.gd_policy_rollout_compact.argtypes
    assert at[1]._type_ is _capi.GdPolicy and at[2]._type_ is _capi.GdPolicyRolloutBuffers
    assert at[3]._type_ is _capi.GdPolicyRolloutRows
    assert "#define GD_LIVE_ROWS_BLOCK %d\n" % _capi.LIVE_ROWS_BLOCK in HEADER


def test_the_struct_has_the_headers_fields():
    R = _capi.GdPolicyRolloutRows
    names = [f[0] for f in R._fields_]
    assert names == ["rows", "count", "scratch", "live_count", "reserved"]
    assert [getattr(R, n).offset for n in names] == [0, 8, 16, 24, 32] and ctypes.sizeof(R) == 40
    body = HEADER[HEADER.index("typedef struct gd_policy_rollout_rows {"):HEADER.index("} gd_policy_rollout_rows;")]
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"[ *](\w+)[,;]", code) == names, "the header declares other fields, or in another order"
    assert re.findall(r"(\w+) +\*?\w+;", code) == ["int32_t"] * 5


# ---- the C calls: every refusal comes before the first launch, so no pointer below is ever read (none points anywhere)
OK4, OK8, OK16, ODD = 0x10000, 0x20000, 0x30000, 0x40002  # aligned addresses of nothing, and one that is not 4-byte aligned


def _refused(rc, match):
    assert rc == _capi.GD_ERR_INVALID
    assert re.search(match, _capi.lib().gd_last_error().decode()), _capi.lib().gd_last_error()


def test_gd_live_rows_refuses_bad_arguments():
    L = _capi.lib()
    good = dict(mask=OK4 + 1, n=70, rows=OK4, count=OK8, scratch=OK16)  # (a mask may start at any byte)
    call = lambda **kw: L.gd_live_rows(*{**good, **kw}.values(), None)  # noqa: E731
    for name in ("mask", "rows", "count", "scratch"):
        _refused(call(**{name: None}), "gd_live_rows: .*(null|required)")
    for name in ("rows", "count", "scratch"):
        _refused(call(**{name: ODD}), "gd_live_rows: .*aligned")
    for n in (0, -1, (1 << 20) + 1):
        _refused(call(n=n), r"gd_live_rows: n must be in \[1, 2\^20\]")


def _policy_struct(n=70, A=64, ew=6, na=91):
    p = _capi.GdPolicy()
    p.num_rows, p.max_agents, p.ego_width, p.n_actions = n, A, ew, na
    p.blob, p.features, p.logits = OK16, OK16 + 0x1000, OK16 + 0x2000
    p.blob_floats = 0  # (set below: the layout's size is the library's to say)
    return p


def test_gd_policy_forward_rows_refuses_bad_arguments():
    L = _capi.lib()
    p = _policy_struct()
    good = dict(obs=OK4, u=OK4, deterministic=0, actions=OK8, logprob=OK4, entropy=OK4, value=OK4, logits_out=None, rows=OK4,
                count=OK4)
    call = lambda d=None, **kw: L.gd_policy_forward_rows(ctypes.byref(p), d, *{**good, **kw}.values(), None)  # noqa: E731
    _refused(call(), "gd_policy_forward_rows: blob_floats")  # whatever gd_policy_forward refuses, first
    # the layout's size, from the refusals themselves: the only value the check lets through
    from gpudrive_lab_amd.policy import pack_index
    p.blob_floats = len(pack_index(6, 91))
    for name in ("rows", "count"):
        _refused(call(**{name: None}), "gd_policy_forward_rows: rows and count are required")
        _refused(call(**{name: ODD}), "gd_policy_forward_rows: rows and count must be 4-byte aligned")
    _refused(call(obs=None), "gd_policy_forward_rows: null")
    _refused(call(u=None), "gd_policy_forward_rows: null")
    _refused(call(actions=OK4 + 4), "gd_policy_forward_rows: .*aligned")
    _refused(call(logits_out=ODD), "gd_policy_forward_rows: .*aligned")
    d = _capi.GdDropout(seed=1, call=None, used=OK8, threshold=100, scale=1.0)
    _refused(call(ctypes.byref(d)), "gd_policy_forward_rows: dropout")
    d = _capi.GdDropout(seed=1, call=OK8, used=OK8, threshold=0, scale=1.0)
    _refused(call(ctypes.byref(d)), "gd_policy_forward_rows: dropout: threshold")
    p.num_rows = 0
    _refused(call(), "gd_policy_forward_rows: num_rows")


def test_gd_policy_rollout_compact_refuses_a_bad_row_list_before_the_simulator_is_read():
    """The row list is checked before anything else: the simulator here is 4 KiB of zeros that no check may read."""
    L = _capi.lib()
    sim = ctypes.create_string_buffer(4096)
    p, b = _policy_struct(), _capi.GdPolicyRolloutBuffers()
    good = dict(rows=OK4, count=OK4, scratch=OK4, live_count=None, reserved=0)

    def call(sim=sim, pp=ctypes.byref(p), bb=ctypes.byref(b), rr=True, **kw):
        r = _capi.GdPolicyRolloutRows(**{**good, **kw})
        return L.gd_policy_rollout_compact(sim, pp, bb, ctypes.byref(r) if rr else None, 91)

    for kw in (dict(sim=None), dict(pp=None), dict(bb=None), dict(rr=False)):
        _refused(call(**kw), "gd_policy_rollout_compact: null argument")
    for name in ("rows", "count", "scratch"):
        _refused(call(**{name: None}), "gd_policy_rollout_compact: .*required")
        _refused(call(**{name: ODD}), "gd_policy_rollout_compact: .*aligned")
    _refused(call(live_count=ODD), "gd_policy_rollout_compact: live_count must be 4-byte aligned")
    _refused(call(reserved=1), "gd_policy_rollout_compact: the row list's reserved must be 0")
    _refused(call(reserved=-1), "gd_policy_rollout_compact: the row list's reserved must be 0")
    assert sim.raw == bytes(4096)


# ---- Python
def test_live_rows_refuses_a_bad_mask_before_any_device_call():
    from gpudrive_lab_amd.policy import LiveRows, live_rows
    for mask in (None, [1, 0], torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.bool),
                 torch.zeros(8, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError, match="mask must be a contiguous bool or uint8"):
            live_rows(mask)
    with pytest.raises(ValueError, match="N must be in"):
        live_rows(torch.zeros(0, dtype=torch.bool))
    with pytest.raises(ValueError, match="N must be in"):
        live_rows(torch.zeros((1 << 20) + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="on the GPU"):
        live_rows(torch.zeros(4, dtype=torch.bool))
    for n in (0, (1 << 20) + 1, 4.0, True, None):
        with pytest.raises(ValueError, match="LiveRows: N"):
            LiveRows(n, "cpu")
    lr = LiveRows(1025, "cpu")
    assert lr.rows.dtype == lr.count.dtype == lr.scratch.dtype == torch.int32
    assert (tuple(lr.rows.shape), tuple(lr.count.shape), tuple(lr.scratch.shape)) == ((1025,), (1,), (2,)) and int(lr.count) == 0
    assert LiveRows.nbytes(1025) == 4 * (1025 + 1 + 2) and LiveRows.nbytes(1024) == 4 * (1024 + 1 + 1)
    assert LiveRows.nbytes(1 << 20) == 4 * ((1 << 20) + 1 + 1024)


def test_the_policy_refuses_bad_rows_before_any_device_call():
    """A stub policy that owns nothing on a device: a bad rows= is refused before obs (here on the host) is looked at."""
    from gpudrive_lab_amd.policy import LiveRows, obs_width
    pol = _stub_policy()
    pol.obs_width = obs_width(64, 6)
    obs = torch.zeros(5, pol.obs_width)
    for rows in ("rows", 5, torch.zeros(5, dtype=torch.int32), (torch.zeros(5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(ValueError, match="rows must be a LiveRows of N = 5"):
            pol(obs, deterministic=True, rows=rows)
    for n in (4, 6):
        with pytest.raises(ValueError, match="rows must be a LiveRows of N = 5.*one of N = %d" % n):
            pol(obs, deterministic=True, rows=LiveRows(n, "cpu"))


def test_run_checks_its_arguments_before_compact_matters():
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO
    loop = object.__new__(ClosedLoopPPO)  # (no simulator, no policy: anything run() touched would raise AttributeError)
    with pytest.raises(ValueError, match="n_steps"):
        loop.run(n_steps=0, deterministic=True, compact=True)
    with pytest.raises(ValueError, match="generator"):
        loop.run(compact=True)
    with pytest.raises(ValueError, match="State"):
        ClosedLoopPPO.nbytes(_StubSim(3), _stub_policy(), compact=True)


def test_nbytes_compact_adds_the_four_new_arrays():
    import types
    from gpudrive_lab_amd.ppo_rollout import ClosedLoopPPO

    class Counted(_StubSim):
        def __init__(self, model, n, **kw):
            super().__init__(model, **kw)
            self.__dict__["n"] = n

        def controlled_state_tensor(self):
            t = torch.zeros(self._W * self._A, 1, dtype=torch.int32)
            t[:self.n] = 1
            return types.SimpleNamespace(to_torch=lambda: t.view(self._W, self._A, 1))

    pol = _stub_policy()
    for n, W in ((6, 3), (1024, 20), (1025, 20)):
        sim = Counted(0, n, W=W)
        new = 4 * n + 4 * 1 + 4 * -(-n // 1024) + 4 * 91  # rows, count, scratch, live_count
        for kw in (dict(), dict(record=True), dict(stochastic=True)):
            assert ClosedLoopPPO.nbytes(sim, pol, compact=True, **kw) - ClosedLoopPPO.nbytes(sim, pol, **kw) == new, (n, kw)
        assert ClosedLoopPPO.nbytes(sim, pol, compact=False) == ClosedLoopPPO.nbytes(sim, pol)
