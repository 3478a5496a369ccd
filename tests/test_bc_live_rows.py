"""CPU tests of the live-row BC forward (gd_bc_forward_rows, gd_bc_rollout_compact; DeviceBCPolicy(rows=),
ClosedLoopBC.run(compact=True)): the surface, the struct, the refusals -- every one before anything is launched or any
simulator touched -- and the byte count."""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

from gpudrive_lab_amd import _capi
from tests.conftest import ROOT
from tests.test_bc_rollout import _StubSim, _stub_policy

HEADER = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
NAMES = ("gd_bc_forward_rows", "gd_bc_rollout_compact")


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
    for name, n_args in zip(NAMES, (13, 5)):
        args = _declared_args(name)
        assert len(args) == n_args, (name, args)
        assert name in _capi.SYMBOLS and name in exported
        assert len(getattr(L, name).argtypes) == n_args, name
    # gd_bc_forward's eleven arguments, plus rows and count before the stream
    fwd = _declared_args("gd_bc_forward")
    assert _declared_args("gd_bc_forward_rows") == fwd[:-1] + ["const int32_t *rows", "const int32_t *count"] + fwd[-1:]
    at = L.gd_bc_forward_rows.argtypes
    assert at[0]._type_ is _capi.GdBCPolicy and at[9]._type_ is _capi.GdBCOutputs
    assert list(at[:9]) + list(at[10:11]) == list(L.gd_bc_forward.argtypes[:9]) + list(L.gd_bc_forward.argtypes[10:])
    # gd_bc_rollout's four arguments, with the list before n_steps
    ro = _declared_args("gd_bc_rollout")
    assert _declared_args("gd_bc_rollout_compact") == ro[:-1] + ["const gd_bc_rollout_rows *rows"] + ro[-1:]
    at = L.gd_bc_rollout_compact.argtypes
    assert at[1]._type_ is _capi.GdBCPolicy and at[2]._type_ is _capi.GdBCRolloutBuffers
    assert at[3]._type_ is _capi.GdBCRolloutRows


def test_the_struct_has_the_headers_fields():
    R = _capi.GdBCRolloutRows
    names = [f[0] for f in R._fields_]
    assert names == ["rows", "count", "scratch", "live_count", "reserved"]
    assert [getattr(R, n).offset for n in names] == [0, 8, 16, 24, 32] and ctypes.sizeof(R) == 40
    body = HEADER[HEADER.index("typedef struct gd_bc_rollout_rows {"):HEADER.index("} gd_bc_rollout_rows;")]
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"[ *](\w+)[,;]", code) == names, "the header declares other fields, or in another order"
    assert re.findall(r"(\w+) +\*?\w+;", code) == ["int32_t"] * 5


# ---- the C calls: every refusal comes before the first launch, so no pointer below is ever read (none points anywhere)
OK4, OK16, OK256, ODD = 0x10000, 0x30000, 0x50000, 0x40002  # aligned addresses of nothing, and one that is not 4-byte aligned


def _refused(rc, match, code=_capi.GD_ERR_INVALID):
    assert rc == code
    assert re.search(match, _capi.lib().gd_last_error().decode()), _capi.lib().gd_last_error()


def _policy_struct(A=64):
    from gpudrive_lab_amd.bc_policy import pack_index, scratch_floats
    p = _capi.GdBCPolicy()
    p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers, p.head_layers, p.n_components = A, 1, 1, 1, 0, 1
    p.clip_value, p.chunk_rows = -20.0, 4
    p.blob, p.blob_floats = OK16, len(pack_index(1, (1, 1), 0, 1))
    p.scratch, p.scratch_floats = OK256, scratch_floats(A, 4)
    return p


def test_gd_bc_forward_rows_refuses_bad_arguments():
    L = _capi.lib()
    p = _policy_struct()
    o = _capi.GdBCOutputs(actions=OK4)
    good = dict(obs=OK4, partner_mask=OK4 + 1, road_mask=OK4 + 3, n=11, deterministic=0, u=OK4, z=OK4, expert_actions=None,
                out=ctypes.byref(o), rows=OK4, count=OK4)
    call = lambda pp=ctypes.byref(p), **kw: L.gd_bc_forward_rows(pp, *{**good, **kw}.values(), None)  # noqa: E731
    for name in ("rows", "count"):
        _refused(call(**{name: None}), "gd_bc_forward_rows: rows and count are required")
        _refused(call(**{name: ODD}), "gd_bc_forward_rows: rows and count must be 4-byte aligned")
    # whatever gd_bc_forward refuses, under the new name
    for kw in (dict(pp=None), dict(obs=None), dict(partner_mask=None), dict(road_mask=None), dict(out=None)):
        _refused(call(**kw), "gd_bc_forward_rows: null argument")
    _refused(call(u=None), "gd_bc_forward_rows: u and z are required unless deterministic")
    _refused(call(z=None), "gd_bc_forward_rows: u and z are required unless deterministic")
    for n in (0, -1, (1 << 20) + 1):
        _refused(call(n=n), r"gd_bc_forward_rows: n must be in \[1, 2\^20\]")
    _refused(call(obs=ODD), "gd_bc_forward_rows: .*4-byte aligned")
    with_nll = _capi.GdBCOutputs(nll=OK4)
    _refused(call(out=ctypes.byref(with_nll)), "gd_bc_forward_rows: expert_actions is required with out->nll")
    odd_out = _capi.GdBCOutputs(component=ODD)
    _refused(call(out=ctypes.byref(odd_out)), "gd_bc_forward_rows: .*4-byte aligned")
    for field, value, match in (("max_agents", 96, "max_agents"), ("num_stack", 9, "num_stack"), ("chunk_rows", 0, "chunk_rows"),
                                ("blob_floats", 5, "blob_floats"), ("scratch_floats", 7, "scratch_floats"),
                                ("scratch", OK256 + 16, "256-byte aligned"), ("n_components", 17, "n_components")):
        bad = _policy_struct()
        setattr(bad, field, value)
        _refused(call(pp=ctypes.byref(bad)), "gd_bc_forward_rows: .*" + match)


def _buffers(**kw):
    b = _capi.GdBCRolloutBuffers()
    for name, _ in _capi.GdBCRolloutBuffers._fields_:
        if name not in ("n_rows", "deterministic", "u", "z", "actions", "dead_mask", "ego_global_pos", "ego_global_rot"):
            setattr(b, name, OK16)
    b.n_rows, b.deterministic = 11, 1
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_gd_bc_rollout_compact_refuses_bad_arguments_before_the_simulator_is_read():
    """The row list is checked before anything else, then what gd_bc_rollout checks before it looks at the simulator: the
    simulator here is 4 KiB of zeros that no check may read."""
    L = _capi.lib()
    sim = ctypes.create_string_buffer(4096)
    p, b = _policy_struct(), _buffers()
    good = dict(rows=OK4, count=OK4, scratch=OK4, live_count=None, reserved=0)

    def call(sim=sim, pp=ctypes.byref(p), bb=ctypes.byref(b), rr=True, n_steps=91, **kw):
        r = _capi.GdBCRolloutRows(**{**good, **kw})
        return L.gd_bc_rollout_compact(sim, pp, bb, ctypes.byref(r) if rr else None, n_steps)

    for kw in (dict(sim=None), dict(pp=None), dict(bb=None), dict(rr=False)):
        _refused(call(**kw), "gd_bc_rollout_compact: null argument")
    for name in ("rows", "count", "scratch"):
        _refused(call(**{name: None}), "gd_bc_rollout_compact: .*required")
        _refused(call(**{name: ODD}), "gd_bc_rollout_compact: .*aligned")
    _refused(call(live_count=ODD), "gd_bc_rollout_compact: live_count must be 4-byte aligned")
    _refused(call(reserved=1), "gd_bc_rollout_compact: the row list's reserved must be 0")
    _refused(call(reserved=-1), "gd_bc_rollout_compact: the row list's reserved must be 0")
    # gd_bc_rollout's own refusals, word for word under either name
    for fn, who in ((lambda **kw: L.gd_bc_rollout(sim, ctypes.byref(p), kw.get("bb", ctypes.byref(b)), kw.get("n_steps", 91)),
                     "gd_bc_rollout"), (call, "gd_bc_rollout_compact")):
        for name in ("row_slot", "row_of_slot", "window", "partner_mask", "road_mask", "partner_value", "row_actions", "dead",
                     "goal_achieved", "off_road", "veh_collision", "goal_step", "off_road_step", "init_goal_dist", "goal_dist",
                     "any_alive", "summary"):
            _refused(fn(bb=ctypes.byref(_buffers(**{name: None}))), who + ": every buffer but the per-step records is required")
        for n in (0, -1, (1 << 20) + 1):
            _refused(fn(bb=ctypes.byref(_buffers(n_rows=n))), who + r": n_rows must be in \[1, 2\^20\]")
        for n_steps in (0, -1, 92):
            _refused(fn(n_steps=n_steps), who + r": an episode has 91 steps, n_steps must be in \[1, 91\]")
    assert sim.raw == bytes(4096)


# ---- Python
def _forward_stub(A=64, R=1):
    """A DeviceBCPolicy that owns nothing on a device: `device` is the host, so host tensors pass the input checks and anything
    past the checks would fail on the missing library handle."""
    from gpudrive_lab_amd.bc_policy import obs_width
    pol = _stub_policy(A, R)
    pol.obs_width, pol.device, pol.n_components = obs_width(A), torch.device("cpu"), 2
    return pol


def test_the_policy_refuses_bad_rows_before_any_device_call():
    from gpudrive_lab_amd.policy import LiveRows
    A, R, B = 64, 1, 5
    pol = _forward_stub(A, R)
    obs = torch.zeros(B, R, pol.obs_width)
    pm, rm = torch.zeros(B, R, A - 1, dtype=torch.bool), torch.zeros(B, R, 200, dtype=torch.bool)
    actions = torch.zeros(B, 1, 3)
    for rows in ("rows", 5, torch.zeros(B, dtype=torch.int32), (torch.zeros(B, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(ValueError, match="rows must be a LiveRows"):
            pol(obs, pm, rm, deterministic=True, out=actions, rows=rows)
    for n in (4, 6):
        with pytest.raises(ValueError, match="rows must be a LiveRows of N = 5, got one of N = %d" % n):
            pol(obs, pm, rm, deterministic=True, out=actions, rows=LiveRows(n, "cpu"))
    lr = LiveRows(B, "cpu")
    with pytest.raises(ValueError, match="rows= needs out=.*actions"):
        pol(obs, pm, rm, deterministic=True, rows=lr)
    with pytest.raises(ValueError, match="rows= needs out=.*context"):
        pol.context(obs, pm, rm, rows=lr)
    with pytest.raises(ValueError, match="rows= needs out=.*means, covariances, weights"):
        pol.gmm_params(obs, pm, rm, rows=lr)
    with pytest.raises(ValueError, match="rows= needs out=.*nll"):
        pol.nll(obs, pm, rm, torch.zeros(B, 3), rows=lr)
    with pytest.raises(ValueError, match="rows= needs out=.*means"):
        pol.forward(obs, pm, rm, ("actions", "means"), out={"actions": actions}, rows=lr)
    # a list on another device than the policy's
    pol.device = torch.device("meta")
    with pytest.raises(ValueError, match="rows is on cpu, the policy on meta"):
        pol(obs.to("meta"), pm.to("meta"), rm.to("meta"), deterministic=True, out=actions.to("meta"), rows=lr)


def test_run_checks_its_arguments_before_compact_matters():
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    loop = object.__new__(ClosedLoopBC)  # (no simulator, no policy: anything run() touched would raise AttributeError)
    with pytest.raises(ValueError, match="n_steps"):
        loop.run(n_steps=0, compact=True)
    with pytest.raises(ValueError, match="generator"):
        loop.run(deterministic=False, compact=True)
    with pytest.raises(ValueError, match="State"):
        ClosedLoopBC.nbytes(_StubSim(3), _stub_policy(), compact=True)


def test_nbytes_compact_adds_the_four_new_arrays():
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC

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
            assert ClosedLoopBC.nbytes(sim, pol, compact=True, **kw) - ClosedLoopBC.nbytes(sim, pol, **kw) == new, (n, kw)
        assert ClosedLoopBC.nbytes(sim, pol, compact=False) == ClosedLoopBC.nbytes(sim, pol)
