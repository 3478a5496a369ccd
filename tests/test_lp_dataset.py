"""CPU tests of the device linear-probing dataset (gd_il_future_batch, gpudrive_lab_amd.il_dataset.DeviceFutureDataset): the
yardstick of the GPU suite (the numpy rule of tests/lp_cases.py) against the reference's own FutureDataset as recorded in
tests/golden/lp_dataset_golden.npz, the C surface, and everything the Python layer decides without a device."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import il_cases, lp_cases
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "lp_dataset_golden.npz")
A = 128


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def case():
    return lp_cases.make_case(A)


def check_labels(got, want, near, exact_rows, what):
    """Labels equal the rule; off the rows that must be exact one may differ where the float64 value lies within 1e-6 of a
    bin edge, and at most 1 in 1000 may.  got, want, near: [rows, ...] arrays, exact_rows: a bool per row."""
    diff = got != want
    print("%s: %d of %d labels differ, %d of them near an edge" % (what, diff.sum(), diff.size, (diff & near).sum()))
    assert not diff[exact_rows].any(), what
    assert not (diff & ~near).any(), what
    assert diff.sum() * 1000 <= diff.size, what


# ---- the yardstick is the reference's rule ----
def test_the_golden_is_small_and_covers_the_cases(golden):
    assert os.path.getsize(GOLDEN) <= 100 * 1024
    assert tuple(golden["future_steps"]) == lp_cases.FUTURE_STEPS == (1, 35, 90) and tuple(golden["ego_steps"]) == (1, 5, 35, 90)
    assert np.array_equal(golden["ego_range"], np.array(lp_cases.EGO_RANGE))
    assert golden["other_f1_pos"].shape == (6, 91, 127) and golden["ego_f1_pos"].shape == (6, 91)
    assert 8 <= len(golden["items_other_pos"]) <= 10


def test_the_case_holds_what_the_rule_must_decide(case):
    keep, valid = case["keep"], il_cases.valid_steps(case)
    assert np.abs(case["obs"][:, :, 7:6 + 6 * 127:6]).max() < 0.08 and np.abs(case["obs"][:, :, 8:6 + 6 * 127:6]).max() < 0.08
    mask, lab = lp_cases.labels(case, 1, "other")
    assert len(np.unique(lab[keep][~mask[keep]])) == 64  # every class among the unmasked labels at F = 1
    fvm, lab = lp_cases.labels(case, 35, "ego")
    assert len(np.unique(lab[keep][fvm[keep]])) >= 8
    for F in (1, 5, 35, 90):
        fvm, lab = lp_cases.labels(case, F, "ego")
        assert (lab[lp_cases.STATIONARY_ROW] == 36).all()  # d = 0: the class of norm(0) twice, whatever cos returns
        assert (lab[:, 91 - F:] == 36).all() and not fvm[:, 91 - F:].any()  # the raw pair (0, 0) past the episode's end
    rot = case["ego_global_rot"]
    assert (rot[lp_cases.EDGE_ROW] == 0).all() and np.abs(rot[lp_cases.PI_ROW]).max() > np.pi > np.abs(rot[lp_cases.PI_ROW]).min()
    assert rot[5].max() < -3.0 and rot[5].min() < -np.pi
    # the edge row at F = 1: every displacement is +-(k * 12.5) or one of its fp32 neighbours, on both sides of every edge
    d = np.diff(case["ego_global_pos"][lp_cases.EDGE_ROW], axis=0)
    e = (np.arange(-4, 5) * 12.5).astype(np.float32)
    three = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])
    assert np.isin(np.abs(d), np.abs(three)).all() and len(np.unique(d[:, 0])) >= 27
    assert len(np.unique(lp_cases.labels(case, 1, "ego")[1][lp_cases.EDGE_ROW])) >= 16
    assert np.isnan(case["ego_global_pos"][lp_cases.NAN_ROW, lp_cases.NAN_TIME, 0])
    fvm, lab = lp_cases.labels(case, 5, "ego")
    assert lab[lp_cases.NAN_ROW, lp_cases.NAN_TIME] // 8 == 7 and lab[lp_cases.NAN_ROW, lp_cases.NAN_TIME - 5] // 8 == 7  # digitize's NaN
    assert fvm[lp_cases.NAN_ROW, lp_cases.NAN_TIME]  # (a NaN position does not invalidate the step)
    # future_valid_mask sees an invalid step on either side
    fvm, _ = lp_cases.labels(case, 35, "ego")
    r = il_cases.DEAD_FROM_40
    assert fvm[r, 4] and not fvm[r, 5] and valid[r, 5] and not valid[r, 40]  # idx2 + F = 39 | 40
    r = il_cases.DEAD_FIRST_7
    assert not fvm[r, 6] and fvm[r, 7] and valid[r, 41]
    assert not valid[5, 63] and not fvm[5, 63] and not fvm[5, 63 - 35] and fvm[5, 62 - 35]
    # the two switching partner columns of the edge row: 0 then 2 and 2 then 0 across a future step
    pm, s = case["partner_mask"][lp_cases.EDGE_ROW], lp_cases.SWITCH_TIME
    aux, _ = lp_cases.labels(case, 35, "other")
    for col in (lp_cases.OFF_THEN_ON, lp_cases.ON_THEN_OFF):
        assert {int(pm[s - 1, col]), int(pm[s, col])} == {0, 2}
        assert aux[lp_cases.EDGE_ROW, s - 35:s, col].all()  # one end masked is enough
    assert not aux[lp_cases.EDGE_ROW, :s - 35, lp_cases.OFF_THEN_ON].any() and not aux[lp_cases.EDGE_ROW, s:56, lp_cases.ON_THEN_OFF].any()
    # positions outside the index
    out = lp_cases.batch(case, 3, 2, 35, "other", [-1, 0, 10 ** 6])
    assert not out[2][[0, 2]].any() and not out[3][[0, 2]].any() and out[6][[0, 2]].all() and (out[7][[0, 2]] == 36).all()
    out = lp_cases.batch(case, 3, 2, 35, "ego", [-1, 0, 10 ** 6], lp_cases.EGO_RANGE)
    assert not out[6][[0, 2]].any() and out[7][[0, 2]].tolist() == [lp_cases.label(0.0, 0.0, lp_cases.EGO_RANGE)] * 2 != [36, 36]
    assert out[2][1] and out[3][1].tolist() == [False, False, True]


def test_the_numpy_rule_equals_the_reference_on_every_row_and_time(golden, case):
    keep = case["keep"]
    exact = np.isin(np.nonzero(keep)[0], (lp_cases.STATIONARY_ROW, lp_cases.EDGE_ROW))
    for F in lp_cases.FUTURE_STEPS:
        mask, lab = lp_cases.labels(case, F, "other")
        assert np.array_equal(np.packbits(mask[keep], axis=-1), golden["other_f%d_mask" % F])
        assert not mask[keep].all()
        check_labels(lab[keep], golden["other_f%d_pos" % F].astype(np.int64), lp_cases.near_edge(case, F, "other")[keep], exact,
                     "other F=%d" % F)
    for F in (1, 5, 35, 90):
        mask, lab = lp_cases.labels(case, F, "ego")
        assert np.array_equal(mask[keep], golden["ego_f%d_mask" % F]) and mask[keep].any()
        check_labels(lab[keep], golden["ego_f%d_pos" % F].astype(np.int64), lp_cases.near_edge(case, F, "ego")[keep], exact,
                     "ego F=%d" % F)
    mask, lab = lp_cases.labels(case, 35, "ego", lp_cases.EGO_RANGE)
    assert np.array_equal(mask[keep], golden["ego_range_mask"])
    check_labels(lab[keep], golden["ego_range_pos"].astype(np.int64), lp_cases.near_edge(case, 35, "ego", lp_cases.EGO_RANGE)[keep],
                 exact, "ego with xy_range")
    assert not np.array_equal(golden["ego_range_pos"], golden["ego_f35_pos"])


@pytest.mark.parametrize("exp", ["other", "ego"])
def test_the_rule_gives_the_reference_items_in_order_shape_and_dtype(golden, case, exp):
    R, P, F = (int(v) for v in golden["window"])
    key = "items_%s_" % exp
    pos = golden[key + "pos"]
    out = lp_cases.batch(case, R, P, F, exp, pos, cols=golden["cols"])
    obs, actions, valid_mask, ego_mask, partner, road, fmask, fpos = out
    assert np.array_equal(obs, golden[key + "obs"]) and np.array_equal(actions, golden[key + "actions"])
    assert np.array_equal(valid_mask, golden[key + "valid_mask"]) and valid_mask.all()
    assert np.array_equal(ego_mask, golden[key + "ego_mask"]) and not ego_mask.all()
    assert np.array_equal(np.packbits(partner, axis=-1), golden[key + "partner_mask"])
    assert np.array_equal(np.packbits(road, axis=-1), golden[key + "road_mask"])
    assert np.array_equal(fmask, golden[key + "future_mask"]) and fmask.any() and not fmask.all()
    vi, rows = il_cases.index(case, R, P)
    near = lp_cases.near_edge(case, F, exp)[rows[pos], vi[pos, 1]]
    check_labels(fpos, golden[key + "future_pos"].astype(np.int64), near, np.isin(rows[pos], (lp_cases.STATIONARY_ROW, lp_cases.EDGE_ROW)),
                 "items " + exp)
    # the reference's own element shapes (one sample) and dtype kinds: ours are those with the batch in front
    want_shapes = [s[1:] for s in (o.shape for o in out)]
    want_shapes[0] = (R, il_cases.width(A))
    assert str(want_shapes) == str(golden[key + "shapes"][0])
    assert "".join(o.dtype.kind for o in (obs.view(np.float32), actions.view(np.float32)) + out[2:]) == str(golden[key + "kinds"][0])


# ---- the C surface ----
def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert ("int gd_il_future_batch(const gd_il_dataset *ds, const gd_il_future *future, const gd_il_future_buffers *buffers, "
            "void *stream);") in header
    assert "linear_probing/dataloader.py" in header and "gd_il_future_batch" in _capi.SYMBOLS
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "gd_il_future_batch" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert [a._type_ for a in L.gd_il_future_batch.argtypes[:3]] == [_capi.GdIlDataset, _capi.GdIlFuture, _capi.GdIlFutureBuffers]
    assert len(L.gd_il_future_batch.argtypes) == 4
    # the C structs' layouts against the header's declarations: the same fields in the same order, LP64 sizes
    for name, S, size in (("gd_il_future", _capi.GdIlFuture, 16 * 8 + 8 + 18 * 8), ("gd_il_future_buffers", _capi.GdIlFutureBuffers, 13 * 8)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [m for stmt in body.split(";") for m in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", stmt.strip())]
        assert declared == [f[0] for f in S._fields_], (declared, name)
        assert ctypes.sizeof(S) == size
    F, B = _capi.GdIlFuture, _capi.GdIlFutureBuffers
    assert F.ego_global_rot.offset == 64 and F.future_step.offset == 128 and F.exp.offset == 132 and F.xbins.offset == 136
    assert F.ybins.offset == 208 and B.bad_indices.offset == 32 and B.obs.offset == 40 and B.future_pos.offset == 96
    assert (_capi.IL_FUTURE_OTHER, _capi.IL_FUTURE_EGO) == (0, 1) and "GD_IL_FUTURE_OTHER = 0" in header and "GD_IL_FUTURE_EGO = 1" in header
    # the existing structs keep their layout
    assert ctypes.sizeof(_capi.GdIlShard) == 56 and ctypes.sizeof(_capi.GdIlDataset) == 464 and ctypes.sizeof(_capi.GdIlBatchBuffers) == 80


def _table(**kw):
    d = _capi.GdIlDataset()
    d.n_shards, d.max_agents, d.rollout_len, d.pred_len = 1, 128, 5, 1
    for k in ("obs", "actions", "dead_mask", "partner_mask", "road_mask", "keep"):
        setattr(d.shard[0], k, 4096)  # (never dereferenced: every call below is refused on the host)
    d.shard[0].n_rows = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _future(**kw):
    f = _capi.GdIlFuture()
    f.ego_global_pos[0] = f.ego_global_rot[0] = 4096
    f.future_step, f.exp = 1, _capi.IL_FUTURE_OTHER
    f.xbins[:] = f.ybins[:] = np.linspace(-0.05, 0.05, 9).tolist()
    for k, v in kw.items():
        if k in ("ego_global_pos", "ego_global_rot"):
            getattr(f, k)[0] = v
        elif k in ("xbins", "ybins"):
            getattr(f, k)[:] = v
        else:
            setattr(f, k, v)
    return f


def _buffers(**kw):
    b = _capi.GdIlFutureBuffers()
    for k, _ in _capi.GdIlFutureBuffers._fields_:
        if k not in ("n_entries", "batch"):
            setattr(b, k, 4096)
    b.n_entries, b.batch = 4, 2
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_the_entry_point_refuses_bad_arguments_on_the_host():
    L = _capi.lib()
    call = lambda d, f, b: L.gd_il_future_batch(ctypes.byref(d) if d else None, ctypes.byref(f) if f else None,
                                                ctypes.byref(b) if b else None, None)
    assert call(None, _future(), _buffers()) == _capi.GD_ERR_INVALID
    assert call(_table(), None, _buffers()) == _capi.GD_ERR_INVALID
    assert call(_table(), _future(), None) == _capi.GD_ERR_INVALID and b"gd_il_future_batch" in L.gd_last_error()
    for bad in (dict(rollout_len=0), dict(pred_len=91), dict(max_agents=96), dict(n_shards=9)):
        assert call(_table(**bad), _future(), _buffers()) == _capi.GD_ERR_INVALID, bad
    up = np.linspace(-0.05, 0.05, 9)
    flat, nan = up.copy(), up.copy()
    flat[4], nan[8] = flat[3], np.nan
    for bad in (dict(future_step=0), dict(future_step=91), dict(future_step=-1), dict(exp=2), dict(exp=-1),
                dict(ego_global_pos=None), dict(ego_global_rot=None), dict(xbins=up[::-1].tolist()), dict(ybins=flat.tolist()),
                dict(ybins=nan.tolist()), dict(xbins=[0.0] * 9)):
        assert call(_table(), _future(**bad), _buffers()) == _capi.GD_ERR_INVALID, bad
        assert b"gd_il_future_batch" in L.gd_last_error()
    for bad in (dict(batch=-1), dict(batch=1 << 25), dict(n_entries=-1), dict(sel=None), dict(bad_indices=None), dict(valid_mask=None),
                dict(ego_mask=None), dict(future_mask=None), dict(future_pos=None), dict(obs=4104), dict(road_mask=4100),
                dict(entries=4104), dict(future_pos=4100)):
        assert call(_table(), _future(), _buffers(**bad)) == _capi.GD_ERR_INVALID, bad


def test_the_documents_name_the_entry_point():
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "gd_il_future_batch" in text and "DeviceFutureDataset" in text, name


# ---- the Python layer's checks: all before a device is touched ----
def _shard(n=2, A=128, **kw):
    """Host tensors of the right shapes: nothing below may get as far as asking for a device."""
    D = il_cases.width(A)
    t = dict(obs=torch.zeros(n, 91, D), actions=torch.zeros(n, 91, 3), dead_mask=torch.zeros(n, 91, dtype=torch.bool),
             partner_mask=torch.zeros(n, 91, A - 1, dtype=torch.uint8), road_mask=torch.zeros(n, 91, 200, dtype=torch.bool),
             keep=torch.ones(n, dtype=torch.bool), ego_global_pos=torch.zeros(n, 91, 2), ego_global_rot=torch.zeros(n, 91, 1))
    t.update(kw)
    return t


@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)


@pytest.mark.parametrize("what,kw", [
    ("future_step", dict(future_step=0)), ("future_step", dict(future_step=91)), ("future_step", dict(future_step=1.0)),
    ("future_step", dict(future_step=True)), ("exp", dict(exp="partner")), ("exp", dict(exp=None)),
    ("xy_range", dict(exp="other", xy_range=lp_cases.EGO_RANGE)), ("xy_range", dict(xy_range=lp_cases.EGO_RANGE)),
    ("xy_range", dict(exp="ego", xy_range=((0.05, -0.05), (-0.05, 0.05)))), ("xy_range", dict(exp="ego", xy_range=((0.0, 0.0), (-1, 1)))),
    ("xy_range", dict(exp="ego", xy_range=((-1, 1), (-1, float("inf"))))), ("xy_range", dict(exp="ego", xy_range=((float("nan"), 1), (-1, 1)))),
    ("xy_range", dict(exp="ego", xy_range=(-1, 1))), ("xy_range", dict(exp="ego", xy_range=((-1, 1),))),
    ("rollout_len", dict(rollout_len=0)), ("rollout_len", dict(rollout_len=46, pred_len=46)),
])
def test_a_bad_argument_is_refused(no_library, what, kw):
    from gpudrive_lab_amd.il_dataset import DeviceFutureDataset
    from gpudrive_lab_amd.recorder import ExpertEpisode
    with pytest.raises(ValueError, match=what):
        DeviceFutureDataset(_shard(), **kw)
    with pytest.raises(ValueError, match=what):
        ExpertEpisode.future_dataset(types.SimpleNamespace(**_shard()), **kw)


@pytest.mark.parametrize("what,bad", [
    ("ego_global_pos must be a tensor", dict(ego_global_pos=None)),
    ("ego_global_rot must be a tensor", dict(ego_global_rot=np.zeros((2, 91, 1), np.float32))),
    ("float32", dict(ego_global_pos=torch.zeros(2, 91, 2, dtype=torch.float64))),
    ("ego_global_pos", dict(ego_global_pos=torch.zeros(2, 91, 3))),
    ("ego_global_pos", dict(ego_global_pos=torch.zeros(3, 91, 2))),
    ("ego_global_rot", dict(ego_global_rot=torch.zeros(2, 91))),
    ("contiguous", dict(ego_global_pos=torch.zeros(2, 2, 91).transpose(1, 2))),
    ("is on", dict(ego_global_rot=torch.zeros(2, 91, 1, device="meta"))),
    (r"\[N, 91, D\]", dict(obs=torch.zeros(2, 91, 3367))),
    ("partner_mask", dict(partner_mask=torch.zeros(2, 91, 63, dtype=torch.uint8))),
])
def test_a_bad_shard_is_refused(no_library, what, bad):
    from gpudrive_lab_amd.il_dataset import DeviceFutureDataset
    with pytest.raises(ValueError, match=what):
        DeviceFutureDataset(_shard(**bad), exp="ego")
    with pytest.raises(ValueError, match="DeviceFutureDataset: shard 1"):
        DeviceFutureDataset([_shard(), _shard(**bad)])


def test_shards_that_disagree_or_are_too_many_are_refused(no_library):
    from gpudrive_lab_amd.il_dataset import DeviceFutureDataset
    with pytest.raises(ValueError, match="at most 8"):
        DeviceFutureDataset([_shard(n=1)] * 9)
    with pytest.raises(ValueError, match="agent slot counts"):
        DeviceFutureDataset([_shard(A=128), _shard(A=64)])
    meta = {k: v.to("meta") for k, v in _shard().items()}
    with pytest.raises(ValueError, match="different devices"):
        DeviceFutureDataset([_shard(), meta])
    with pytest.raises(ValueError, match="no host path"):  # the last check: host tensors that are otherwise in order
        DeviceFutureDataset(_shard(), future_step=90, exp="ego", xy_range=lp_cases.EGO_RANGE)


def test_the_plain_dataset_does_not_ask_for_poses(no_library):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    t = _shard()
    del t["ego_global_pos"], t["ego_global_rot"]
    with pytest.raises(ValueError, match="no host path"):
        DeviceExpertDataset(t)
