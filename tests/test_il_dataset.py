"""CPU tests of the device expert dataset (gd_il_index / gd_il_batch, gpudrive_lab_amd.il_dataset): the yardstick of the GPU
suite (the numpy rule of tests/il_cases.py) against the reference's own ExpertDataset as recorded in
tests/golden/il_dataset_golden.npz, the C surface, and everything the Python layer decides without a device."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import il_cases
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "il_dataset_golden.npz")


# ---- the yardstick is the reference's rule ----
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def case128():
    return il_cases.make_case(128)


def test_the_golden_is_small_and_covers_the_windows(golden):
    assert os.path.getsize(GOLDEN) <= 64 * 1024
    assert [tuple(w) for w in golden["windows"].tolist()] == il_cases.WINDOWS
    assert len(golden["cols"]) == 24 and {0, 5, 6, il_cases.width(128) - 4, il_cases.width(128) - 1} <= set(golden["cols"].tolist())


@pytest.mark.parametrize("R,P", il_cases.WINDOWS)
def test_the_numpy_rule_equals_the_reference_dataset(golden, case128, R, P):
    key = "r%d_p%d_" % (R, P)
    vi, rows = il_cases.index(case128, R, P)
    assert np.array_equal(vi, golden[key + "valid_indices"].astype(np.int64))
    assert len(vi) > 0 and (rows != vi[:, 0]).any()  # the dropped row moved idx1 away from the source row
    pos = golden[key + "pos"]
    obs, actions, partner, road, data_idx = il_cases.batch(case128, R, P, pos, cols=golden["cols"])
    assert np.array_equal(obs, golden[key + "obs"])
    assert np.array_equal(actions, golden[key + "actions"])
    assert np.array_equal(np.packbits(partner, axis=-1), golden[key + "partner_mask"])
    assert np.array_equal(np.packbits(road, axis=-1), golden[key + "road_mask"])
    assert np.array_equal(data_idx, golden[key + "data_idx"])
    if R > 1:
        assert (obs[:, 0] == 0).all(axis=1).any(), "no golden sample crosses t = 0"


def test_the_case_holds_what_the_rule_must_decide(case128):
    v = il_cases.valid_steps(case128)
    assert v[0, [10, 12, 20, 22, 30, 32, 50, 51, 52]].all()      # a threshold hit exactly and a NaN stay valid
    assert not v[0, [11, 13, 21, 23, 31, 33]].any()             # one ulp beyond is not
    assert not v[5, [0, 63, 64, 66, 89, 90]].any() and v[5, [1, 62, 65, 88]].all()
    assert not v[il_cases.DEAD_ALWAYS].any() and not v[il_cases.DEAD_FROM_40, 40:].any() and v[il_cases.DEAD_FROM_40, :40].all()
    assert not v[il_cases.DEAD_FIRST_7, :7].any() and v[il_cases.DEAD_FIRST_7, 7:].all()
    assert case128["keep"].tolist() == [True, False, True, True, True, True, True]
    assert int(case128["obs"].max()) < 1 << 24  # every value exact in fp32
    a, b = il_cases.make_case(64), case128
    assert a["obs"].shape == (7, 91, 2984) and b["obs"].shape == (7, 91, 3368) and a["partner_mask"].shape == (7, 91, 63)
    # the byte phases of the partner mask spans the GPU suite relies on: 127 = 63 = 3 (mod 4), so R = 4 is needed for phase 0
    assert {R * 127 % 4 for R in (1, 2, 3, 4, 5)} == {R * 63 % 4 for R in (1, 2, 3, 4, 5)} == {0, 1, 2, 3}
    # out-of-range positions give the all-padding sample
    obs, actions, partner, road, data_idx = il_cases.batch(a, 3, 2, [-1, 0, 10 ** 6])
    assert not obs[[0, 2]].any() and not actions[[0, 2]].any() and partner[[0, 2]].all() and road[[0, 2]].all()
    assert data_idx.tolist() == [[-1, -1], [0, 0], [-1, -1]] and obs[1, 2].any() and not obs[1, :2].any()


# ---- the C surface ----
def test_the_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
    assert ("int gd_il_index(const gd_il_dataset *ds, int32_t *counts, int32_t *kept, const int64_t *entry_offset,\n"
            "                const int64_t *kept_ordinal, int32_t *entries, void *stream);") in header
    assert "int gd_il_batch(const gd_il_dataset *ds, const gd_il_batch_buffers *buffers, void *stream);" in header
    assert "#define GD_IL_MAX_SHARDS 8" in header and "dataloader.py:5-71, 183-211" in header
    assert {"gd_il_index", "gd_il_batch"} <= set(_capi.SYMBOLS)
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert {"gd_il_index", "gd_il_batch"} <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    assert len(L.gd_il_index.argtypes) == 7 and L.gd_il_index.argtypes[0]._type_ is _capi.GdIlDataset
    assert len(L.gd_il_batch.argtypes) == 3 and L.gd_il_batch.argtypes[1]._type_ is _capi.GdIlBatchBuffers
    # the C structs' layouts
    S, Dt, B = _capi.GdIlShard, _capi.GdIlDataset, _capi.GdIlBatchBuffers
    assert [f[0] for f in S._fields_] == ["obs", "actions", "dead_mask", "partner_mask", "road_mask", "keep", "n_rows"]
    assert ctypes.sizeof(S) == 56 and S.n_rows.offset == 48
    assert ctypes.sizeof(Dt) == 8 * 56 + 16 and Dt.n_shards.offset == 448 and Dt.pred_len.offset == 460
    assert [f[0] for f in B._fields_] == ["entries", "n_entries", "sel", "batch", "bad_indices", "obs", "actions",
                                          "partner_mask", "road_mask", "data_idx"]
    assert ctypes.sizeof(B) == 80 and B.bad_indices.offset == 32 and B.data_idx.offset == 72


def _table(**kw):
    d = _capi.GdIlDataset()
    d.n_shards, d.max_agents, d.rollout_len, d.pred_len = 1, 128, 5, 1
    for k in ("obs", "actions", "dead_mask", "partner_mask", "road_mask", "keep"):
        setattr(d.shard[0], k, 4096)  # (never dereferenced: every call below is refused on the host)
    d.shard[0].n_rows = 1
    for k, v in kw.items():
        if k in ("n_rows", "obs", "road_mask", "keep"):
            setattr(d.shard[0], k, v)
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad", [dict(rollout_len=0), dict(pred_len=0), dict(rollout_len=90, pred_len=2), dict(max_agents=96),
                                 dict(n_shards=9), dict(n_shards=-1), dict(n_rows=-1), dict(keep=None), dict(obs=4104),
                                 dict(road_mask=4100)])
def test_the_entry_points_refuse_a_bad_table_on_the_host(bad):
    L = _capi.lib()
    d = _table(**bad)
    assert L.gd_il_index(ctypes.byref(d), 4096, 4096, None, None, None, None) == _capi.GD_ERR_INVALID
    assert b"gd_il_index" in L.gd_last_error()
    b = _capi.GdIlBatchBuffers()
    assert L.gd_il_batch(ctypes.byref(d), ctypes.byref(b), None) == _capi.GD_ERR_INVALID
    assert b"gd_il_batch" in L.gd_last_error()


def test_the_entry_points_refuse_null_and_negative_arguments_on_the_host():
    L = _capi.lib()
    d = _table()
    assert L.gd_il_index(None, 4096, 4096, None, None, None, None) == _capi.GD_ERR_INVALID
    assert L.gd_il_index(ctypes.byref(d), None, 4096, None, None, None, None) == _capi.GD_ERR_INVALID
    assert L.gd_il_index(ctypes.byref(d), None, None, None, 4096, 4096, None) == _capi.GD_ERR_INVALID  # no entry_offset
    assert L.gd_il_batch(ctypes.byref(d), None, None) == _capi.GD_ERR_INVALID

    def buffers(**kw):
        b = _capi.GdIlBatchBuffers()
        for k in ("entries", "sel", "bad_indices", "obs", "actions", "partner_mask", "road_mask", "data_idx"):
            setattr(b, k, 4096)
        b.n_entries, b.batch = 4, 2
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    for kw in (dict(batch=-1), dict(batch=1 << 25), dict(n_entries=-1), dict(sel=None), dict(bad_indices=None), dict(data_idx=None), dict(obs=4104),
               dict(road_mask=4100), dict(entries=4104)):
        assert L.gd_il_batch(ctypes.byref(d), ctypes.byref(buffers(**kw)), None) == _capi.GD_ERR_INVALID, kw


def test_integration_notes_name_the_entry_points():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gd_il_index" in text and "gd_il_batch" in text


# ---- the Python layer's checks: all before a device is touched ----
def _shard(n=2, A=128, **kw):
    """Host tensors of the right shapes: nothing below may get as far as asking for a device."""
    D = il_cases.width(A)
    t = dict(obs=torch.zeros(n, 91, D), actions=torch.zeros(n, 91, 3), dead_mask=torch.zeros(n, 91, dtype=torch.bool),
             partner_mask=torch.zeros(n, 91, A - 1, dtype=torch.uint8), road_mask=torch.zeros(n, 91, 200, dtype=torch.bool),
             keep=torch.ones(n, dtype=torch.bool))
    t.update(kw)
    return t


@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)


@pytest.mark.parametrize("R,P", [(0, 1), (1, 0), (-1, 5), (91, 1), (1, 91), (46, 46), (5.0, 1), (True, 1)])
def test_window_out_of_range_is_refused(no_library, R, P):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    with pytest.raises(ValueError, match="rollout_len"):
        DeviceExpertDataset(_shard(), rollout_len=R, pred_len=P)
    from gpudrive_lab_amd.recorder import ExpertEpisode
    ep = types.SimpleNamespace(**_shard())
    with pytest.raises(ValueError, match="rollout_len"):
        ExpertEpisode.dataset(ep, rollout_len=R, pred_len=P)


@pytest.mark.parametrize("what,bad", [
    ("tensor", dict(obs=np.zeros((2, 91, 3368), np.float32))),
    ("tensor", dict(keep=None)),
    ("float32", dict(obs=torch.zeros(2, 91, 3368, dtype=torch.float64))),
    ("float32", dict(actions=torch.zeros(2, 91, 3, dtype=torch.float16))),
    ("uint8", dict(partner_mask=torch.zeros(2, 91, 127, dtype=torch.int64))),
    ("bool", dict(road_mask=torch.zeros(2, 91, 200, dtype=torch.uint8))),
    ("bool", dict(dead_mask=torch.zeros(2, 91, dtype=torch.uint8))),
    ("bool", dict(keep=torch.ones(2))),
    (r"\[N, 91, D\]", dict(obs=torch.zeros(2, 90, 3368))),
    (r"\[N, 91, D\]", dict(obs=torch.zeros(2, 91, 3367))),
    (r"\[N, 91, D\]", dict(obs=torch.zeros(2 * 91, 3368))),
    ("actions", dict(actions=torch.zeros(2, 91, 10))),
    ("partner_mask", dict(partner_mask=torch.zeros(2, 91, 63, dtype=torch.uint8))),
    ("road_mask", dict(road_mask=torch.zeros(2, 91, 199, dtype=torch.bool))),
    ("dead_mask", dict(dead_mask=torch.zeros(3, 91, dtype=torch.bool))),
    ("keep", dict(keep=torch.ones(3, dtype=torch.bool))),
    ("contiguous", dict(actions=torch.zeros(2, 3, 91).transpose(1, 2))),
    ("is on", dict(actions=torch.zeros(2, 91, 3, device="meta"))),
])
def test_a_bad_shard_is_refused(no_library, what, bad):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    with pytest.raises(ValueError, match=what):
        DeviceExpertDataset(_shard(**bad))
    with pytest.raises(ValueError, match="shard 1"):
        DeviceExpertDataset([_shard(), _shard(**bad)])


def test_shards_that_disagree_or_are_too_many_are_refused(no_library):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    with pytest.raises(ValueError, match="agent slot counts"):
        DeviceExpertDataset([_shard(A=128), _shard(A=64)])
    with pytest.raises(ValueError, match="at most 8"):
        DeviceExpertDataset([_shard(n=1)] * 9)
    with pytest.raises(ValueError, match="no episode"):
        DeviceExpertDataset([])
    meta = {k: v.to("meta") for k, v in _shard().items()}
    with pytest.raises(ValueError, match="different devices"):
        DeviceExpertDataset([_shard(), meta])
    with pytest.raises(ValueError, match="no host path"):  # the last check: host tensors that are otherwise in order
        DeviceExpertDataset([_shard(), _shard(n=0)])


# ---- batches(): the index bookkeeping ----
def test_batch_selections_cover_the_permutation_in_order():
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    order = torch.tensor([7, 2, 9, 0, 4, 1, 8, 3, 6, 5])
    runs = [s.tolist() for s in DeviceExpertDataset.batch_selections(order, 4)]
    assert runs == [[7, 2, 9, 0], [4, 1, 8, 3], [6, 5]]  # a short last batch
    runs = [s.tolist() for s in DeviceExpertDataset.batch_selections(order, 4, drop_last=True)]
    assert runs == [[7, 2, 9, 0], [4, 1, 8, 3]]
    assert [s.tolist() for s in DeviceExpertDataset.batch_selections(order, 5, drop_last=True)] == [[7, 2, 9, 0, 4], [1, 8, 3, 6, 5]]
    assert [s.tolist() for s in DeviceExpertDataset.batch_selections(order, 10)] == [order.tolist()]
    assert [s.tolist() for s in DeviceExpertDataset.batch_selections(order, 11)] == [order.tolist()]
    assert list(DeviceExpertDataset.batch_selections(order, 11, drop_last=True)) == []
    assert list(DeviceExpertDataset.batch_selections(order[:0], 4)) == []
    for s in DeviceExpertDataset.batch_selections(order, 3):
        assert s.is_contiguous() and s.dtype == torch.int64  # what batch() takes as it is
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="batch_size"):
            list(DeviceExpertDataset.batch_selections(order, bad))
