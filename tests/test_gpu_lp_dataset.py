"""GPU suite: the device linear-probing dataset (gd_il_future_batch, gpudrive_lab_amd.il_dataset.DeviceFutureDataset) against
the numpy rule of tests/lp_cases.py, which tests/test_lp_dataset.py pins to the reference's own FutureDataset.  Synthetic
tensors only, no simulator.  The window, the targets and every mask are compared exactly (floats as int32, bools as bytes);
a label may differ from the rule only where the value recomputed in float64 lies within 1e-6 of a bin edge, at most 1 in 1000,
and nowhere on the stationary and the edge row."""
import functools

import numpy as np
import pytest
import torch

from tests import il_cases, lp_cases

pytestmark = pytest.mark.gpu

NAMES = ("obs", "actions", "valid_mask", "ego_mask", "partner_mask", "road_mask", "future_mask", "future_pos")
WINDOWS = [(5, 1), (1, 1), (10, 5), (1, 90)]
EXACT_ROWS = (lp_cases.STATIONARY_ROW, lp_cases.EDGE_ROW)
FRONT = 64  # guard bytes in front of and behind every carved output


@functools.lru_cache(maxsize=None)
def _case(A):
    return lp_cases.make_case(A)


@functools.lru_cache(maxsize=None)
def _shards(A, sizes):
    """The case on the device, cut into shards of the given row counts (shared by the tests; never written)."""
    return tuple({k: torch.from_numpy(v).cuda() for k, v in part.items()} for part in lp_cases.split(_case(A), sizes))


@functools.lru_cache(maxsize=None)
def _labels(A, F, exp, xy_range=None):
    return lp_cases.labels(_case(A), F, exp, xy_range)


@functools.lru_cache(maxsize=None)
def _near(A, F, exp, xy_range=None):
    return lp_cases.near_edge(_case(A), F, exp, xy_range)


@functools.lru_cache(maxsize=None)
def _index(A, R, P):
    return il_cases.index(_case(A), R, P)


def _dataset(A, R, P, F, exp, sizes=(il_cases.N_ROWS,), xy_range=None):
    from gpudrive_lab_amd.il_dataset import DeviceFutureDataset
    return DeviceFutureDataset(list(_shards(A, sizes)), rollout_len=R, pred_len=P, future_step=F, exp=exp, xy_range=xy_range)


def _want(A, R, P, F, exp, sel, xy_range=None):
    return lp_cases.batch(_case(A), R, P, F, exp, sel, xy_range, _all=_labels(A, F, exp, xy_range))


def _sel(A, R, P, F):
    """About 40 positions: the first and the last, repeats, windows that cross t = 0, idx2 + F on both sides of 91, the
    neighbours of the dead stretches, of the NaN and of the switching partner columns, the stationary and the edge row, and
    two positions outside the index."""
    vi, rows = _index(A, R, P)
    M = len(vi)
    times = {0, 1, R - 2, R - 1, 89 - F, 90 - F, 91 - F, 92 - F, 39 - F, 40 - F, 6, 7, lp_cases.NAN_TIME, lp_cases.NAN_TIME - F,
             lp_cases.SWITCH_TIME - 1, lp_cases.SWITCH_TIME - F, 91 - P}
    hit = np.nonzero(np.isin(vi[:, 1], sorted(times)))[0]
    hit = hit[np.linspace(0, len(hit) - 1, min(len(hit), 24)).astype(int)] if len(hit) else hit
    rows_hit = [np.nonzero(rows == r)[0] for r in EXACT_ROWS]
    extra = np.concatenate([h[np.linspace(0, len(h) - 1, min(len(h), 5)).astype(int)] for h in rows_hit if len(h)])
    return tuple(int(p) for p in [0, M - 1, -1, 0] + hit.tolist() + [M] + extra.tolist() + [M // 2, M // 2])


def _bytes(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _host(out):
    dts = [o.dtype for o in out]
    assert dts == [torch.float32, torch.float32] + [torch.bool] * 5 + [torch.int64], dts
    return tuple(_bytes(o).cpu().numpy() for o in out)


def _check(got, want, A, R, P, F, exp, sel, what, xy_range=None):
    """got: the eight outputs as bit patterns (bools as bytes, so that a byte nobody wrote is seen)."""
    vi, rows = _index(A, R, P)
    for i, (name, g, w) in enumerate(zip(NAMES, got, want)):
        if w.dtype == bool:
            w = w.astype(np.uint8)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if i == 7:
            break
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d elements differ, first at %s: %s vs %s"
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
    sel = np.asarray(sel, np.int64)
    ok = (sel >= 0) & (sel < len(vi))
    pos = np.where(ok, sel, 0)
    n, idx2 = rows[pos], vi[pos, 1]
    near = _near(A, F, exp, xy_range)[n, idx2] & (ok if exp == "ego" else ok[:, None])
    diff = got[7] != want[7]
    print("%s: %d of %d labels differ, %d of them near an edge" % (what, diff.sum(), diff.size, (diff & near).sum()))
    assert not diff[np.isin(n, EXACT_ROWS) | ~ok].any(), what
    assert not (diff & ~near).any(), (what, np.argwhere(diff & ~near)[:4].tolist())
    assert diff.sum() * 1000 <= diff.size, what


class _Carved:
    """The eight outputs carved out of buffers filled with 0xFF bytes, the future mask `lead` bytes past a 16-byte boundary."""

    def __init__(self, ds, B, lead):
        self.raw, self.out, self.span = [], [], []
        for name, (shape, dt) in zip(NAMES, ds.batch_shapes(B)):
            size = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            front = FRONT + (lead if name == "future_mask" else 0)
            raw = torch.full((front + size + FRONT + 3,), 0xFF, dtype=torch.uint8, device="cuda")
            self.raw.append(raw)
            self.span.append((front, size))
            self.out.append(raw[front:front + size].view(dt).view(shape))
        self.out = tuple(self.out)

    def check(self, what):
        for name, raw, (front, size) in zip(NAMES, self.raw, self.span):
            assert bool((raw[:front] == 0xFF).all()) and bool((raw[front + size:] == 0xFF).all()), "%s %s: a guard was written" % (what, name)


# ---- 1. every output against the rule and against the plain dataset ----
@pytest.mark.parametrize("R,P", WINDOWS)
@pytest.mark.parametrize("F", lp_cases.FUTURE_STEPS)
@pytest.mark.parametrize("exp", ["other", "ego"])
@pytest.mark.parametrize("A", [64, 128])
def test_a_batch_equals_the_rule_in_one_shard_and_in_three(A, exp, F, R, P):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    sel = _sel(A, R, P, F)
    want = _want(A, R, P, F, exp, sel)
    vi, _ = _index(A, R, P)
    bad = sum(1 for p in sel if not 0 <= p < len(vi))
    assert bad == 2 and (30 <= len(sel) or len(vi) < 30) and len(sel) <= 45 and len(set(sel)) < len(sel)
    idx2 = vi[[p for p in sel if 0 <= p < len(vi)], 1]
    assert R == 1 or (idx2 < R - 1).any()
    assert (idx2 + F < 91).any() and ((idx2 + F >= 91).any() or F < P)  # the future on both sides of the episode's end
    tsel = torch.tensor(sel, dtype=torch.int64, device="cuda")
    for k, sizes in enumerate(((7,), (3, 0, 4))):
        ds = _dataset(A, R, P, F, exp, sizes)
        assert len(ds) == len(vi) and np.array_equal(ds.valid_indices.cpu().numpy(), vi) and ds.nbytes == 16 * len(vi) + 4
        carved = _Carved(ds, len(sel), lead=1 + 2 * k)
        assert carved.out[6].data_ptr() % 4 == 1 + 2 * k
        out = ds.batch(tsel, out=carved.out)
        assert all(o.data_ptr() == c.data_ptr() for o, c in zip(out, carved.out))
        what = "A=%d %s F=%d R=%d P=%d shards %s" % (A, exp, F, R, P, sizes)
        carved.check(what)
        _check(_host(out), want, A, R, P, F, exp, sel, what)
        assert int(ds.bad_indices) == bad
        # the window, the targets and both window masks are the plain dataset's, bit for bit
        plain = DeviceExpertDataset(list(_shards(A, sizes)), rollout_len=R, pred_len=P).batch(tsel)
        for i, j in ((0, 0), (1, 1), (4, 2), (5, 3)):
            assert torch.equal(_bytes(out[i]), _bytes(plain[j])), (what, NAMES[i])
        fresh = ds.batch(tsel)  # buffers of its own: the same bytes
        assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(fresh, out)), what


def test_the_classes_follow_xy_range():
    A, R, P, F = 64, 5, 1, 35
    sel = _sel(A, R, P, F)
    ds = _dataset(A, R, P, F, "ego", xy_range=lp_cases.EGO_RANGE)
    got = _host(ds.batch(torch.tensor(sel, dtype=torch.int64, device="cuda")))
    want = _want(A, R, P, F, "ego", sel, lp_cases.EGO_RANGE)
    _check(got, want, A, R, P, F, "ego", sel, "xy_range", lp_cases.EGO_RANGE)
    assert not np.array_equal(want[7], _want(A, R, P, F, "ego", sel)[7]) and want[7][2] != 36  # (the padding label moved too)


# ---- 2. the plain dataset on the same tensors is what it was ----
@pytest.mark.parametrize("A,R,P", [(128, 5, 1), (64, 10, 5)])
def test_the_plain_dataset_is_unchanged(A, R, P):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    ds = DeviceExpertDataset(list(_shards(A, (3, 0, 4))), rollout_len=R, pred_len=P)
    sel = _sel(A, R, P, 35)
    out = ds.batch(torch.tensor(sel, dtype=torch.int64, device="cuda"))
    want = il_cases.batch(_case(A), R, P, np.array(sel, np.int64))
    assert len(out) == 5
    for name, o, w in zip(("obs", "actions", "partner_mask", "road_mask", "data_idx"), out, want):
        g = _bytes(o).cpu().numpy()
        assert np.array_equal(g, w.astype(np.uint8) if w.dtype == bool else w), name
    assert int(ds.bad_indices) == 2


# ---- 3. an epoch ----
@pytest.mark.parametrize("exp", ["other", "ego"])
def test_an_unshuffled_epoch_visits_every_sample_once(exp):
    A, R, P, F = 64, 5, 1, 35
    ds = _dataset(A, R, P, F, exp)
    M = len(ds)
    batches = list(ds.batches(16, shuffle=False))
    assert [b[0].shape[0] for b in batches] == [16] * (M // 16) + [M % 16] and M % 16 != 0
    got = _host(tuple(torch.cat([b[i] for b in batches]) for i in range(8)))
    sel = tuple(range(M))
    _check(got, _want(A, R, P, F, exp, sel), A, R, P, F, exp, sel, "epoch " + exp)  # sample k of the epoch is sample k of the index
    assert int(ds.bad_indices) == 0
    assert sum(b[0].shape[0] for b in ds.batches(16, drop_last=True)) == M - M % 16


def test_out_buffers_and_sel_are_checked():
    ds = _dataset(64, 5, 1, 1, "other")
    sel = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = ds.batch(sel)
    assert [tuple(o.shape) for o in good] == [s for s, _ in ds.batch_shapes(4)]
    for i, bad in ((0, good[0].double()), (2, good[2].to(torch.uint8)), (3, good[3][:, :4]), (6, good[6][:, :62]), (7, good[7].to(torch.int32)),
                   (7, good[7].cpu())):
        out = list(good)
        out[i] = bad
        with pytest.raises(ValueError, match=ds.OUT_NAMES["other"][i]):
            ds.batch(sel, out=tuple(out))
    with pytest.raises(ValueError, match="eight"):
        ds.batch(sel, out=good[:5])
    for bad_sel in (sel.to(torch.int32), sel.cpu(), sel.view(2, 2), [0, 1]):
        with pytest.raises(ValueError, match="sel"):
            ds.batch(bad_sel)
    empty = ds.batch(sel[:0])
    assert [tuple(o.shape) for o in empty] == [s for s, _ in ds.batch_shapes(0)]
    assert int(ds.bad_indices) == 0
