"""GPU suite: the device expert dataset (gd_il_index / gd_il_batch, gpudrive_lab_amd.il_dataset.DeviceExpertDataset) against
the numpy rule of tests/il_cases.py, which tests/test_il_dataset.py pins to the reference's own ExpertDataset.  Everything is
compared bit for bit (float outputs as int32).  Only the last test builds a simulator."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import il_cases
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

CANARY_BITS = 0x7FC0DEAD  # a NaN payload nothing here writes
CANARY_BYTE = 0xA5
CANARY_I64 = 0x5A5A5A5A5A5A5A5A
NAMES = ("obs", "actions", "partner_mask", "road_mask", "data_idx")


@functools.lru_cache(maxsize=None)
def _case(A):
    return il_cases.make_case(A)


@functools.lru_cache(maxsize=None)
def _shards(A, sizes):
    """The case on the device, cut into shards of the given row counts (shared by the tests; never written)."""
    return tuple({k: torch.from_numpy(v).cuda() for k, v in part.items()} for part in il_cases.split(_case(A), sizes))


@functools.lru_cache(maxsize=None)
def _dataset(A, R, P, sizes=(il_cases.N_ROWS,)):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    return DeviceExpertDataset(list(_shards(A, sizes)), rollout_len=R, pred_len=P)


@functools.lru_cache(maxsize=None)
def _want(A, R, P, sel):
    """The rule's batch for a tuple of positions (computed once per case)."""
    return il_cases.batch(_case(A), R, P, np.array(sel, np.int64))


def _shuffled(M, step=89, first=17):
    """A permutation of range(M) from integer arithmetic."""
    while math.gcd(step, M) != 1:
        step += 1
    return tuple(int(x) for x in (first + step * np.arange(M, dtype=np.int64)) % M)


def _host(out):
    obs, actions, partner, road, data_idx = out
    assert obs.dtype == torch.float32 and actions.dtype == torch.float32 and data_idx.dtype == torch.int64
    assert partner.dtype == torch.bool and road.dtype == torch.bool
    return (obs.cpu().numpy().view(np.int32), actions.cpu().numpy().view(np.int32), partner.cpu().numpy(), road.cpu().numpy(),
            data_idx.cpu().numpy())


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d elements differ, first at %s: %s vs %s"
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


# ---- 1. the index ----
@pytest.mark.parametrize("R,P", il_cases.WINDOWS)
@pytest.mark.parametrize("A", [64, 128])
def test_the_index_equals_the_rule_with_one_shard_and_with_two(A, R, P):
    want, _ = il_cases.index(_case(A), R, P)
    assert len(want) > 0
    for sizes in ((7,), (4, 3)):
        ds = _dataset(A, R, P, sizes)
        vi = ds.valid_indices
        assert vi.dtype == torch.int64 and vi.is_cuda and len(ds) == len(want), (sizes, len(ds), len(want))
        assert np.array_equal(vi.cpu().numpy(), want), sizes
        assert ds.nbytes == 16 * len(want) + 4 and ds.num_rows == 7 and ds.max_agents == A


# ---- 2. the batch ----
WINDOW_OF_R = {1: 1, 2: 3, 3: 2, 4: 1, 5: 1}  # R -> P; R * (A - 1) mod 4 takes 3, 2, 1, 0, 3 (A - 1 = 3 mod 4 for both widths)


@pytest.mark.parametrize("R", sorted(WINDOW_OF_R))
@pytest.mark.parametrize("A,sizes", [(128, (7,)), (64, (4, 3))])
def test_every_sample_equals_the_rule_at_three_batch_sizes(A, sizes, R):
    P = WINDOW_OF_R[R]
    ds = _dataset(A, R, P, sizes)
    M = len(ds)
    order = _shuffled(M)
    want = _want(A, R, P, order)
    sel = torch.tensor(order, dtype=torch.int64, device="cuda")
    assert R == 1 or (want[0][:, 0] == 0).all(axis=1).any()  # a window that crosses t = 0 is among them
    for B in (1, 3, M):
        parts = [ds.batch(sel[lo:lo + B]) for lo in range(0, M, B)]
        got = _host(tuple(torch.cat([p[i] for p in parts]) for i in range(5)))
        _same(got, want, "A=%d R=%d P=%d B=%d" % (A, R, P, B))
    assert int(ds.bad_indices) == 0


# ---- 3. ownership: every byte of every output is written, nothing outside them ----
class _Carved:
    """The five outputs carved out of larger canary-filled buffers, with `lead` extra bytes in front of the partner mask so
    that its first byte takes every phase of a dword."""

    def __init__(self, ds, B, lead):
        self.raw, self.out, self.span = [], [], []
        for name, (shape, dt) in zip(NAMES, ds.batch_shapes(B)):
            n = int(np.prod(shape))
            if dt == torch.float32:
                front, fill, raw_dt = 64, CANARY_BITS, torch.int32
            elif dt == torch.int64:
                front, fill, raw_dt = 4, CANARY_I64, torch.int64
            else:
                front, fill, raw_dt = (64 + lead if name == "partner_mask" else 64), CANARY_BYTE, torch.uint8
            raw = torch.full((front + n + 67,), fill, dtype=raw_dt, device="cuda")
            self.raw.append(raw)
            self.span.append((front, n, fill))
            self.out.append(raw[front:front + n].view(dt).view(shape))
        self.out = tuple(self.out)

    def check(self, what):
        for name, raw, (front, n, fill) in zip(NAMES, self.raw, self.span):
            assert bool((raw[:front] == fill).all()) and bool((raw[front + n:] == fill).all()), "%s %s: a guard was written" % (what, name)
            assert not bool((raw[front:front + n] == fill).any()), "%s %s: a canary survives inside the output" % (what, name)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("A,R,P", [(128, 3, 2), (64, 5, 1), (64, 4, 1)])
def test_outputs_are_written_whole_and_nothing_else_is(A, R, P, lead):
    ds = _dataset(A, R, P)
    M = len(ds)
    first, second = (0, 1, M - 1, 200, 1), (M - 2, 0, 77, 2, 130)  # windows that cross t = 0, the ends, a repeat
    carved = _Carved(ds, len(first), lead)
    assert carved.out[2].data_ptr() % 4 == lead
    for round_, sel in enumerate((first, second)):  # the second call reuses buffers that hold another batch
        out = ds.batch(torch.tensor(sel, dtype=torch.int64, device="cuda"), out=carved.out)
        assert all(o.data_ptr() == c.data_ptr() for o, c in zip(out, carved.out))
        carved.check("call %d" % round_)
        _same(_host(out), _want(A, R, P, sel), "A=%d R=%d lead=%d call %d" % (A, R, lead, round_))


def test_out_buffers_are_checked():
    ds = _dataset(64, 5, 1)
    sel = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = ds.batch(sel)
    for i, bad in ((0, good[0].double()), (1, good[1][:3]), (2, good[2].to(torch.uint8)), (3, good[3].cpu()),
                   (4, good[4].to(torch.int32)), (0, good[0].transpose(1, 2)), (0, torch.empty(4, 5, 2985, device="cuda")[..., 1:])):
        out = list(good)
        out[i] = bad
        with pytest.raises(ValueError, match=NAMES[i]):
            ds.batch(sel, out=tuple(out))
    with pytest.raises(ValueError, match="five"):
        ds.batch(sel, out=good[:4])
    for bad_sel in (sel.to(torch.int32), sel.cpu(), sel.view(2, 2), torch.zeros(8, dtype=torch.int64, device="cuda")[::2], [0, 1]):
        with pytest.raises(ValueError, match="sel"):
            ds.batch(bad_sel)
    assert int(ds.bad_indices) == 0


# ---- 4. repeats and positions outside the index ----
@pytest.mark.parametrize("A,R,P", [(128, 5, 1), (64, 3, 2)])
def test_repeats_and_out_of_range_positions(A, R, P):
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    ds = DeviceExpertDataset(list(_shards(A, (7,))), rollout_len=R, pred_len=P)  # (its own counter)
    M = len(ds)
    sel = (3, -1, 3, M, 7, 2 ** 31, 3, M - 1, -2 ** 40)
    got = _host(ds.batch(torch.tensor(sel, dtype=torch.int64, device="cuda")))
    _same(got, _want(A, R, P, sel), "A=%d" % A)  # the rule pads them; the others are unaffected
    for g in got:
        assert np.array_equal(g[0], g[2]) and np.array_equal(g[0], g[6])
    assert not got[0][[1, 3, 5, 8]].any() and got[2][[1, 3, 5, 8]].all() and got[4][[1, 3, 5, 8]].tolist() == [[-1, -1]] * 4
    assert ds.bad_indices.dtype == torch.int32 and int(ds.bad_indices) == 4
    ds.batch(torch.tensor([M, 0], dtype=torch.int64, device="cuda"))
    assert int(ds.bad_indices) == 5


# ---- 5. an epoch ----
def test_an_epoch_visits_every_sample_once_and_a_seed_fixes_the_order():
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    A, R, P = 64, 3, 2
    a = _dataset(A, R, P)
    b = DeviceExpertDataset(list(_shards(A, (4, 3))), rollout_len=R, pred_len=P)
    M = len(a)
    want = il_cases.index(_case(A), R, P)[0]
    ga, gb = (torch.Generator(device="cuda").manual_seed(1234) for _ in range(2))
    epochs = []
    for _ in range(2):
        ba, bb = list(a.batches(50, generator=ga)), list(b.batches(50, generator=gb))
        assert [x[0].shape[0] for x in ba] == [50] * (M // 50) + [M % 50] and M % 50 != 0  # a short last batch
        for x, y in zip(ba, bb):
            for u, v in zip(x, y):  # (bit patterns: the actions hold NaNs)
                assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                                   v.view(torch.int32) if v.dtype == torch.float32 else v)
        idx = torch.cat([x[4] for x in ba]).cpu().numpy()
        assert sorted(map(tuple, idx.tolist())) == sorted(map(tuple, want.tolist()))  # the multiset of data_idx
        epochs.append(idx)
    assert not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[0], want)  # shuffled, anew every epoch
    assert [x[0].shape[0] for x in a.batches(50, drop_last=True)] == [50] * (M // 50)
    plain = torch.cat([x[4] for x in a.batches(64, shuffle=False)]).cpu().numpy()
    assert np.array_equal(plain, want)
    assert int(a.bad_indices) == 0 and int(b.bad_indices) == 0


def test_no_samples_and_no_rows():
    from gpudrive_lab_amd.il_dataset import DeviceExpertDataset
    full = _shards(64, (7,))[0]
    dead = dict(full, dead_mask=torch.ones_like(full["dead_mask"]))
    none = {k: v[:0] for k, v in full.items()}
    for ds in (DeviceExpertDataset(dead, rollout_len=2), DeviceExpertDataset(none), DeviceExpertDataset([none, none])):
        assert len(ds) == 0 and tuple(ds.valid_indices.shape) == (0, 2) and ds.valid_indices.dtype == torch.int64
        out = ds.batch(torch.zeros(0, dtype=torch.int64, device="cuda"))
        assert [tuple(o.shape) for o in out] == [s for s, _ in ds.batch_shapes(0)] and out[0].shape[0] == 0
        assert list(ds.batches(8)) == [] and list(ds.batches(8, shuffle=False)) == []
        out = ds.batch(torch.zeros(2, dtype=torch.int64, device="cuda"))  # nothing to point at: padding
        assert not out[0].any() and out[2].all() and out[3].all() and out[4].tolist() == [[-1, -1]] * 2
        assert int(ds.bad_indices) == 2
    some = DeviceExpertDataset([none, full, none], rollout_len=5, pred_len=1)  # shards without rows change nothing
    assert torch.equal(some.valid_indices, _dataset(64, 5, 1).valid_indices)
    _same(_host(some.batch(torch.tensor([0, 100], dtype=torch.int64, device="cuda"))), _want(64, 5, 1, (0, 100)), "empty shards")


# ---- 6. end to end: record, then train from it, against the files the reference's trainer would be given ----
def test_recorded_episode_to_batches_equals_the_rule_on_the_saved_files(tmp_path):
    from gpudrive_lab_amd.recorder import ExpertRecorder
    from tests import parity as P
    sim = P.make_gpu_sim([TEST_JSON, SCENE_407, SCENE_4], max_agents=128, knn_order=0, dynamicsModel=2, collisionBehaviour=1,
                         roadObservationAlgorithm=1, isStaticAgentControlled=0, polylineReductionThreshold=0.1,
                         observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0, initOnlyValidAgentsAtFirstStep=1,
                         IgnoreNonVehicles=1)
    try:
        ep = ExpertRecorder(sim).record()
        ds = ep.dataset(rollout_len=5, pred_len=1)
        main, _ = ep.save(str(tmp_path))
        with np.load(main) as z:
            saved = {k: z[k] for k in z.files}
        saved["keep"] = np.ones(saved["obs"].shape[0], bool)  # the file holds the kept rows only
        want_vi, _ = il_cases.index(saved, 5, 1)
        M = len(ds)
        print("IL DATASET end to end: rows %d kept %d samples %d" % (ep.obs.shape[0], saved["obs"].shape[0], M))
        assert M == len(want_vi) > 100 and np.array_equal(ds.valid_indices.cpu().numpy(), want_vi)
        assert bool(ep.dead_mask.any()) and saved["obs"].shape[2] == il_cases.width(128)
        order = _shuffled(M)
        got = _host(ds.batch(torch.tensor(order, dtype=torch.int64, device="cuda")))
        _same(got, il_cases.batch(saved, 5, 1, np.array(order, np.int64)), "end to end")
        assert int(ds.bad_indices) == 0
    finally:
        sim.close()
