"""GPU suite: the two single-workgroup scans of the learner path past one element per lane -- k_rollout_plan
(csrc/rollout.hip, `DeviceRollout.store`) and k_learner_rows (csrc/learner.hip, `set_learner_rows`).  Each is one workgroup of
1024 lanes with a contiguous chunk of ceil(n / 1024) rows or slots per lane; every other test of them has n <= 512, where the
chunk is 1, no lane loops twice and the room left in the batch can only end between two lanes.

The references, yardsticks and comparisons are the ones of tests/test_gpu_rollout.py (the numpy restatement of the reference's
Experience, bit for bit after every step, in canary-filled storage) and of tests/test_gpu_learner_rows.py (twin simulators:
the full [W, A, D] pack indexed with torch's boolean mask against the learner rows, bit for bit)."""
import numpy as np
import pytest
import torch

from tests import parity as P
from tests import ppo_reference as PR
from tests import rollout_cases as RC
from tests import test_gpu_learner_rows as LR
from tests import test_gpu_rollout as TR
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

LANES = 1024  # PLAN_THREADS of csrc/rollout.hip, MAP_THREADS of csrc/learner.hip


def lanes_of(n):
    """(chunk, lanes that hold at least one element, lanes that hold none) of a scan over n elements."""
    chunk = -(-n // LANES)
    used = -(-n // chunk)
    return chunk, used, LANES - used


# ---- DeviceRollout.store

STEP_KINDS = ("all", "none", "random", "last_lane", "lane0", "alternating")  # then the truncated step


def _mask(kind, n, rng):
    chunk, used, _ = lanes_of(n)
    i = np.arange(n)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "none":
        return np.zeros(n, bool)
    if kind == "random":
        return rng.random(n) < 0.6
    if kind == "last_lane":   # live only in the chunk of the last lane that holds a row
        return i >= (used - 1) * chunk
    if kind == "lane0":       # live only in lane 0's chunk
        return i < chunk
    assert kind == "alternating"  # every lane with two rows or more holds both kinds
    return i % 2 == 0


def _masks(n, cut, seed):
    rng = np.random.default_rng(seed)
    return [_mask(k, n, rng) for k in STEP_KINDS] + [_mask("random" if cut == "inside" else "all", n, rng)]


def _room_for(last, n, cut):
    """How many rows of the last step's mask must fit for the cut to fall where the case wants it: strictly inside a lane's
    chunk (that lane's live rows in front of the cut are stored, a later live row of the same lane is dropped), or exactly
    on a lane boundary."""
    chunk = lanes_of(n)[0]
    live = np.flatnonzero(last)
    for room in range(len(live) // 2, len(live)):
        same = live[room - 1] // chunk == live[room] // chunk
        if cut == "inside" and same:
            return room
        if cut == "boundary" and not same and live[room] % chunk == 0 and (live[room - 1] + 1) % chunk == 0:
            return room
    raise AssertionError("no such cut in this mask")


def _assert_the_cut(ex, mask, n, cut, what):
    """The premise of the case, from the mask of the step about to be stored and the restatement's ptr."""
    chunk = lanes_of(n)[0]
    live = np.flatnonzero(mask)
    room = ex.batch_size - ex.ptr
    assert 0 < room < len(live), (what, "the step must be truncated", room, len(live))
    kept, lost = int(live[room - 1]), int(live[room])
    if cut == "inside":
        assert chunk > 1 and kept // chunk == lost // chunk, (what, "the cut is not inside one lane's chunk", kept, lost, chunk)
        first = int(live[live // chunk == kept // chunk][0])
        assert first <= kept < lost, what  # the lane's first live row is stored, a later live row of the same lane is not
    else:
        assert chunk > 1 and lost % chunk == 0 and kept == lost - 1 and mask[lost - chunk:lost].all(), (what, "not a lane boundary")
    return kept // chunk, kept, lost


ROLLOUT_CASES = ([(n, w, "inside") for n in (1025, 2048, 3000) for w in (4, 7)] +
                 [(1025, 7, "boundary"), (2048, 4, "boundary"), (3000, 7, "boundary")])


@pytest.mark.parametrize("n,width,cut", ROLLOUT_CASES, ids=["N%d-w%d-%s" % c for c in ROLLOUT_CASES])
def test_store_sort_gae_and_gather_past_one_row_per_lane(n, width, cut):
    k = ROLLOUT_CASES.index((n, width, cut))
    chunk, used, empty = lanes_of(n)
    assert (chunk, empty) == {1025: (2, 511), 2048: (2, 0), 3000: (3, 24)}[n]
    action_shape = (2,) if k % 2 else ()
    masks = _masks(n, cut, seed=50 + k)
    B = sum(int(m.sum()) for m in masks[:-1]) + _room_for(masks[-1], n, cut)
    carver = TR.Carver()
    ro = TR._carved_rollout(carver, 0, B, num_rows=n, obs_width=width, action_shape=action_shape)
    ex = PR.Experience(B, obs_width=width, action_shape=action_shape)
    TR._check_storage(ro, ex, carver, "empty")

    def rollout(tag, seed, canary_beyond):
        for step, mask in enumerate(masks):
            what = "%s step %d (%s)" % (tag, step, (STEP_KINDS + ("truncated",))[step])
            assert not ex.full and not ro.full, what
            inputs = RC.step_inputs(step, n, width, action_shape, "all", seed=seed)[:6] + (mask,)
            if step == len(masks) - 1:
                lane, kept, lost = _assert_the_cut(ex, mask, n, cut, what)
                dropped = int(mask.sum()) - (B - ex.ptr)
            TR._store_both(ro, ex, inputs, value_2d=step % 2 == 1)
            TR._check_storage(ro, ex, carver, what, canary_beyond=canary_beyond)
        assert ex.full and ro.full and int(ro.ptr.item()) == B and int(ro.step.item()) == len(masks)
        return lane, kept, lost, dropped

    lane, kept, lost, dropped = rollout("first rollout", k, True)
    assert ex.dropped == dropped == int(ro.dropped.item()) and dropped > 0
    print("ROLLOUT_SCALE N=%d w=%d %s: chunk %d, %d empty lanes, batch %d, the cut fell in lane %d after row %d (row %d dropped), "
          "dropped %d" % (n, width, cut, chunk, empty, B, lane, kept, lost, dropped))
    for r in range(2):
        rows = np.array([key[0] for key in ex.sort_keys])
        assert np.bincount(rows, minlength=n).max() >= 3, "some row is stored three times: ord > 1 at chunk > 1"
        idxs = ro.sort_training_data().cpu().numpy()
        want_idxs = ex.sort_training_data()
        assert np.array_equal(idxs, want_idxs), "rollout %d: the sorted order" % r
        assert ro.state.cpu().numpy().tolist() == [0, 0, ex.dropped, 0] and int(ro._count.abs().sum().item()) == 0
        adv = ro.compute_gae(0.99, 0.95).cpu().numpy()
        want_adv = PR.compute_gae(ex.dones[want_idxs], ex.values[want_idxs], ex.rewards[want_idxs], 0.99, 0.95)
        assert np.isfinite(want_adv).all() and np.array_equal(adv, want_adv), "rollout %d: the advantages" % r
        want = ex.flatten_batch(adv)
        for name, g, w in zip(type(ro).OUT_NAMES, ro.minibatch(0), want):
            TR._equal_bits(g.cpu().numpy(), w[0], "rollout %d: minibatch %s" % (r, name))
        assert int(ro.bad_positions.item()) == 0
        if r == 0:  # a second rollout into the same object: other values, the same masks, the same cut
            rollout("second rollout", 100 + k, False)
            assert ex.dropped == 2 * dropped


# ---- set_learner_rows

WORLDS = 18
TWIN_STEPS = 3    # compared steps per mask: 6 masks, 18 steps and more per pair of simulators
MASKS = ("controlled", "random", "all", "none", "last_world", "first_slot")


def _slot_mask(kind, sim):
    if kind in ("last_world", "first_slot"):
        m = torch.zeros(sim._W, sim._A, dtype=torch.bool, device=sim._device)
        if kind == "last_world":   # true only in the last world: every lane in front of it counts nothing
            m[-1] = True
        else:                      # true only in slot 0 of world 0: the total comes from lane 0 alone
            m[0, 0] = True
        return m
    return LR._mask(kind, sim)


@pytest.mark.parametrize("roads,slots", [("linear", 64), ("linear", 128), ("ref_order", 64), ("ref_order", 128)],
                         ids=lambda v: str(v))
def test_learner_rows_past_one_slot_per_lane(monkeypatch, tmp_path, roads, slots):
    from gpudrive_lab_amd.learner import action_table
    knn_order, algo, env = LR.ROADS[roads]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    small = [TEST_JSON, SCENE_407, SCENE_4, P.parked_car_scene(tmp_path)]
    scenes = (small * WORLDS)[:WORLDS]
    chunk, used, empty = lanes_of(WORLDS * slots)
    assert (chunk, used, empty) == {64: (2, 576, 448), 128: (3, 768, 256)}[slots]
    kw = dict(LR.BASE, roadObservationAlgorithm=algo, collisionBehaviour=1)
    full = P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, **kw)
    rsim = P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, **kw)
    try:
        assert full.direct_pack(only=True)
        table = action_table("classic").cuda()
        gen = torch.Generator().manual_seed(13)
        for mi, kind in enumerate(MASKS):
            what = "%s A=%d %s" % (roads, slots, kind)
            mask = _slot_mask(kind, rsim)
            want_n = int(mask.sum())
            n = rsim.set_learner_rows(mask)
            assert n == want_n, (what, "the returned count", n, want_n)
            D = 6 + (slots - 1) * 6 + 200 * 13
            guard = LR._Guarded(n, D, rsim._device)
            rows = rsim.direct_pack_rows(only=True, out=guard.buf)
            assert tuple(rows.shape) == (n, D)
            torch.cuda.synchronize()
            guard.check(what + " attach")
            LR._equal_bits(rows, full.packed_observations()[mask], what + " attach")
            for k in range(TWIN_STEPS):
                a = LR._actions(gen, WORLDS, slots, full._device)
                full.action_tensor().to_torch().copy_(a)
                rsim.action_tensor().to_torch().copy_(a)
                if n > 0:  # the decoded table rows land in the mask's slots, in its row-major order, and nowhere else
                    idx = torch.randint(0, table.shape[0], (n,), generator=gen).cuda()
                    rsim.set_discrete_actions(idx, table)
                    act = full.action_tensor().to_torch()
                    act[:, :, :3][mask] = table[idx]
                    torch.cuda.synchronize()
                    LR._equal_bits(rsim.action_tensor().to_torch(), act, what + " actions step %d" % k)
                full.step()
                rsim.step()
                torch.cuda.synchronize()
                guard.check(what + " step %d" % k)
                LR._equal_bits(rows, full.packed_observations()[mask], what + " step %d" % k)
            print("LEARNER_ROWS_SCALE %s: %d slots, chunk %d, %d empty lanes, rows %d" % (what, WORLDS * slots, chunk, empty, n))
    finally:
        full.close()
        rsim.close()
