"""GPU suite: the expert trajectory recorder (gd_record_expert, gpudrive_lab_amd.recorder.ExpertRecorder) against the
reference's own loop (tests/il_reference.py: gpudrive/integrations/il/storage.py:17-98 on the call-sequence harness).

Twin simulators on the same scenes: one recorded by one C call, the other driven step by step by the restated loop.  With
the loop's observation taken from `packed_observations()` (the second-pass kernel the reference's golden pins on the CPU)
every output is compared bit for bit; with torch's own assembly on the device the observation is held to PACK_ATOL /
PACK_RTOL (tests/parity.py, what tests/test_gpu_round2.py already uses between the two: torch's device division is not
bit-identical to the kernels') and everything else stays bitwise."""
import pytest
import torch

from tests import il_reference
from tests import parity as P
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON

pytestmark = pytest.mark.gpu

BASE = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, distanceToGoalThreshold=2.0,
            initOnlyValidAgentsAtFirstStep=1, IgnoreNonVehicles=1)
ROADS = {  # (knn_order, roadObservationAlgorithm, environment), as in tests/test_gpu_learner_rows.py
    "ref_order": (0, 0, {"GPUDRIVE_RANK_MIN_ROADS": "200"}),
    "linear": (0, 1, {}),
}
MODELS = {"classic": 0, "delta_local": 2}
REMOVED, IGNORE = 1, 2  # CollisionBehaviour
SCENES = [TEST_JSON, SCENE_407, SCENE_4] * 2  # 6 worlds: the per-index reference loop is slow on purpose
T = 91
CANARY = 1 << 16
CANARY_BITS = 0x7FC0DEAD  # a NaN payload no kernel writes
CANARY_BYTE = 0xA5
DEFAULTS = dict(obs=0, actions=0, dead_mask=1, partner_mask=2, road_mask=1, ego_global_pos=0, ego_global_rot=0)
FLOATS = ("obs", "actions", "ego_global_pos", "ego_global_rot")


def _sim(model, cb, roads, slots, static, monkeypatch, scenes=SCENES):
    knn_order, algo, env = ROADS[roads]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return P.make_gpu_sim(scenes, max_agents=slots, knn_order=knn_order, dynamicsModel=MODELS[model], collisionBehaviour=cb,
                          roadObservationAlgorithm=algo, isStaticAgentControlled=static, **BASE)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what, bits=False):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    x, y = (_bits(a), _bits(b)) if bits else (a, b)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        raise AssertionError("%s: %d elements differ, first at %s: %s vs %s"
                             % (what, bad.shape[0], bad[0].tolist(), a[tuple(bad[0])].item(), b[tuple(bad[0])].item()))


def _compare(ep, r, what, obs_bitwise):
    """Every output of the recorder against the reference loop's."""
    if obs_bitwise:
        _same(ep.obs, r["obs"], what + " obs", bits=True)
    else:
        diff = (ep.obs - r["obs"]).abs()
        worst = (diff - P.PACK_RTOL * r["obs"].abs()).max().item()
        print("RECORDER %s obs vs torch's assembly: max |diff| %.3g, max (|diff| - rtol |ref|) %.3g (atol %.1g)"
              % (what, diff.max().item(), worst, P.PACK_ATOL))
        assert torch.allclose(ep.obs, r["obs"], atol=P.PACK_ATOL, rtol=P.PACK_RTOL), (what, worst)
    _same(ep.actions, r["actions"], what + " actions", bits=True)
    _same(ep.dead_mask, r["dead_mask"], what + " dead_mask")
    _same(ep.partner_mask.to(torch.int64), r["partner_mask"], what + " partner_mask")
    _same(ep.road_mask, r["road_mask"], what + " road_mask")
    _same(ep.ego_global_pos, r["ego_global_pos"], what + " ego_global_pos", bits=True)
    _same(ep.ego_global_rot, r["ego_global_rot"], what + " ego_global_rot", bits=True)
    for k in ("goal_achieved", "off_road", "veh_collision"):
        _same(getattr(ep, k), r[k], what + " " + k, bits=True)
    _same(ep.keep, ~r["collision"], what + " keep")
    assert int(ep.steps) == r["iterations"], (what, int(ep.steps), r["iterations"])


MATRIX = [  # dynamics, collisionBehaviour, roads, slots, isStaticAgentControlled
    ("delta_local", REMOVED, "linear", 128, 0),     # storage.py's own configuration ...
    ("delta_local", REMOVED, "ref_order", 128, 0),  # ... with both road algorithms
    ("delta_local", REMOVED, "linear", 64, 1),
    ("delta_local", IGNORE, "ref_order", 128, 1),
    ("classic", IGNORE, "linear", 64, 0),
    ("classic", REMOVED, "ref_order", 64, 1),
]


@pytest.mark.parametrize("model,cb,roads,slots,static", MATRIX, ids=["%s-cb%d-%s-%d-static%d" % c for c in MATRIX])
def test_recording_equals_the_reference_loop(monkeypatch, model, cb, roads, slots, static):
    from gpudrive_lab_amd.harness import TorchCallSequence
    from gpudrive_lab_amd.recorder import ExpertRecorder
    rsim = _sim(model, cb, roads, slots, static, monkeypatch)
    tsim = _sim(model, cb, roads, slots, static, monkeypatch)
    try:
        rec = ExpertRecorder(rsim)
        ep = rec.record()
        torch.cuda.synchronize()
        N, D = rec.num_agents, 6 + (slots - 1) * 6 + 200 * 13
        assert N == int((tsim.controlled_state_tensor().to_torch() == 1).sum()) and N >= 26
        assert tuple(ep.obs.shape) == (N, T, D) and tuple(ep.partner_mask.shape) == (N, T, slots - 1)
        # the conditions this test relies on, so that a vacuous pass cannot hide a failure
        dm = ep.dead_mask
        assert bool(dm[:, :90].any()), "no row dies before t = 90"
        assert bool((~dm[:, 50:]).any()), "no row is alive at t >= 50"
        assert bool((~dm[:, 0]).all()), "a recorded row is dead at t = 0"
        if model == "classic" or static:
            assert bool(ep.keep.any()) and bool((~ep.keep).any()), "both values of keep must occur here"
        if model == "delta_local" and not static:
            assert int(ep.steps) < T, "the early break is not exercised"
        assert bool((ep.partner_mask == 0).any()) and bool((ep.partner_mask == 2).any())
        if static == 0:
            assert bool((ep.partner_mask == 1).any()), "no Static partner in sight"
        print("RECORDER %s cb%d %s A=%d static=%d: rows %d steps %d dropped %d goal %d"
              % (model, cb, roads, slots, static, N, int(ep.steps), int((~ep.keep).sum()), int(ep.goal_achieved.sum())))
        for source in ("packed_observations", "get_obs"):
            h = TorchCallSequence(tsim, dynamics_model=model)
            r = il_reference.save_trajectory(h, get_obs=tsim.packed_observations if source == "packed_observations" else None)
            _compare(ep, r, "%s-%s" % (model, source), obs_bitwise=source == "packed_observations")
    finally:
        rsim.close()
        tsim.close()


class _Guarded:
    """One output array pre-filled with its default, with a canary tail behind it."""

    def __init__(self, name, shape, dev):
        self.name, self.shape = name, shape
        self.n = 1
        for s in shape:
            self.n *= s
        if name in FLOATS:
            self.raw = torch.full((self.n + CANARY,), float(DEFAULTS[name]), dtype=torch.float32, device=dev)
            self.raw.view(torch.int32)[self.n:] = CANARY_BITS
            self.buf = self.raw
        else:
            self.raw = torch.full((self.n + CANARY,), DEFAULTS[name], dtype=torch.uint8, device=dev)
            self.raw[self.n:] = CANARY_BYTE
            self.buf = self.raw if name == "partner_mask" else self.raw.view(torch.bool)

    def check(self):
        tail = self.raw.view(torch.int32)[self.n:] if self.name in FLOATS else self.raw[self.n:]
        want = CANARY_BITS if self.name in FLOATS else CANARY_BYTE
        assert bool((tail == want).all()), "%s: write past the buffer" % self.name


@pytest.mark.parametrize("slots", [64, 128])
def test_dead_steps_keep_the_defaults_and_nothing_is_written_past_the_buffers(monkeypatch, slots):
    from gpudrive_lab_amd.recorder import ExpertRecorder
    sim = _sim("delta_local", REMOVED, "linear", slots, 1, monkeypatch)
    try:
        rec = ExpertRecorder(sim)
        N = rec.num_agents
        cols = dict(obs=6 + (slots - 1) * 6 + 200 * 13, actions=3, dead_mask=1, partner_mask=slots - 1, road_mask=200,
                    ego_global_pos=2, ego_global_rot=1)
        guards = {k: _Guarded(k, (N, T, c), sim._device) for k, c in cols.items()}
        ep = rec.record(buffers={k: g.buf for k, g in guards.items()})
        torch.cuda.synchronize()
        assert ExpertRecorder.nbytes(sim) == sum(g.n * g.raw.element_size() for g in guards.values()) + N * 13 + 92 * 4
        dead = ep.dead_mask
        assert bool(dead.any()) and bool((~dead).any())
        for k, g in guards.items():
            g.check()
            x = getattr(ep, k)
            assert x.data_ptr() == g.buf.data_ptr(), k  # recorded in place
            if k == "dead_mask":
                continue
            at_dead = x[dead]
            assert bool((at_dead == DEFAULTS[k]).all()), "%s: a dead (row, step) was written" % k
        # ... and a live one was: the observation of a live step is never all zeros (the one-hot road types alone)
        assert bool((ep.obs[~dead] != 0).any(dim=-1).all())
        assert bool((~ep.road_mask[~dead]).any())
    finally:
        sim.close()


def test_explicit_mask_of_one_agent_that_finishes_early(monkeypatch):
    from gpudrive_lab_amd.harness import TorchCallSequence
    from gpudrive_lab_amd.recorder import ExpertRecorder
    rsim = _sim("delta_local", REMOVED, "linear", 64, 0, monkeypatch)
    tsim = _sim("delta_local", REMOVED, "linear", 64, 0, monkeypatch)
    try:
        rec = ExpertRecorder(rsim)
        ep = rec.record()
        first = torch.where(ep.dead_mask.any(1), ep.dead_mask.to(torch.int32).argmax(1), T)  # first dead step of every row
        first = torch.where(ep.goal_achieved > 0, first, T)
        n = int(first.argmin())
        assert int(first[n]) < 45, "no agent reaches its goal early"
        slot = int(rec.row_slot[n])
        mask = torch.zeros(len(SCENES), 64, dtype=torch.bool, device=rsim._device)
        mask[slot // 64, slot % 64] = True
        one = ExpertRecorder(rsim, mask=mask)
        assert one.num_agents == 1 and one.row_slot.tolist() == [slot]
        e1 = one.record()
        h = TorchCallSequence(tsim, dynamics_model="delta_local")
        r = il_reference.save_trajectory(h, mask=mask, get_obs=tsim.packed_observations)
        assert r["iterations"] == int(first[n]) < 45  # the reference's break, long before t = 90
        _compare(e1, r, "one agent", obs_bitwise=True)
        assert int(e1.steps) == int(first[n]) and bool(e1.dead_mask[0, int(first[n]):].all())
        # the same row of the full recording, up to its death
        k = int(first[n])
        _same(e1.obs[0, :k], ep.obs[n, :k], "one agent vs its row of the full recording", bits=True)
    finally:
        rsim.close()
        tsim.close()


def test_refused_while_only_the_packed_buffer_is_written(monkeypatch):
    from gpudrive_lab_amd.recorder import ExpertRecorder
    sim = _sim("delta_local", REMOVED, "linear", 64, 0, monkeypatch, scenes=SCENES[:3])
    try:
        rec = ExpertRecorder(sim)
        assert sim.direct_pack(only=True)
        with pytest.raises(NotImplementedError, match="stale"):
            rec.record()
        assert sim.direct_pack(only=False)  # the raw rows are written again: allowed
        ep = rec.record()
        assert int(ep.steps) > 0
        with pytest.raises(ValueError):
            rec.record(n_steps=0)
        with pytest.raises(ValueError):
            rec.record(n_steps=92)
    finally:
        sim.close()


def test_fewer_steps_give_the_prefix_of_the_full_recording(monkeypatch):
    from gpudrive_lab_amd.recorder import ExpertRecorder
    sim = _sim("classic", REMOVED, "linear", 64, 1, monkeypatch)
    try:
        rec = ExpertRecorder(sim)
        full = rec.record()
        K = 40
        part = rec.record(n_steps=K)
        torch.cuda.synchronize()
        assert int(full.steps) == T and int(part.steps) == K
        assert bool(full.dead_mask[:, :K].any()) and bool((~full.dead_mask[:, K:]).any())
        for k in ("obs", "actions", "dead_mask", "partner_mask", "road_mask", "ego_global_pos", "ego_global_rot"):
            a, b = getattr(part, k), getattr(full, k)
            _same(a[:, :K], b[:, :K], "prefix " + k, bits=k in FLOATS)
            assert bool((a[:, K:] == DEFAULTS[k]).all()), "%s: written past n_steps" % k
        for k in ("goal_achieved", "off_road", "veh_collision"):
            assert bool((getattr(part, k) <= getattr(full, k)).all()), k
    finally:
        sim.close()


def test_resample_derives_the_rows_of_the_new_scenes(monkeypatch):
    from gpudrive_lab_amd.recorder import ExpertRecorder
    scenes = SCENES[:3]
    sim = _sim("delta_local", REMOVED, "linear", 64, 0, monkeypatch, scenes=scenes)
    fresh = _sim("delta_local", REMOVED, "linear", 64, 0, monkeypatch, scenes=scenes[1:] + scenes[:1])
    try:
        rec = ExpertRecorder(sim)
        before = rec.row_slot.clone()
        rec.record()
        rec.resample(scenes[1:] + scenes[:1])
        want = ExpertRecorder(fresh)
        assert rec.num_agents == want.num_agents and torch.equal(rec.row_slot, want.row_slot)
        assert not torch.equal(rec.row_slot, before)  # 2 / 3 / 8 controlled agents per scene: the rows moved
        a, b = rec.record(), want.record()
        for k in ("obs", "actions", "ego_global_pos", "ego_global_rot"):
            _same(getattr(a, k), getattr(b, k), "resample " + k, bits=True)
        for k in ("dead_mask", "partner_mask", "road_mask", "keep"):
            _same(getattr(a, k), getattr(b, k), "resample " + k)
        assert int(a.steps) == int(b.steps)
    finally:
        sim.close()
        fresh.close()
