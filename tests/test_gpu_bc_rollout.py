"""GPU suite: the closed-loop BC driver (gd_bc_rollout, gpudrive_lab_amd.bc_rollout.ClosedLoopBC) against the reference's own
loop (tests/bc_rollout_reference.py: baselines/il/test/simulation.py:22-135 on the call-sequence harness, with a
`DeviceBCPolicy` called once per step on obs[~dead]).

Twin simulators on the same scenes: one driven by one C call, the other step by step by the restated loop, whose observation
comes from `packed_observations()` (the kernels' own bits: with torch's own assembly the actions would differ in the last bit
and the trajectories would drift apart).  Every output is compared bit for bit.

The weights are tests/bc_cases.state_dict(R) with `head.head`'s bias scaled by HEAD_BIAS_SCALE (see there)."""
import os

import numpy as np
import pytest
import torch

from tests import bc_cases as BC
from tests import bc_rollout_reference as REF
from tests import parity as P
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON
from tests.test_gpu_bc_policy import _no_sync

pytestmark = pytest.mark.gpu

BASE = dict(polylineReductionThreshold=0.1, observationRadius=50.0, rewardType=1, initOnlyValidAgentsAtFirstStep=1,
            IgnoreNonVehicles=1, isStaticAgentControlled=0)
ROADS = {  # (knn_order, roadObservationAlgorithm, environment), as in tests/test_gpu_expert_recorder.py
    "ref_order": (0, 0, {"GPUDRIVE_RANK_MIN_ROADS": "200"}),
    "linear": (0, 1, {}),
}
MODELS = {"classic": 0, "delta_local": 2}
REMOVED, IGNORE = 1, 2  # CollisionBehaviour
SCENES = [TEST_JSON, SCENE_407, SCENE_4] * 2  # 6 worlds
T = 91
# The factor on head.head's bias in the test's state dict.  1.0 was chosen: with the weights of tests/bc_cases.state_dict as they
# are the reference loop already loses rows long before the last step under REMOVED on these scenes (10 to 18 of 26 rows leave
# the road, 10 to 12 collide; asserted below), so nothing is scaled.
HEAD_BIAS_SCALE = 1.0

MATRIX = {  # name -> (A, R, dynamics, collision behaviour, roads)
    "64-5-delta-ignore-linear": (64, 5, "delta_local", IGNORE, "linear"),
    "128-5-delta-removed-linear": (128, 5, "delta_local", REMOVED, "linear"),
    "128-5-delta-removed-ref_order": (128, 5, "delta_local", REMOVED, "ref_order"),
    "64-1-classic-removed-linear": (64, 1, "classic", REMOVED, "linear"),
}


def _state_dict(R):
    sd = BC.state_dict(R)
    sd["head.head.bias"] = sd["head.head.bias"] * HEAD_BIAS_SCALE
    return sd


def _policy(A, R, sd=None):
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    return DeviceBCPolicy.from_state_dict(sd if sd is not None else _state_dict(R), max_agents=A, num_stack=R, **BC.CFG)


class _Env:
    """The environment of one road algorithm for the lifetime of the simulators made under it."""

    def __init__(self, roads):
        self.env = ROADS[roads][2]

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _sim(A, model, cb, roads, scenes=SCENES, goal=2.0):
    knn_order, algo, _ = ROADS[roads]
    return P.make_gpu_sim(scenes, max_agents=A, knn_order=knn_order, dynamicsModel=MODELS[model], collisionBehaviour=cb,
                          roadObservationAlgorithm=algo, distanceToGoalThreshold=goal, **BASE)


def _loop(tsim, policy, model, R, **kw):
    from gpudrive_lab_amd.harness import TorchCallSequence
    h = TorchCallSequence(tsim, dynamics_model=model, num_stack=R)
    return REF.closed_loop(h, policy, source=tsim.packed_observations, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    x, y = _bits(a), _bits(b)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        raise AssertionError("%s: %d elements differ, first at %s: %s vs %s"
                             % (what, bad.shape[0], bad[0].tolist(), a[tuple(bad[0])].item(), b[tuple(bad[0])].item()))


PER_STEP = ("actions", "dead_mask", "ego_global_pos", "ego_global_rot")
PER_ROW = ("goal_achieved", "off_road", "veh_collision", "goal_step", "off_road_step", "init_goal_dist", "goal_dist", "dead")
LAST_SEEN = ("window", "partner_value", "partner_mask", "road_mask")


def _compare(ep, r, what, record=True):
    """Every output of run() against the reference loop's, bit for bit; the summary against the restatement's float32."""
    for k in (PER_STEP if record else ()) + PER_ROW + LAST_SEEN:
        got, want = getattr(ep, k), r[k]
        if k == "partner_value":
            got = got.to(want.dtype)
        _same(got, want, "%s %s" % (what, k))
    assert int(ep.steps) == r["iterations"], (what, int(ep.steps), r["iterations"])
    got = ep.summary_tensor.cpu().numpy()
    want = r["summary"]
    nan = np.isnan(want)  # (0 / 0 of a row that starts on its goal: IEEE leaves a NaN's sign and payload open, the bits differ by platform)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)), (what, got, want)
    s = ep.summary()
    assert tuple(s) == REF.SUMMARY_NAMES and s["n_rows"] == r["dead"].shape[0] and s["iterations"] == r["iterations"]


_CACHE = {}


def _case(name):
    """One matrix case, computed once: the episode of run(record=True) and the reference loop's outputs on a twin simulator."""
    if name not in _CACHE:
        A, R, model, cb, roads = MATRIX[name]
        from gpudrive_lab_amd import ClosedLoopBC
        with _Env(roads):
            rsim, tsim = _sim(A, model, cb, roads), _sim(A, model, cb, roads)
            try:
                pol = _policy(A, R)
                loop = ClosedLoopBC(rsim, pol)
                ep = loop.run(record=True)
                torch.cuda.synchronize()
                r = _loop(tsim, pol, model, R)
                # after the run: the action tensor's columns 0..2, and who was a live row when they were written
                act = rsim.action_tensor().to_torch()[:, :, :3].clone()
                _CACHE[name] = dict(ep=ep, r=r, N=loop.num_agents, mask=loop.mask.clone(), act=act)
            finally:
                rsim.close()
                tsim.close()
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_run_equals_the_reference_loop(name):
    A, R, model, cb, roads = MATRIX[name]
    c = _case(name)
    ep, r, N = c["ep"], c["r"], c["N"]
    D = 6 + (A - 1) * 6 + 200 * 13
    assert N >= 26 and tuple(ep.window.shape) == (N, R, D) and tuple(ep.actions.shape) == (N, T, 3)
    assert tuple(ep.partner_mask.shape) == (N, A - 1) and tuple(ep.road_mask.shape) == (N, 200)
    print("BC ROLLOUT %s: rows %d steps %d dead %d goal %d off_road %d veh %d summary %s"
          % (name, N, r["iterations"], int(r["dead"].sum()), int(r["goal_achieved"].sum()), int(r["off_road"].sum()),
             int(r["veh_collision"].sum()), r["summary"].tolist()))
    _compare(ep, r, name)
    assert bool((ep.actions != 0).any()) and bool(torch.isfinite(ep.actions).all())
    if R > 1:  # the older frames are the earlier observations, not copies of the newest one
        assert not torch.equal(ep.window[:, R - 1], ep.window[:, R - 2])


def test_the_matrix_meets_the_conditions():
    """Asserted on the REFERENCE loop's outputs, so that no case passes by exercising nothing."""
    rs = {k: _case(k)["r"] for k in MATRIX}
    last = lambda r: r["iterations"] - 1
    assert any(bool(r["dead_mask"][:, :last(r) + 1].any()) for r in rs.values()), "no row dies before the last step"
    assert any(bool((~r["dead_mask"][:, last(r)]).any()) for r in rs.values()), "no row is alive at the last step"
    assert any(bool((r["off_road"] + r["veh_collision"] > 0).any()) for r in rs.values()), "no off-road or collision flag"
    assert any(bool((r["partner_value"] == 1).any() or (r["partner_value"] == 2).any()) for r in rs.values())
    removed = [r for k, r in rs.items() if MATRIX[k][3] == REMOVED]
    assert any(bool(r["dead_mask"][:, 1:last(r) + 1].any()) for r in removed), "HEAD_BIAS_SCALE: no death under REMOVED"


def test_action_zero_fill_under_removed():
    """After a run under REMOVED the action tensor's columns 0..2 are zero in every slot that is not a live row."""
    c = _case("128-5-delta-removed-linear")
    ep, act, mask = c["ep"], c["act"], c["mask"]
    steps = int(ep.steps)
    dead_before_last = ep.dead_mask[:, steps - 1] if steps == T else torch.ones_like(ep.dead_mask[:, 0])
    live = torch.zeros_like(mask)
    live[mask] = ~dead_before_last
    assert bool((~live).any()) and bool((act[~live] == 0).all()), "a slot that is no live row kept an action"
    if steps == T:  # the last iteration ran: its live rows hold the policy's action of that step
        _same(act[live], ep.actions[:, T - 1][~dead_before_last], "live rows' actions")
        assert bool(dead_before_last.any()), "no dead row among the rows: the zero-fill of dead rows is not exercised"


def _goal_sims(scenes):
    return [P.make_gpu_sim(scenes, max_agents=64, knn_order=0, dynamicsModel=2, collisionBehaviour=IGNORE,
                           roadObservationAlgorithm=1, distanceToGoalThreshold=1.0e6, **BASE) for _ in range(2)]


def test_every_agent_reaches_its_goal_at_the_first_step():
    """distanceToGoalThreshold far above every distance: every controlled agent reaches its goal in step 0 and is done with it,
    so the loop breaks after one iteration -- the goal path and the early all-dead `steps`.  (The reference's loop notes a goal
    in the iteration AFTER the step that reached it, simulation.py:61-66; with every row dead that iteration does not exist and
    goal_step stays -1.  The next test keeps the loop running.)"""
    from gpudrive_lab_amd import ClosedLoopBC
    A, R, model = 64, 5, "delta_local"
    rsim, tsim = _goal_sims(SCENES)
    try:
        pol = _policy(A, R)
        ep = ClosedLoopBC(rsim, pol).run(record=True)
        r = _loop(tsim, pol, model, R)
        print("BC ROLLOUT goal: iterations %d goal_step %s" % (r["iterations"], r["goal_step"].tolist()))
        assert r["iterations"] == 1 and bool(r["dead"].all()) and bool((r["goal_achieved"] == 1).all())
        assert r["summary"][2] == 1.0 and r["summary"][4] == 1.0 and r["summary"][7] == 1.0
        _compare(ep, r, "goal at the first step")
        assert bool(ep.dead_mask[:, 1:].all()) and bool((ep.actions[:, 1:] == 0).all())
        ep5 = ClosedLoopBC(rsim, pol).run(n_steps=5)  # four more steps of the simulator change nothing
        for k in PER_ROW:
            _same(getattr(ep5, k), getattr(ep, k), "steps behind the break " + k)
        assert int(ep5.steps) == 1
    finally:
        rsim.close()
        tsim.close()


def test_goal_step_is_one_for_the_agents_that_reach_their_goal_in_step_zero():
    """A threshold in the widest gap of the controlled agents' initial goal distances: the agents below it reach their goal in
    step 0, the others keep the loop running, so iteration 1 exists and notes goal_step == 1 for the former."""
    from gpudrive_lab_amd import ClosedLoopBC
    A, R, model = 64, 5, "delta_local"
    scenes = [TEST_JSON, SCENE_407, SCENE_4]
    probe = _sim(A, model, IGNORE, "linear", scenes=scenes)
    try:
        ctrl = probe.controlled_state_tensor().to_torch().squeeze(-1) == 1
        g = probe.self_observation_tensor().to_torch()[ctrl][:, 4:6].double()
        d = torch.sort(torch.sqrt((g * g).sum(-1))).values.cpu()
    finally:
        probe.close()
    gaps = d[1:] - d[:-1]
    i = int(gaps.argmax())
    assert float(gaps[i]) > 20.0, "no gap wide enough for a step's movement either side: %s" % d.tolist()
    thr = float((d[i] + d[i + 1]) / 2)
    rsim, tsim = (_sim(A, model, IGNORE, "linear", scenes=scenes, goal=thr) for _ in range(2))
    try:
        pol = _policy(A, R)
        ep = ClosedLoopBC(rsim, pol).run(record=True)
        r = _loop(tsim, pol, model, R)
        print("BC ROLLOUT goal in step 0: threshold %.1f (distances %s) iterations %d goal_step %s"
              % (thr, [round(x, 1) for x in d.tolist()], r["iterations"], r["goal_step"].tolist()))
        _compare(ep, r, "goal in step 0")
        assert r["iterations"] > 1 and int((r["goal_step"] == 1).sum()) >= i + 1
        at_once = r["goal_step"] == 1
        assert bool(r["dead_mask"][at_once][:, 1:r["iterations"]].all()) and bool((r["goal_achieved"][at_once] == 1).all())
        assert bool((r["actions"][at_once][:, 1:] == 0).all())
    finally:
        rsim.close()
        tsim.close()


def test_explicit_mask_seven_steps_and_the_draw():
    """One pair of simulators, three runs: an explicit mask with two agents of one world and a slot that is never valid; n_steps
    = 7 as the prefix of the full run; deterministic=False with a seeded generator against the loop fed the same u and z."""
    from gpudrive_lab_amd import ClosedLoopBC
    A, R, model = 64, 5, "delta_local"
    rsim, tsim = _sim(A, model, REMOVED, "linear"), _sim(A, model, REMOVED, "linear")
    try:
        pol = _policy(A, R)
        ctrl = rsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        w = int(ctrl.sum(1).argmax())
        agents = ctrl[w].nonzero().squeeze(1)[:2].tolist()
        assert len(agents) == 2
        n_w = int(rsim.shape_tensor().to_torch()[w, 0])
        assert n_w < A  # slot A - 1 of the world holds no agent
        mask = torch.zeros_like(ctrl)
        mask[w, agents] = True
        mask[w, A - 1] = True
        loop = ClosedLoopBC(rsim, pol, mask=mask)
        assert loop.num_agents == 3 and loop.row_slot.tolist() == [w * A + a for a in agents] + [w * A + A - 1]
        full = loop.run(record=True)
        r = _loop(tsim, pol, model, R, mask=mask)
        _compare(full, r, "explicit mask")
        # the never-valid slot keeps its defaults
        assert int(full.goal_step[2]) == -1 and int(full.off_road_step[2]) == -1
        assert float(full.goal_achieved[2]) == 0 and float(full.off_road[2]) == 0 and float(full.veh_collision[2]) == 0

        K = 7
        part = loop.run(n_steps=K, record=True)
        assert int(part.steps) == min(K, int(full.steps))
        for k in PER_STEP:
            a, b = getattr(part, k), getattr(full, k)
            _same(a[:, :K], b[:, :K], "prefix " + k)
            assert bool((a[:, K:] == (1 if k == "dead_mask" else 0)).all()), "%s: written past n_steps" % k
        _compare(part, _loop(tsim, pol, model, R, mask=mask, n_steps=K), "seven steps")

        all_rows = ClosedLoopBC(rsim, pol)
        g = torch.Generator(device="cuda").manual_seed(5)
        drawn = all_rows.run(deterministic=False, generator=g, record=True)
        N = all_rows.num_agents
        assert tuple(drawn.u.shape) == (T, N) and tuple(drawn.z.shape) == (T, N, 3)
        rd = _loop(tsim, pol, model, R, deterministic=False, u=drawn.u, z=drawn.z)
        _compare(drawn, rd, "the draw")
        det = all_rows.run(record=True)
        assert not torch.equal(det.actions, drawn.actions), "the draw changed nothing"
        g2 = torch.Generator(device="cuda").manual_seed(5)
        _same(all_rows.run(deterministic=False, generator=g2, record=True).actions, drawn.actions, "the same seed")
    finally:
        rsim.close()
        tsim.close()


GUARD = 1 << 12
CANARY_BYTE = 0xA5


class _Carved:
    """run()'s arrays carved from canary-filled byte buffers, GUARD bytes either side."""

    def __init__(self):
        self.whole = {}

    def new(self, name, shape, dtype, fill, device):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((GUARD + n + GUARD,), CANARY_BYTE, dtype=torch.uint8, device=device)
        t = buf[GUARD:GUARD + n].view(dtype).view(shape)
        if fill is not None:
            t.fill_(fill)
        self.whole[name] = (buf, n)
        return t

    def check(self):
        for name, (buf, n) in self.whole.items():
            assert bool((buf[:GUARD] == CANARY_BYTE).all()) and bool((buf[GUARD + n:] == CANARY_BYTE).all()), \
                "bytes beside %s were written" % name


def test_no_host_synchronisation_canaries_and_in_place_following():
    from gpudrive_lab_amd import ClosedLoopBC, DeviceBC
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    A, R, model = 64, 5, "delta_local"
    rsim, tsim = _sim(A, model, REMOVED, "linear"), _sim(A, model, REMOVED, "linear")
    try:
        sd = _state_dict(R)
        bc = DeviceBC(sd, max_agents=A, num_stack=R, batch_size=8, chunk_rows=8, partials=3, **BC.CFG)
        loop = ClosedLoopBC(rsim, bc.policy)
        first = loop.run(record=True)  # (the first step of a simulator may build its launch plan)
        carved = _Carved()
        loop._new = carved.new
        ep = _no_sync(lambda: loop.run(record=True))
        torch.cuda.synchronize()
        carved.check()
        assert set(carved.whole) >= {"window", "partner_mask", "road_mask", "partner_value", "row_actions", "any_alive", "summary",
                                     "actions", "dead_mask", "ego_global_pos", "ego_global_rot", "dead", "goal_dist"}
        for k in PER_STEP + PER_ROW + LAST_SEEN:
            _same(getattr(ep, k), getattr(first, k), "two runs " + k)
        del loop._new

        # one update moves the weights in place; the next run follows them
        obs, pm, rm = first.window[:8].contiguous(), torch.zeros((8, R, A - 1), dtype=torch.bool, device="cuda"), \
            torch.zeros((8, R, 200), dtype=torch.bool, device="cuda")
        pm[:, R - 1], rm[:, R - 1] = first.partner_mask[:8], first.road_mask[:8]
        expert = torch.zeros((8, 1, 3), dtype=torch.float32, device="cuda")
        ptr = bc.policy.blob.data_ptr()
        bc.update(obs, expert, pm, rm)
        assert bc.policy.blob.data_ptr() == ptr
        after = loop.run(record=True)
        fresh = DeviceBCPolicy.from_state_dict(bc.state_dict(), max_agents=A, num_stack=R, chunk_rows=8, **BC.CFG)
        r = _loop(tsim, fresh, model, R)
        _compare(after, r, "after one update")
        assert not torch.equal(after.actions, first.actions), "the weights did not move the actions"
    finally:
        rsim.close()
        tsim.close()


def test_refused_while_only_the_packed_buffer_is_written():
    from gpudrive_lab_amd import ClosedLoopBC
    sim = _sim(64, "delta_local", REMOVED, "linear", scenes=SCENES[:3])
    try:
        loop = ClosedLoopBC(sim, _policy(64, 1))
        assert sim.direct_pack(only=True)
        with pytest.raises(NotImplementedError, match="stale"):
            loop.run()
        assert sim.direct_pack(only=False)
        assert int(loop.run(n_steps=3).steps) == 3
    finally:
        sim.close()


# ---- past one row per lane of the summary

BIG_W = 258  # 258 worlds x 64 slots: more than 256 learner rows, and k_learner_rows scans 16,512 slots, 17 to a lane


@pytest.fixture(scope="module")
def big_twins():
    """Twin simulators of 258 worlds x 64 slots (the three small scenes, 86 times), built once for this module."""
    scenes = [TEST_JSON, SCENE_407, SCENE_4] * (BIG_W // 3)
    assert len(scenes) == BIG_W
    rsim, tsim = (_sim(64, "classic", REMOVED, "linear", scenes=scenes) for _ in range(2))
    yield rsim, tsim
    rsim.close()
    tsim.close()


def test_run_equals_the_reference_loop_on_258_worlds(big_twins):
    """More than 256 rows, and no multiple of 256: lane l of k_bc_summary's 256 adds rows l, l + 256, ..., several terms to a
    lane and one term more in the first lanes than in the last.  Every row draws its own u and z, so the replicas of a scene
    end differently.  The progress sum is a float32 sum of values that are not exactly representable, and it DIFFERS from the
    same sum taken in other orders (asserted below on the reference loop's outputs): the order of bc_rollout_rule.hpp is what
    the summary is held to here."""
    from gpudrive_lab_amd import ClosedLoopBC
    rsim, tsim = big_twins
    A, R, model = 64, 1, "classic"
    pol = _policy(A, R)
    loop = ClosedLoopBC(rsim, pol)
    N = loop.num_agents
    assert N > 256 and N % 256 != 0, N
    g = torch.Generator(device="cuda").manual_seed(5)
    ep = loop.run(deterministic=False, generator=g, record=True)
    r = _loop(tsim, pol, model, R, deterministic=False, u=ep.u, z=ep.z)
    _compare(ep, r, "258 worlds")
    host = lambda k: r[k].cpu().numpy()  # noqa: E731
    # the rows of a world, and what became of them: replicas of one scene must not all end alike
    ctrl = loop.mask.cpu().numpy()
    world_of_row = np.nonzero(ctrl)[0]
    per_world = np.stack([np.bincount(world_of_row, weights=host(k), minlength=BIG_W)
                          for k in ("goal_achieved", "off_road", "veh_collision")], 1)
    differ = [len({tuple(row) for row in per_world[s::3].tolist()}) for s in range(3)]
    assert max(differ) > 1, "the replicas of every scene end alike"
    # the progress sum, as summary() takes it, in the rule's order and in three others
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (host("goal_dist") / host("init_goal_dist")).astype(f32)
    ratio[host("goal_achieved").astype(bool)] = 0
    progress = (f32(1) - ratio).astype(f32)
    assert np.isfinite(progress).all()
    ordered = REF.ordered_sum(progress)

    def serial(v):
        s = f32(0)
        for x in v:
            s = f32(s + x)
        return s

    others = [serial(progress), serial(progress[::-1]), f32(progress.sum(dtype=np.float64))]
    print("BC ROLLOUT 258 worlds: rows %d (%d to a lane, %d lanes one more) iterations %d, distinct outcomes among the replicas %s, "
          "progress sum %r in the rule's order, %s in others" % (N, N // 256, N % 256, r["iterations"], differ, float(ordered),
                                                                  [float(x) for x in others]))
    assert f32(ordered / f32(N)) == r["summary"][4]
    assert any(x != ordered for x in others), "the progress sum is the same in every order: the order would not show"
