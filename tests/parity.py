"""Helpers for the GPU parity suite: build the HIP sim and the oracle on the same scenes and
parameters, and compare every exported tensor.

Tolerances (BASELINE.json north_star): collision/done/info flags and every int tensor bit-exact;
fp32 observations within 1e-5 of the oracle GIVEN IDENTICAL INPUT STATE.  Device libm (OCML) and
host libm (glibc) differ by 1-2 ulp in sinf/cosf/atan2f, and one ulp of a 200 m coordinate is
1.5e-5, so after a free-running dynamics step positions are compared with rtol 1e-6 + atol 1e-5;
observations are compared after the oracle's state has been injected into the HIP engine
(teacher forcing)."""
import numpy as np

from tests.ref_cases import as_np, write_actions

OBS_ATOL = 1e-5
# Observations computed from independently evolved state (before injection): one ulp of a
# quaternion component (cosf/sinf of the half heading, device vs glibc) moves an egocentric
# coordinate at 50 m by ~1.2e-5, so un-injected comparisons use a looser bound.
FREE_OBS_ATOL = 5e-5
# Integer-valued outputs (BASELINE.json north_star: bit-exact).  The BEV cell values and the LiDAR hit / type pattern follow
# from float predicates on sin / cos / atan2 of per-entity headings; the device evaluates those in double and rounds once
# (gd_math.hpp p_sin / p_cos / p_atan2), which equals glibc's float result except where glibc itself is not correctly
# rounded.  The bounds below are the largest counts ever MEASURED on the test cases (printed by every run), not a tolerance
# chosen in advance: 0 means bit-exact on every case.
BEV_MAX_CELLS_OFF = 0
LIDAR_MAX_RAYS_OFF = 0
STATE_RTOL = 1e-6
STATE_ATOL = 1e-5

PARAM_KEYS = ("polylineReductionThreshold", "observationRadius", "rewardType", "distanceToGoalThreshold",
              "distanceToExpertThreshold", "collisionBehaviour", "maxNumControlledAgents", "IgnoreNonVehicles",
              "roadObservationAlgorithm", "initOnlyValidAgentsAtFirstStep", "isStaticAgentControlled",
              "enableLidar", "disableClassicalObs", "dynamicsModel", "readFromTracksToPredict")
ORACLE_ONLY_KEYS = ("enableBev", "lidarHalfAngle")


def make_gpu_sim(scenes, max_agents=64, knn_order=0, enable_bev=False, lidar_half_angle=0.0, sync=None, **kw):
    import madrona_gpudrive as mg
    p = mg.Parameters()
    for k, v in kw.items():
        assert k in PARAM_KEYS, k
        if k in ("rewardType", "distanceToGoalThreshold", "distanceToExpertThreshold"):
            setattr(p.rewardParams, k, v)
        else:
            setattr(p, k, v)
    return mg.SimManager(exec_mode=mg.madrona.ExecMode.CUDA, gpu_id=0, scenes=list(scenes), params=p,
                         max_agents=max_agents, knn_order=knn_order, enable_bev=enable_bev,
                         lidar_half_angle=lidar_half_angle, sync=sync)


def make_oracle_sim(O, scenes, max_agents=64, **kw):
    return O.OracleSim(list(scenes), O.default_params(**kw), max_agents=max_agents)


INT_TENSORS = ["done_tensor", "info_tensor", "steps_remaining_tensor", "shape_tensor", "controlled_state_tensor",
               "response_type_tensor", "metadata_tensor", "deleted_agents_tensor", "map_name_tensor",
               "scenario_id_tensor"]
STATIC_FLOAT_TENSORS = ["expert_trajectory_tensor", "world_means_tensor", "map_observation_tensor"]
OBS_TENSORS = ["reward_tensor", "self_observation_tensor", "absolute_self_observation_tensor",
               "partner_observations_tensor", "agent_roadmap_tensor"]


def _live_mask(orc):
    shape = orc.shape_tensor()
    W, A = orc.W, orc.A
    return np.arange(A)[None, :] < shape[:, 0:1]


def compare_ints(gpu, orc, names=INT_TENSORS):
    for name in names:
        g = as_np(getattr(gpu, name)())
        o = np.asarray(getattr(orc, name)())
        assert g.shape == o.shape, (name, g.shape, o.shape)
        if not np.array_equal(g, o):
            bad = np.argwhere(g != o)
            raise AssertionError("%s differs at %d places, first %s: gpu %s oracle %s" %
                                 (name, len(bad), bad[0], g[tuple(bad[0])], o[tuple(bad[0])]))


def compare_static(gpu, orc):
    for name in STATIC_FLOAT_TENSORS:
        g = as_np(getattr(gpu, name)())
        o = np.asarray(getattr(orc, name)())
        assert np.array_equal(g.view(np.uint32), o.view(np.uint32)), name + " is not bit-identical"


def compare_obs(gpu, orc, atol=OBS_ATOL, rtol=0.0, names=OBS_TENSORS, live_only=("absolute_self_observation_tensor",)):
    live = _live_mask(orc)
    for name in names:
        g = as_np(getattr(gpu, name)())
        o = np.asarray(getattr(orc, name)())
        assert g.shape == o.shape, (name, g.shape, o.shape)
        if name in live_only:  # rows of padding agents are never written by the reference
            g = g[live]
            o = o[live]
        if name == "absolute_self_observation_tensor":
            ok = np.isclose(g, o, atol=atol, rtol=max(rtol, STATE_RTOL))
        else:
            ok = np.isclose(g, o, atol=atol, rtol=rtol)
        if not ok.all():
            bad = np.argwhere(~ok)
            raise AssertionError("%s: %d elements beyond atol %g; first at %s gpu %r oracle %r" %
                                 (name, len(bad), atol, bad[0], g[tuple(bad[0])], o[tuple(bad[0])]))


def compare_state(gpu, orc):
    gs = gpu.debug_get_state()
    os_ = orc.get_state()
    live = _live_mask(orc)
    assert np.array_equal(gs[..., 10][live], os_[..., 10][live]), "collided flags differ"
    g = gs[live][:, :10]
    o = os_[live][:, :10]
    ok = np.isclose(g, o, rtol=STATE_RTOL, atol=STATE_ATOL)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError("agent state differs: %d elements, first %s gpu %r oracle %r" %
                             (len(bad), bad[0], g[tuple(bad[0])], o[tuple(bad[0])]))


def random_actions(rng, W, A, model):
    """Seeded U(-3,2) x U(-0.7,0.7) (reference src/headless.cpp:69-70); deltas / states for the
    other models."""
    act = np.zeros((W, A, 10), np.float32)
    if model in (0, 1):
        act[..., 0] = rng.uniform(-3.0, 2.0, (W, A))
        act[..., 1] = rng.uniform(-0.7, 0.7, (W, A))
    elif model == 2:
        act[..., 0] = rng.uniform(-0.5, 1.5, (W, A))
        act[..., 1] = rng.uniform(-0.2, 0.2, (W, A))
        act[..., 2] = rng.uniform(-0.1, 0.1, (W, A))
    else:
        act[..., 0] = rng.uniform(-60, 60, (W, A))
        act[..., 1] = rng.uniform(-60, 60, (W, A))
        act[..., 2] = 1.0
        act[..., 3] = rng.uniform(-3.1, 3.1, (W, A))
        act[..., 4] = rng.uniform(-8, 8, (W, A))
        act[..., 5] = rng.uniform(-8, 8, (W, A))
    return act


def inject_and_compare(gpu, orc):
    """Copy the oracle's agent state into the HIP engine, recompute both through the Reset graph
    (no movement, no decrement) and require every observation within 1e-5, ints exact."""
    gpu.debug_set_state(orc.get_state())
    gpu.reset([])
    orc.reset([])
    compare_ints(gpu, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
    compare_obs(gpu, orc)


def compare_fresh(gpu, orc):
    """After construction / reset / set_maps: ints and init-time rows exact, state close,
    observations within the un-injected bound, then the strict injected comparison."""
    compare_ints(gpu, orc)
    compare_static(gpu, orc)
    compare_state(gpu, orc)
    compare_obs(gpu, orc, atol=FREE_OBS_ATOL)
    inject_and_compare(gpu, orc)


def lockstep(gpu, orc, steps, model, seed=0, teacher_force=True, check_every=1):
    """Step both simulators on the same seeded actions.  After every step: int tensors exact, agent
    state close; then the oracle's state is injected into the HIP engine, both recompute through
    the Reset graph (no movement, no decrement) and all observations must agree to 1e-5."""
    rng = np.random.default_rng(seed)
    W, A = orc.W, orc.A
    for k in range(steps):
        act = random_actions(rng, W, A, model)
        write_actions(gpu, act)
        np.copyto(orc.action_tensor(), act)
        gpu.step()
        orc.step()
        if k % check_every:
            continue
        try:
            compare_ints(gpu, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
            compare_state(gpu, orc)
            if teacher_force:
                inject_and_compare(gpu, orc)
        except AssertionError as e:
            raise AssertionError("step %d: %s" % (k + 1, e))


def _sorted_rows(x):
    """Sort the 200 road rows of every agent lexicographically (set comparison)."""
    flat = x.reshape(-1, x.shape[-2], x.shape[-1])
    out = np.empty_like(flat)
    for i in range(flat.shape[0]):
        r = flat[i]
        # padding rows (type 0) last; real rows by their ego-frame (x, y), which both sides compute
        # with the same IEEE mul/add sequence (bit-identical given identical injected state)
        key = np.lexsort((r[:, 7], r[:, 1], r[:, 0], -(r[:, 6] != 0).astype(np.int8)))
        out[i] = r[key]
    return out.reshape(x.shape)


def compare_roadmap_as_set(gpu, orc, atol=OBS_ATOL):
    """GD_KNN_SET_ORDER: same rows as the reference, any order."""
    g = _sorted_rows(as_np(gpu.agent_roadmap_tensor()))
    o = _sorted_rows(np.asarray(orc.agent_roadmap_tensor()))
    ok = np.isclose(g, o, atol=atol, rtol=0)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError("agent_roadmap (as a set): %d elements differ; first at %s gpu %r oracle %r" %
                             (len(bad), bad[0], g[tuple(bad[0])], o[tuple(bad[0])]))


def compare_lidar(gpu, orc, depth_atol=1e-4):
    """LiDAR rows of live agents: hit/miss pattern and entity type exact, depth and hit position
    within 1e-4 (200 m range; ray directions come from sin/cos of the ray angle)."""
    live = _live_mask(orc)
    g = as_np(gpu.lidar_tensor())[live]
    o = np.asarray(orc.lidar_tensor())[live]
    hit_g, hit_o = g[..., 0] > 0, o[..., 0] > 0
    # a ray grazing a box corner may hit on one side only: allow a vanishing fraction
    mism = (hit_g != hit_o) | (g[..., 1] != o[..., 1])
    print("lidar: hit/type pattern differs on %d of %d rays" % (mism.sum(), mism.size))
    assert mism.sum() <= LIDAR_MAX_RAYS_OFF, "lidar hit/type pattern differs on %d of %d rays" % (mism.sum(), mism.size)
    ok = ~mism
    assert np.allclose(g[ok][:, [0, 2, 3]], o[ok][:, [0, 2, 3]], atol=depth_atol, rtol=1e-5)
    return float(hit_o.mean())


def compare_bev(gpu, orc):
    """BEV grids of live agents: cell values are entity types; cells whose centre lies within float
    rounding of a rectangle edge may differ (device vs host sin/cos), nothing else."""
    live = _live_mask(orc)
    g = as_np(gpu.bev_observation_tensor())[live]
    o = np.asarray(orc.bev_observation_tensor())[live]
    mism = g != o
    print("bev: %d of %d cells differ" % (mism.sum(), mism.size))
    assert mism.sum() <= BEV_MAX_CELLS_OFF, "BEV differs on %d of %d cells" % (mism.sum(), mism.size)
    return float((o != 0).mean())


# ---- the packed observation (packed_observations() / gd_attach_packed) restated in float64 ----
def _nm(x):
    return 2 * ((x + 1000) / 2000) - 1


def pack_observation_f64(self_obs, partner, roadmap):
    """GPUDriveTorchEnv.get_obs() with norm_obs: ego (6) | partners ((A-1) x 6) | road points (200 x 13), from the raw
    [..., 8] self, [..., A-1, 9] partner and [..., 200, 9] road rows, in float64 (tests/golden/obs_pack_golden.npz pins it to
    the reference's own gpudrive/datatypes code)."""
    so = np.asarray(self_obs, np.float64)
    po = np.asarray(partner, np.float64)
    ro = np.asarray(roadmap, np.float64)
    ego = np.stack([so[..., 0] / 100, so[..., 1] * 0.7 / 30, so[..., 2] * 0.7 / 15, _nm(so[..., 4]), _nm(so[..., 5]),
                    so[..., 6]], -1)
    part = np.stack([po[..., 0] / 100, _nm(po[..., 1]), _nm(po[..., 2]), po[..., 3] / (2 * np.pi), po[..., 4] * 0.7 / 30,
                     po[..., 5] * 0.7 / 15], -1).reshape(po.shape[:-2] + (-1,))
    one_hot = (ro[..., 6:7] == np.arange(7)).astype(np.float64)
    road = np.concatenate([_nm(ro[..., 0:1]), _nm(ro[..., 1:2]), ro[..., 2:5] / 100, ro[..., 5:6] / (2 * np.pi), one_hot],
                          -1).reshape(ro.shape[:-2] + (-1,))
    return np.concatenate([ego, part, road], -1)


def pack_column_gain(A):
    """|d packed column / d raw input| for every column of the packed observation: how far a raw difference moves it (the
    one-hot road type follows an integer-valued column that is compared exactly)."""
    ego = [1 / 100, 0.7 / 30, 0.7 / 15, 1e-3, 1e-3, 1.0]
    part = [1 / 100, 1e-3, 1e-3, 1 / (2 * np.pi), 0.7 / 30, 0.7 / 15] * (A - 1)
    road = ([1e-3, 1e-3, 1 / 100, 1 / 100, 1 / 100, 1 / (2 * np.pi)] + [0.0] * 7) * 200
    return np.asarray(ego + part + road, np.float64)


# The packed kernel divides / multiplies in fp32: against a float64 restatement of the same raw rows it is within a couple of
# ulps of a [-1, 1] value.
PACK_ATOL = 3e-7
PACK_RTOL = 1e-6


def compare_packed(got, self_obs, partner, roadmap, raw_atol=0.0, what="packed observation"):
    """`got` [W, A, D] against pack_observation_f64 of the raw rows; raw_atol is how far those raw rows may be from the ones
    the kernel packed (OBS_ATOL when they are the oracle's), carried through every column's gain."""
    got = np.asarray(got, np.float64)
    want = pack_observation_f64(self_obs, partner, roadmap)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    atol = PACK_ATOL + raw_atol * pack_column_gain((got.shape[-1] - 6 - 200 * 13) // 6 + 1)
    ok = np.abs(got - want) <= atol + PACK_RTOL * np.abs(want)
    if not ok.all():
        bad = np.argwhere(~ok)
        raise AssertionError("%s: %d elements off, first at %s got %r want %r" %
                             (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))
    return got.size


# ---- drift-free lockstep: the State model (dynamicsModel = 3) on scripted actions ----
RESP_STATIC = 2
PAD_Z = np.float32(np.finfo(np.float32).max)   # kPaddingPosition's z (reference src/consts.hpp:64)
_LIBM = None


def _host_sincos(x):
    global _LIBM
    if _LIBM is None:
        import ctypes
        import ctypes.util
        _LIBM = ctypes.CDLL(ctypes.util.find_library("m"))
        for f in (_LIBM.sinf, _LIBM.cosf):
            f.restype = ctypes.c_float
            f.argtypes = [ctypes.c_float]
    return np.float32(_LIBM.sinf(float(x))), np.float32(_LIBM.cosf(float(x)))


def yaw_rotation_agrees(yaw):
    """Both sides store q_angle_axis_up(yaw) = (cos(yaw / 2), 0, 0, sin(yaw / 2)): the oracle with the host's sinf / cosf, the
    device in double rounded once (gd_math.hpp p_sincos).  True when the two give the same bits for this yaw."""
    half = np.float32(np.float32(yaw) / np.float32(2))
    s, c = _host_sincos(half)
    return s == np.float32(np.sin(np.float64(half))) and c == np.float32(np.cos(np.float64(half)))


def agreeing_yaw(yaw):
    """The float32 nearest `yaw` (stepping up ulp by ulp) whose rotation both sides compute bit for bit."""
    y = np.float32(yaw)
    for _ in range(64):
        if yaw_rotation_agrees(y):
            return y
        y = np.nextafter(y, np.float32(np.inf))
    raise AssertionError("no yaw near %r rotates alike on both sides" % yaw)


class StateScript:
    """Scripted State-model actions (position, yaw, velocity written straight into the body on both sides, reference
    src/dynamics.hpp:186-194): every controlled agent is handed back its own pose -- its pose bits do not change, so the
    engine may leave its rows in place -- except a few per step that are shifted or turned, and, on `hit` steps, one controlled
    agent per world that is put on top of a parked (Static) car.  The yaw the script last gave every agent is kept on the host
    (after a reset: the expert heading at t = 0, what the reset writes) so that "its own pose" is bit for bit the pose it has."""

    def __init__(self, orc):
        self.orc = orc
        self.reseed(range(orc.W))

    def reseed(self, worlds):
        if not hasattr(self, "yaw") or self.yaw.shape != (self.orc.W, self.orc.A):
            self.yaw = np.zeros((self.orc.W, self.orc.A), np.float32)
        traj = np.asarray(self.orc.expert_trajectory_tensor())
        for w in worlds:
            self.yaw[w] = traj[w, :, 4 * 91]

    def hit_pairs(self, worlds):
        """(world, controlled agent, parked agent) for every listed world that has both: a controlled agent that is not done, a
        parked one that has not collided nor been removed (a parked car is done from its first step on -- its goal is where it
        stands -- and still collides: isInvalidExpertOrDone looks at a non-controlled agent's log only, src/sim.cpp:631-662)."""
        st = self.orc.get_state()
        n = np.asarray(self.orc.shape_tensor())[:, 0]
        resp = np.asarray(self.orc.response_type_tensor())[..., 0]
        ctl = np.asarray(self.orc.controlled_state_tensor())[..., 0]
        done = np.asarray(self.orc.done_tensor())[..., 0]
        pairs = []
        for w in worlds:
            ok = [a for a in range(n[w]) if st[w, a, 2] != PAD_Z and st[w, a, 10] == 0]
            parked = [a for a in ok if resp[w, a] == RESP_STATIC]
            movers = [a for a in ok if resp[w, a] != RESP_STATIC and ctl[w, a] and done[w, a] == 0]
            if parked and movers:
                pairs.append((w, movers[0], parked[0]))
        return pairs

    def actions(self, k, hits=()):
        st = self.orc.get_state()
        W, A = self.orc.W, self.orc.A
        act = np.zeros((W, A, 10), np.float32)
        act[..., 0:3] = st[..., 0:3]
        act[..., 4:7] = st[..., 7:10]
        act[..., 2] = np.where(st[..., 2] == 0, np.float32(1), st[..., 2])
        yaw = self.yaw.copy()
        a_idx = np.arange(A)
        for w in range(W):
            shift = (a_idx + k) % 5 == 0
            act[w, shift, 0] += np.float32(0.25)
            act[w, shift, 1] -= np.float32(0.15)
            for a in np.nonzero((a_idx + k) % 7 == 3)[0]:
                yaw[w, a] = agreeing_yaw(np.float32(yaw[w, a] + np.float32(0.05)))
        for w, c, s in hits:
            act[w, c, 0:3] = st[w, s, 0:3]
            act[w, c, 4:7] = 0.0
            yaw[w, c] = agreeing_yaw(self.yaw[w, s])
        act[..., 3] = yaw
        # the yaw every controlled agent that is still driving is given becomes the yaw it has
        ctl = np.asarray(self.orc.controlled_state_tensor())[..., 0] != 0
        moving = ctl & (np.asarray(self.orc.done_tensor())[..., 0] == 0) & \
            (np.asarray(self.orc.response_type_tensor())[..., 0] != RESP_STATIC)
        self.yaw[moving] = yaw[moving]
        return act


def compare_state_bits(gpu, orc, yaw=None):
    """Every live agent's state (position, rotation, velocity, collided) bit for bit: the precondition of comparing a step's
    observations without injection.  A differing rotation is reported with the yaw the script gave that agent."""
    gs = gpu.debug_get_state()
    os_ = orc.get_state()
    live = _live_mask(orc)
    g, o = gs.view(np.uint32), os_.view(np.uint32)
    bad = np.argwhere((g != o).any(-1) & live)
    if len(bad):
        w, a = bad[0]
        raise AssertionError("state not bit-identical for %d agents; first (world %d, agent %d): gpu %r oracle %r, scripted yaw %r" %
                             (len(bad), w, a, gs[w, a].tolist(), os_[w, a].tolist(),
                              None if yaw is None else float(yaw[w, a])))
    return int(live.sum()) * 11


def scripted_state_lockstep(gpu, orc, steps, events=None, roads_as_set=False, pack=None, bev=False, lidar=False,
                            skipping=True):
    """Step the HIP engine and the oracle on the same StateScript actions and hold the outputs OF EVERY STEP to the oracle --
    no injection, so the step passes (pose stamps, the linear scan's step list, BEV / LiDAR dirty flags, the direct pack) are
    what is compared.  After every step: int tensors exact; agent state bit-exact (asserted first: it is the precondition);
    reward, self / absolute / partner rows and road rows within OBS_ATOL (road rows as a set in set order); BEV cells and
    LiDAR returns (compare_bev / compare_lidar) when enabled; the packed observation (pack = "both" / "only": attached with
    the raw rows kept / not) against the float64 pack of the oracle's rows.

    events: {step index: [(kind, arg), ...]} -- ("hit", worlds) before that step puts a controlled agent of each world on a
    parked car; ("reset", worlds), ("set_maps", scenes), ("delete", {world: [agent slots]}) after it, on both simulators, and
    that state is compared at once.  Returns a dict of counts: steps, elements compared, rows skipped (gd_stat 30), parked
    cars whose collided flag the oracle set, parked cars the oracle moved to the padding position."""
    from tests.ref_cases import write_actions
    events = events or {}
    script = StateScript(orc)
    out = dict(steps=0, elements=0, skipped=0, parked_hit=0, parked_removed=0)
    gpu.stat(30)
    obs = ["reward_tensor", "self_observation_tensor", "absolute_self_observation_tensor"]
    if pack != "only":
        obs.append("partner_observations_tensor")

    def check(tag):
        try:
            n = compare_state_bits(gpu, orc, script.yaw)
            compare_ints(gpu, orc)
            n += sum(np.asarray(getattr(orc, t)()).size for t in INT_TENSORS)
            compare_obs(gpu, orc, names=obs)
            n += sum(np.asarray(getattr(orc, t)()).size for t in obs)
            if pack != "only":
                if roads_as_set:
                    compare_roadmap_as_set(gpu, orc)
                else:
                    compare_obs(gpu, orc, names=["agent_roadmap_tensor"])
                n += np.asarray(orc.agent_roadmap_tensor()).size
            if bev:
                compare_bev(gpu, orc)
                n += int(_live_mask(orc).sum()) * 200 * 200
            if lidar:
                compare_lidar(gpu, orc)
                n += int(_live_mask(orc).sum()) * 3 * 50 * 4
            if pack is not None:
                assert not roads_as_set, "the packed road columns are compared in the reference's row order"
                got = gpu.packed_observations().cpu().numpy()
                n += compare_packed(got, orc.self_observation_tensor(), orc.partner_observations_tensor(),
                                    orc.agent_roadmap_tensor(), raw_atol=OBS_ATOL)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tag, e))
        out["elements"] += n

    for k in range(steps):
        hits = []
        for kind, arg in events.get(k, []):
            if kind == "hit":
                hits += script.hit_pairs(arg)
        assert not any(kind == "hit" for kind, _ in events.get(k, [])) or hits, "step %d: no parked car to hit" % (k + 1)
        act = script.actions(k, hits)
        write_actions(gpu, act)
        np.copyto(orc.action_tensor(), act)
        gpu.step()
        orc.step()
        out["steps"] += 1
        st = orc.get_state()
        parked = (np.asarray(orc.response_type_tensor())[..., 0] == RESP_STATIC) & _live_mask(orc)
        out["parked_hit"] += int((parked & (st[..., 10] != 0)).sum())
        out["parked_removed"] += int((parked & (st[..., 2] == PAD_Z)).sum())
        check("step %d" % (k + 1))
        for kind, arg in events.get(k, []):
            if kind == "reset":
                gpu.reset(list(arg))
                orc.reset(list(arg))
                script.reseed(arg)
            elif kind == "set_maps":
                gpu.set_maps(list(arg))
                orc.set_maps(list(arg))
                script.reseed(range(orc.W))
            elif kind == "delete":
                ids = np.asarray(orc.agent_id_tensor())
                victims = {w: [int(ids[w, a]) for a in slots] for w, slots in arg.items()}
                gpu.deleteAgents(victims)
                orc.deleteAgents(victims)
                script.reseed(range(orc.W))
            else:
                assert kind == "hit", kind
                continue
            check("after the %s behind step %d" % (kind, k + 1))
    out["skipped"] = gpu.stat(30)
    if skipping:
        assert out["skipped"] > 0, "no road rows were left in place: the skip paths did not run"
    return out


def parked_car_scene(directory, name="parked_car"):
    """A synthetic world for the skip paths' hard case: a controlled car (its expert trajectory moves, so it is Dynamic) driving
    towards two parked cars (trajectories still, goal on the spot: Static under isStaticAgentControlled = 0, reference
    src/level_gen.cpp:102-113) between two wavy road edges and along a lane -- roads in reach of every car."""
    import json
    import os

    def car(i, xs, ys, yaw, goal):
        return {"position": [{"x": x, "y": y, "z": 0.0} for x, y in zip(xs, ys)], "width": 2.0, "length": 4.5, "height": 1.6,
                "heading": [yaw] * 91, "velocity": [{"x": 5.0 if xs[0] != xs[-1] else 0.0, "y": 0.0}] * 91,
                "valid": [True] * 91, "goalPosition": {"x": goal[0], "y": goal[1], "z": 0.0}, "type": "vehicle", "id": i,
                "mark_as_expert": False}

    def line(y0, amp, kind, rid):
        return {"geometry": [{"x": 60.0 + 2.0 * k, "y": y0 + amp * np.sin(0.3 * k), "z": 0.0} for k in range(50)], "type": kind,
                "map_element_id": {"road_edge": 15, "lane": 2}[kind], "id": rid}

    drive = [80.0 + 0.5 * k for k in range(91)]
    sc = {"name": name, "scenario_id": name,
          "objects": [car(0, drive, [50.0] * 91, 0.0, (200.0, 50.0)),
                      car(1, [100.0] * 91, [50.5] * 91, 0.3, (100.0, 50.5)),
                      car(2, [112.0] * 91, [55.0] * 91, 1.2, (112.0, 55.0))],
          "roads": [line(44.0, 0.6, "road_edge", 0), line(58.0, 0.6, "road_edge", 1), line(51.0, 0.3, "lane", 2)],
          "tl_states": {}, "metadata": {"sdc_track_index": 0, "objects_of_interest": [], "tracks_to_predict": []}}
    path = os.path.join(str(directory), name + ".json")
    with open(path, "w") as f:
        json.dump(sc, f)
    return path
