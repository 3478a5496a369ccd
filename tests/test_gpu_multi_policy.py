"""GPU suite: the multi-policy evaluator.

`gd_owned_rows` must give the numpy restatement's segmented list; `gd_policy_forward_owned` must give every listed row the bits
of its OWNER's full forward and touch nothing else; `ClosedLoopMultiPPO.run()` must give what the reference's loop gives
(tests/multi_policy_reference.closed_loop: gpudrive/utils/multi_policy_rollout.py:36-169 in torch, a `DevicePolicy` per policy
called on next_obs[mask_p & live]) on a twin simulator fed the same u.  Everything here is an exact comparison: float32 viewed
as int32, NaN matched as NaN, no tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import multi_policy_reference as MREF
from tests import policy_cases as PC
from tests import ppo_rollout_reference as REF
from tests.test_gpu_live_rows import CANARY, F_CANARY, _bits, _Carver
from tests.test_gpu_policy import _no_sync
from tests.test_gpu_ppo_rollout import (BIG_W, MATRIX, PER_ROW, PER_STEP, REMOVED, SCENES, WORLD, T, _Carved, _Env, _same, _sim, _table)
from tests.test_gpu_ppo_rollout import big_twins  # noqa: F401 (the module-scoped fixture: twin simulators of 258 worlds)

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)  # the weights of policies "a", "b", "c": tests/policy_cases.state_dict(seed, ego_width, n_actions)
NAMES = ("a", "b", "c")
SEEDS8 = SEEDS + (14, 15, 16, 17, 18)  # GD_POLICY_SET_MAX policies: the first three are a, b, c
NAMES8 = NAMES + ("d", "e", "f", "g", "h")


# ---- gd_owned_rows against the numpy restatement
_patterns = MREF.list_patterns  # name -> (mask uint8 [n], owner uint8 [n])


def _check_owned_rows(what, mask, owner, n, P, lr, carver, dev):
    """One list against the restatement: counts, starts, every position, the padding, the canary past start[P], the guards,
    two calls equal, and at P = 1 gd_live_rows' list."""
    from gpudrive_lab_amd.policy import LiveRows, live_rows, owned_rows
    rows, start, count = MREF.owned_list(mask, owner, P, CANARY)
    carver.refill()
    m, o = torch.from_numpy(mask).cuda(), torch.from_numpy(owner).cuda()
    assert owned_rows(m, o, out=lr) is lr
    carver.check(what)
    assert lr.count.cpu().tolist() == count.tolist(), (what, lr.count.tolist(), count.tolist())
    got_start = lr.start.cpu().numpy()
    assert got_start.tolist() == start.tolist() and (got_start % 32 == 0).all(), (what, got_start, start)
    got = lr.rows.cpu().numpy()
    assert np.array_equal(got, rows), "%s: first difference at position %d" % (what, int(np.nonzero(got != rows)[0][0]))
    for p in range(P):
        seg = got[start[p]:start[p] + count[p]]
        assert (np.diff(seg) > 0).all() and (got[start[p] + count[p]:start[p + 1]] == -1).all(), what
    assert (got[start[P]:] == CANARY).all(), what + ": positions at or past start[P] were written"
    first = [t.clone() for t in (lr.rows, lr.start, lr.count, lr.scratch)]
    owned_rows(m, o, out=lr)
    for a, b in zip(first, (lr.rows, lr.start, lr.count, lr.scratch)):
        assert torch.equal(a, b), what + ": two calls differ"
    if P == 1:
        live = live_rows(m * (o == 0), out=LiveRows(n, dev))  # (a stranger's row is listed nowhere)
        k = int(live.count)
        assert k == int(count[0]) and torch.equal(live.rows[:k], lr.rows[:k]), what + ": not gd_live_rows' list"
    return count


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_owned_rows_equals_the_restatement(P):
    from gpudrive_lab_amd.policy import OwnedRows, owned_rows
    rng = np.random.default_rng(100 + P)
    dev = torch.device("cuda", torch.cuda.current_device())
    for n in (1, 31, 32, 33, 1023, 1024, 1025, 2100):
        carver = _Carver()
        lr = OwnedRows(n, P, dev, new=carver.new)
        assert lr.rows.numel() == n + 32 * P and lr.scratch.numel() == P * -(-n // 1024) and lr.start.numel() == P + 1
        assert OwnedRows.nbytes(n, P) == 4 * sum(t.numel() for t in (lr.rows, lr.start, lr.count, lr.scratch))
        for name, (mask, owner) in _patterns(n, P, rng).items():
            _check_owned_rows("n=%d P=%d %s" % (n, P, name), mask, owner, n, P, lr, carver, dev)
        if n == 1025:
            m, o = (torch.from_numpy(t).cuda() for t in _patterns(n, P, rng)["alternating"])
            fresh = owned_rows(m.view(torch.bool), o, P)  # without out=: a fresh list, the same values
            _no_sync(lambda: owned_rows(m, o, out=lr))
            assert torch.equal(fresh.count, lr.count) and torch.equal(fresh.start, lr.start)
            end = int(fresh.start[P])
            assert torch.equal(fresh.rows[:end], lr.rows[:end])
            with pytest.raises(ValueError, match="out must be an OwnedRows"):
                owned_rows(m, o, out=OwnedRows(n - 1, P, dev))


MANY_BLOCKS = (262144, 262145, 1 << 20)  # 256 blocks: one term per lane; 257: lane 0 alone adds a second; 1024: four per lane


@pytest.mark.parametrize("n", MANY_BLOCKS)
@pytest.mark.parametrize("P", [1, 8])
def test_owned_rows_at_more_blocks_than_lanes(P, n):
    """k_owned_write adds up the blocks' counts with `for (i = tid; i < blocks; i += 256)`: above 256 blocks a lane takes a
    second trip, with the split `i < block` inside it and the stride p * blocks at P = 8.  The patterns of the small sizes, and
    `late` (owner P - 1 only in blocks >= 256: a total without the second trip gives it no rows and moves every later start)
    and `straddle` (owner 0 in blocks 255, 256 and the last only: `before` at block 256 and at blocks - 1); that they are what
    they are named for is asserted here on the inputs.  tests/test_multi_policy.py shows that a restatement with either fault
    differs on them."""
    from gpudrive_lab_amd.policy import OwnedRows
    rng = np.random.default_rng(1000 * P + n % 1000)
    dev = torch.device("cuda", torch.cuda.current_device())
    blocks = -(-n // 1024)
    assert blocks == {262144: 256, 262145: 257, 1 << 20: 1024}[n]
    carver = _Carver()
    lr = OwnedRows(n, P, dev, new=carver.new)
    assert lr.scratch.numel() == P * blocks
    cases = dict(_patterns(n, P, rng), **MREF.many_block_patterns(n, P, rng))
    blk = np.arange(n) // 1024
    for name, (mask, owner) in cases.items():
        count = _check_owned_rows("n=%d P=%d %s" % (n, P, name), mask, owner, n, P, lr, carver, dev)
        if name == "late":
            mine = (mask != 0) & (owner == P - 1)
            assert (blk[mine] >= 256).all() and int(count[P - 1]) == int(mine.sum()) and (count[P - 1] > 0) == (blocks > 256)
            assert P == 1 or ((blk[(mask != 0) & (owner < P - 1)] < 256).all() and (count[:P - 1] > 0).all())
        if name == "straddle":
            at = set(blk[(mask != 0) & (owner == 0)].tolist())
            assert at == {b for b in (255, 256, blocks - 1) if b < blocks}, at
            assert P == 1 or (count[1:] > 0).all()


# ---- the forward on an owned list against every owner's full forward
_owner_patterns = MREF.owner_patterns  # name -> (mask bool [n], owner uint8 [n])


def _canaries(n, na):
    f = torch.float32
    ints = lambda shape: torch.full(shape, F_CANARY, dtype=torch.int32, device="cuda")  # noqa: E731
    return (torch.full((n,), F_CANARY, dtype=torch.int64, device="cuda"),) + tuple(ints((n,)).view(f) for _ in range(3)), \
        ints((n, na)).view(f)


def _check_owned(what, mask, owner, P, got, got_logits, full):
    """Every listed row against ITS owner's full forward, every other row against the canary."""
    listed = torch.from_numpy(mask & (owner < P)).cuda()
    own = torch.from_numpy(owner.astype(np.int64)).cuda()
    for i, name in enumerate(("actions", "logprob", "entropy", "value", "logits")):
        g = _bits(got_logits if i == 4 else got[i])
        for p in range(P):
            rows = listed & (own == p)
            w = _bits(full[p][1] if i == 4 else full[p][0][i])
            assert torch.equal(g[rows], w[rows]), "%s: %s of a row of policy %d differs from that policy's full forward" % (what, name, p)
        assert bool((g[~listed] == F_CANARY).all()), "%s: %s of a row that is not listed was written" % (what, name)


N_EIGHT = 140  # the smallest n that holds the eight segment sizes 33, 32, 1, 0, 33, 32, 1, 0 (132 rows) and some dead rows


@pytest.mark.parametrize("a,ew,na,n", [(64, 6, 91, 1), (64, 6, 91, 33), (64, 6, 91, 70), (64, 6, 91, 1100), (128, 9, 91, 70),
                                       (128, 9, 91, 1100), (64, 6, 5, 70), (64, 6, 91, N_EIGHT), (128, 9, 91, N_EIGHT)])
def test_forward_on_an_owned_list_equals_each_owners_full_forward(a, ew, na, n):
    """n = N_EIGHT runs P = 5 and P = 8 (the other sizes 1, 2 and 3): `OwnedList.blob[3 .. 7]` choose weights, an empty segment
    lies between two full ones behind position 96, and segments of index >= 3 have a 32-row and a 1-row tail workgroup, in
    every rotation of the sizes over the owners."""
    from gpudrive_lab_amd.policy import DevicePolicy, LiveRows, OwnedRows, PolicySet, live_rows, owned_rows
    rng = np.random.default_rng(7 * n + a)
    obs = torch.from_numpy(PC.observations(20 + n + a, n, a, ew)).cuda()
    u = torch.from_numpy(PC.uniforms(n + 3, n)).cuda()
    eight = n == N_EIGHT
    assert not eight or n >= sum(MREF.OWNER_SIZES) > n - 32
    pols = [DevicePolicy.from_state_dict(PC.state_dict(s, ew, na), max_agents=a, ego_width=ew) for s in (SEEDS8 if eight else SEEDS)]
    full = {}
    for det in (False, True):
        full[det] = []
        for pol in pols:
            logits = torch.empty((n, na), device="cuda")
            full[det].append((pol(obs, None if det else u, deterministic=det, logits_out=logits), logits))
    for i in range(len(pols)):
        for j in range(i):  # on every row, so that a row given another policy's weights shows whichever row it is
            assert bool((_bits(full[True][i][1]) != _bits(full[True][j][1])).any(1).all()), \
                "policies %d and %d give a row the same logits: a mix-up of weights would not show" % (j, i)
    out, logits_out = _canaries(n, na)
    dev = obs.device
    for P in ((5, 8) if eight else (1, 2, 3)):
        ps = PolicySet(pols[:P])
        lr = OwnedRows(n, P, dev)
        for name, (mask, owner) in _owner_patterns(n, P, rng).items():
            what = "A=%d ego=%d NA=%d N=%d P=%d %s" % (a, ew, na, n, P, name)
            m, o = torch.from_numpy(mask).cuda(), torch.from_numpy(owner).cuda()
            owned_rows(m, o, out=lr)
            if eight and P == 8 and name.startswith("blocks"):  # what the case is for, on the device's own list
                shift, count, start = int(name[6:]), lr.count.tolist(), lr.start.tolist()
                assert count == [MREF.OWNER_SIZES[(p + shift) % 8] for p in range(8)], (what, count)
                assert any(count[p] == 0 and start[p] > 96 and count[p - 1] > 0 and count[p + 1] > 0 for p in range(3, 7)), \
                    (what, "no empty segment of index >= 3 between two full ones behind position 96")
                assert any(count[p] == 32 for p in range(3, 8)) and any(count[p] == 33 for p in range(3, 8))
            for det in (False, True):
                for t in out + (logits_out,):
                    _bits(t).fill_(F_CANARY)
                got = ps(obs, lr, None if det else u, deterministic=det, out=out, logits_out=logits_out)
                assert all(g is x for g, x in zip(got, out))
                _check_owned(what + (" det" if det else ""), mask, owner, P, got, logits_out, full[det])
            if P == 1 and name == "random-with-strangers":  # the same list through gd_policy_forward_rows
                rows_out, rows_logits = _canaries(n, na)
                pols[0](obs, deterministic=True, out=rows_out, logits_out=rows_logits,
                        rows=live_rows(m & (o == 0), out=LiveRows(n, dev)))
                for g, w in zip(got + (logits_out,), rows_out + (rows_logits,)):
                    assert torch.equal(_bits(g), _bits(w)), what + ": differs from gd_policy_forward_rows"
        # no host synchronisation and no allocation with out= and a reused list
        m, o = (torch.from_numpy(t).cuda() for t in _owner_patterns(n, P, rng)["alternating"])
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        _no_sync(lambda: ps(obs, owned_rows(m, o, out=lr), u, out=out, logits_out=logits_out))
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before, "the call allocated"
        fresh = ps(obs, lr, u)
        for p in range(P):
            rows = o == p
            for g, w in zip(fresh, full[False][p][0]):
                assert torch.equal(g[rows], w[rows])
    if n == 70:  # entries that are no row are skipped; a count past the segment's end reads padding and unwritten positions
        P = 2
        ps, lr = PolicySet(pols[:P]), OwnedRows(n, P, dev)
        lr.rows.fill_(CANARY)
        mask, owner = np.ones(n, bool), (np.arange(n) >= 40).astype(np.uint8)
        owned_rows(torch.from_numpy(mask).cuda(), torch.from_numpy(owner).cuda(), out=lr)
        assert lr.start.tolist() == [0, 64, 96] and lr.count.tolist() == [40, 30]
        lr.rows[5:6].fill_(-1)
        lr.rows[64 + 7:64 + 8].fill_(n)
        lr.count[1:2].fill_(1 << 30)
        for t in out + (logits_out,):
            _bits(t).fill_(F_CANARY)
        got = ps(obs, lr, u, out=out, logits_out=logits_out)
        mask[[5, 40 + 7]] = False
        _check_owned("entries that are no row", mask, owner, P, got, logits_out, full[False])


# ---- the episode against the restated loop
ASSIGNMENTS = ("parity", "world", "single")
# Policy c's one row, per case.  With the weights of SEEDS and the seeded draw, row 23 of the IGNORE case reaches its goal after
# a collision and an excursion off the road, and row 6 of the REMOVED case collides and is removed, which empties c's segment
# (test_the_cases_meet_the_conditions asserts both on the restated loop).
SINGLE_ROW = {"64-ignore-linear": 23, "128-removed-linear": 6}
# "mod8": eight policies, owner = slot % 8 among the controlled slots.  It runs on 128-removed-linear with EVERY object of the
# scenes controlled (ALL_OBJECTS): as the other cases build that simulator, the controlled slots of the three scenes are
# 0 .. 1, 0 .. 2 and eight of 0 .. 23 -- none in the second wave of k_mp_world's 128 lanes, and none with slot % 8 in (3, 5) --
# so no seed and no assignment gives a policy rows in both halves.  With every object controlled the last scene has controlled
# slots on either side of 64 (test_the_cases_meet_the_conditions asserts it on the restated loop's control_mask).
ALL_OBJECTS = dict(isStaticAgentControlled=1, initOnlyValidAgentsAtFirstStep=0, IgnoreNonVehicles=0)
MOD8 = ("128-removed-linear", "mod8")
CASES = [("64-ignore-linear", "parity"), ("64-ignore-linear", "single"), ("128-removed-linear", "world"),
         ("128-removed-linear", "single"), ("64-removed-linear-init11", "parity"), ("64-removed-linear-init11", "world"), MOD8]
DET = {("64-ignore-linear", "parity"), ("128-removed-linear", "world"), ("128-removed-linear", "single"), MOD8}
N_POLICIES = {"parity": 2, "world": 2, "single": 3, "mod8": 8}


def _sim_all_objects(A, cb, roads, scenes=SCENES):
    """tests/test_gpu_ppo_rollout._sim with every object of the scenes controlled."""
    from tests import parity
    from tests.test_gpu_ppo_rollout import BASE, GOAL, ROADS
    knn_order, algo, _ = ROADS[roads]
    return parity.make_gpu_sim(scenes, max_agents=A, knn_order=knn_order, collisionBehaviour=cb, roadObservationAlgorithm=algo,
                               distanceToGoalThreshold=GOAL, **dict(BASE, **ALL_OBJECTS))


def _policies(A, seeds=SEEDS):
    from gpudrive_lab_amd.policy import DevicePolicy
    return [DevicePolicy.from_state_dict(PC.state_dict(s, 6, 91), max_agents=A, ego_width=6) for s in seeds]


def _assign(case, assignment, ctrl, pols):
    """name -> (policy, mask): masks of controlled slots only (so the denominator is the world's rows)."""
    W, A = ctrl.shape
    slot = torch.arange(A, device=ctrl.device).expand(W, A)
    world = torch.arange(W, device=ctrl.device).unsqueeze(1).expand(W, A)
    if assignment == "mod8":
        return {name: (pol, ctrl & (slot % 8 == p)) for p, (name, pol) in enumerate(zip(NAMES8, pols))}
    if assignment == "parity":
        masks = [ctrl & (slot % 2 == 0), ctrl & (slot % 2 == 1)]
    elif assignment == "world":
        masks = [ctrl & (world % 2 == 0), ctrl & (world % 2 == 1)]
    else:
        w, s = ctrl.nonzero()[SINGLE_ROW[case]].tolist()
        one = torch.zeros_like(ctrl)
        one[w, s] = True
        masks = [ctrl & (slot % 2 == 0) & ~one, ctrl & (slot % 2 == 1) & ~one, one]
    return {name: (pol, mask) for name, pol, mask in zip(NAMES, pols, masks)}


def _compare(ep, r, what, n_steps=T):
    """Every output of run() against the restated loop's, bit for bit: over all rows (what gd_policy_rollout defines) and per
    policy."""
    for k in WORLD + PER_ROW + PER_STEP + ("any_active",):
        _same(getattr(ep, k), r[k], "%s %s" % (what, k))
    it = r["iterations"]
    assert int(ep.steps) == it, (what, int(ep.steps), it)
    got, want = ep.summary_tensor.cpu().numpy(), r["summary"]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (what, got, want)
    assert bool((ep.bad_indices == 0).all())
    _same(ep.denominator, r["denominator"], what + " denominator")
    for p, name in enumerate(ep.names):
        want = r["policies"][name]
        for k in MREF.WORLD_NAMES:
            _same(getattr(ep, "policy_" + k)[p], want[k], "%s policy %s %s" % (what, name, k))
        m = ep.metrics(name)
        assert tuple(m) == MREF.METRIC_KEYS
        for k in MREF.METRIC_KEYS:
            _same(m[k], want[k], "%s metrics(%s) %s" % (what, name, k))
    got, want = ep.policy_summary_tensor.cpu().numpy(), r["policy_summary"]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (what, got, want)
    assert ep.list_count.dtype == torch.int32 and tuple(ep.list_count.shape) == (T, len(ep.names))
    _same(ep.list_count[:it], r["list_count"][:it], what + " list_count")
    assert bool((ep.list_count[n_steps:] == 0).all()), what + ": list_count was written past n_steps"
    s = ep.summary()
    assert tuple(s) == REF.SUMMARY_NAMES + ("policies",) and tuple(s["policies"]) == ep.names
    for p, name in enumerate(ep.names):
        assert tuple(s["policies"][name].values()) == tuple(float(v) for v in r["policy_summary"][p])
    assert s["n_rows"] == sum(v["n_rows"] for v in s["policies"].values()) == r["live"].shape[0]


def _describe(what, r):
    print("MULTI %s: iterations %d lengths %s" % (what, r["iterations"], r["episode_lengths"].tolist()))
    for p, (name, m) in enumerate(r["policies"].items()):
        print("   %s rows %d goal %s collided %s off_road %s list_count min %d" % (
            name, int(m["n_rows"].sum()), m["goal_achieved_count"].tolist(), m["collided_count"].tolist(),
            m["off_road_count"].tolist(), int(r["list_count"][:r["iterations"], p].min())))


_CACHE = {}


def _case(case, assignment):
    """One case, computed once: run(record=True) with a seeded draw (and deterministically for the cases of DET) and the
    restated loop's outputs on a twin simulator fed the same u."""
    key = (case, assignment)
    if key not in _CACHE:
        from gpudrive_lab_amd import ClosedLoopMultiPPO
        A, cb, roads, init = MATRIX[case]
        with _Env(roads):
            rsim, tsim = (_sim_all_objects(A, cb, roads), _sim_all_objects(A, cb, roads)) if key == MOD8 else \
                (_sim(A, cb, roads), _sim(A, cb, roads))
            try:
                ctrl = rsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
                pols = _assign(case, assignment, ctrl, _policies(A, SEEDS8 if key == MOD8 else SEEDS))
                ev = ClosedLoopMultiPPO(rsim, pols, init_steps=init)
                ep = ev.run(generator=torch.Generator(device="cuda").manual_seed(5), record=True)
                r = MREF.closed_loop(tsim, pols, _table(), u=ep.u, init_steps=init)
                _describe("%s %s" % key, r)
                c = dict(ep=ep, r=r, N=ev.num_agents, owner=ev.owner.clone())
                if key in DET:
                    c["det"] = ev.run(deterministic=True, record=True)
                    c["rd"] = MREF.closed_loop(tsim, pols, _table(), deterministic=True, init_steps=init)
                if key == ("128-removed-linear", "world"):
                    c["part"] = ev.run(n_steps=40, generator=torch.Generator(device="cuda").manual_seed(5), record=True)
                    c["rpart"] = MREF.closed_loop(tsim, pols, _table(), u=ep.u, n_steps=40, init_steps=init)
                _CACHE[key] = c
            finally:
                rsim.close()
                tsim.close()
    return _CACHE[key]


@pytest.mark.parametrize("case,assignment", CASES)
def test_run_equals_the_restated_loop(case, assignment):
    c = _case(case, assignment)
    ep, N = c["ep"], c["N"]
    P = N_POLICIES[assignment]
    assert ep.names == NAMES8[:P] and tuple(ep.u.shape) == (T, N) and tuple(ep.policy_n_rows.shape) == (P, 6)
    assert sorted(set(c["owner"].tolist())) == list(range(P))
    _compare(ep, c["r"], "%s %s" % (case, assignment))
    if "det" in c:
        _compare(c["det"], c["rd"], "%s %s deterministic" % (case, assignment))
        assert not torch.equal(ep.actions_idx, c["det"].actions_idx), "the draw changed nothing"
    if "part" in c:  # n_steps = 40: the prefix of the full episode, and the loop cut at 40
        part, K = c["part"], 40
        _same(part.u, ep.u[:K], "the same seed")
        _compare(part, c["rpart"], "forty steps", n_steps=K)
        for k in ("actions_idx", "live_mask"):
            _same(getattr(part, k)[:, :K], getattr(ep, k)[:, :K], "prefix " + k)
            assert bool((getattr(part, k)[:, K:] == (-1 if k == "actions_idx" else 0)).all()), k + ": written past n_steps"
        _same(part.list_count[:K], ep.list_count[:K], "prefix list_count")
        _same(part.any_active[:K + 1], ep.any_active[:K + 1], "prefix any_active")


def test_the_cases_meet_the_conditions():
    """Asserted on the RESTATED loop's outputs, so that no case passes by exercising nothing.  Over the cases, every policy of
    every assignment has a row, a row that reaches the goal and a row that collides or leaves the road; some case ends early or
    has a world shorter than 90; some step has an empty segment beside one that is not."""
    rs = {key: _case(*key)["r"] for key in CASES}
    for assignment in ASSIGNMENTS:
        mine = {key: r for key, r in rs.items() if key[1] == assignment}
        assert mine
        for name in NAMES[:3 if assignment == "single" else 2]:
            ms = [r["policies"][name] for r in mine.values()]
            assert all(float(m["n_rows"].sum()) >= 1 for m in ms), (assignment, name, "a case in which the policy has no row")
            assert any(float(m["goal_achieved_count"].sum()) > 0 for m in ms), (assignment, name, "no row reaches the goal")
            assert any(float(m["collided_count"].sum() + m["off_road_count"].sum()) > 0 for m in ms), \
                (assignment, name, "no row collides or leaves the road")
    assert all(float(r["policies"]["c"]["n_rows"].sum()) == 1 for key, r in rs.items() if key[1] == "single")
    assert any(r["iterations"] < T or bool((r["episode_lengths"] < 90).any()) for r in rs.values())

    def empty_beside_full(r):
        lc = r["list_count"][:r["iterations"]]
        return bool(((lc == 0).any(1) & (lc > 0).any(1)).any())

    assert any(empty_beside_full(r) for r in rs.values()), "no step with an empty segment beside one that is not"
    world = rs[("128-removed-linear", "world")]
    for name in ("a", "b"):
        assert bool((world["policies"][name]["n_rows"] == 0).any()), "by world: every policy has worlds without rows"
    # eight policies on 128 slots: every policy has a row; some policy has rows in both waves of k_mp_world in one world; a
    # policy whose index only this case reaches has something to count
    r = rs[MOD8]
    ctrl = r["control_mask"].cpu().numpy()
    slot = np.arange(ctrl.shape[1])
    assert ctrl.shape[1] == 128 and all(float(r["policies"][name]["n_rows"].sum()) >= 1 for name in NAMES8)
    both = [(w, p) for w in range(ctrl.shape[0]) for p in range(8)
            if (ctrl[w] & (slot % 8 == p) & (slot < 64)).any() and (ctrl[w] & (slot % 8 == p) & (slot >= 64)).any()]
    counted = {name: [int(r["policies"][name][k].sum()) for k in ("goal_achieved_count", "collided_count", "off_road_count")]
               for name in NAMES8}
    print("MULTI mod8: (world, policy) with rows in both halves of the slots %s; goal / collided / off-road counts %s" % (both, counted))
    assert both, "no world in which a policy has rows on either side of slot 64"
    assert any(sum(counted[name]) > 0 for name in NAMES8[3:]), "no policy of index >= 3 has a non-zero count"
    # and the second wave's rows decide a count: some policy's count is another when only slots < 64 are counted
    acc = {k: np.zeros(ctrl.shape, np.float32) for k in ("goal_achieved", "collided", "off_road")}
    for k in acc:
        acc[k][ctrl] = r[k].cpu().numpy()
    owner = np.where(ctrl, slot % 8, -1)
    right, wave0 = (MREF.world_counts_by_wave(owner, acc["goal_achieved"], acc["collided"], acc["off_road"], 8, wrong=wrong)
                    for wrong in (None, "wave0"))
    for p, name in enumerate(NAMES8):
        for j, k in enumerate(("goal_achieved_count", "collided_count", "off_road_count", "n_rows")):
            assert np.array_equal(right[p, :, j], r["policies"][name][k].cpu().numpy()), (name, k)
    assert (right != wave0).any(), "the second wave counts nothing"


def _seed(s):
    return torch.Generator(device="cuda").manual_seed(s)


ROW_OUT = ("actions", "logprob", "entropy", "value")


def test_one_policy_and_twice_the_same_policy_equal_the_single_policy_evaluator():
    """Two invariants that fail on any mix-up of weights or rows.  P = 1 equals ClosedLoopPPO.run(compact=True) on a twin
    simulator in every output they share; P = 2 with the same weights under both names gives the same per-row results, and
    the two policies' counts add up to the single run's."""
    from gpudrive_lab_amd import ClosedLoopMultiPPO, ClosedLoopPPO
    A = 64
    msim, psim = _sim(A, REMOVED), _sim(A, REMOVED)
    try:
        pol, twin = _policies(A, (SEEDS[0], SEEDS[0]))
        single = ClosedLoopPPO(psim, pol).run(generator=_seed(5), record=True, compact=True)
        ctrl = msim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        one = ClosedLoopMultiPPO(msim, {"only": (pol, ctrl)}).run(generator=_seed(5), record=True)
        both = ClosedLoopMultiPPO(msim, _assign(None, "parity", ctrl, [pol, twin])).run(generator=_seed(5), record=True)
        for ep, what in ((one, "P = 1"), (both, "P = 2, the same weights")):
            for k in WORLD + PER_ROW + PER_STEP + ROW_OUT + ("any_active", "summary_tensor", "world_active", "bad_indices", "u"):
                _same(getattr(ep, k), getattr(single, k), "%s %s" % (what, k))
            assert int(ep.steps) == int(single.steps)
            _same(ep.list_count.sum(1).to(torch.int32), single.live_count, what + " list_count")
            for k in ("goal_achieved_count", "collided_count", "off_road_count"):
                _same(getattr(ep, "policy_" + k).sum(0), getattr(single, k), "%s: the policies' %s add up" % (what, k))
            _same(ep.policy_n_rows.sum(0), single.controlled_per_scene, what + " n_rows")
            _same(ep.denominator, single.controlled_per_scene, what + " denominator")
        for k in ("frac_goal_achieved", "frac_collided", "frac_off_road"):
            _same(getattr(one, "policy_" + k)[0], getattr(single, k), "P = 1 " + k)
        assert bool((both.policy_n_rows > 0).all(0).any()), "no world in which both policies have rows"
        assert float(single.goal_achieved_count.sum()) > 0 and int(single.live_count[int(single.steps) - 1]) < single.live.shape[0]
    finally:
        msim.close()
        psim.close()


def test_a_mask_slot_that_is_not_controlled_changes_the_denominator_only():
    from gpudrive_lab_amd import ClosedLoopMultiPPO
    A = 64
    sim = _sim(A, REMOVED)
    try:
        ctrl = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        pols = _assign(None, "parity", ctrl, _policies(A)[:2])
        plain = ClosedLoopMultiPPO(sim, pols).run(generator=_seed(9), record=True)
        w = 2
        free = (~ctrl[w]).nonzero().squeeze(1)[:3].tolist()
        assert len(free) == 3
        wider = {k: (p, m.clone()) for k, (p, m) in pols.items()}
        wider["a"][1][w, free[:2]] = True
        wider["b"][1][w, free[2]] = True
        ev = ClosedLoopMultiPPO(sim, wider)
        assert ev.num_agents == plain.live.shape[0] and torch.equal(ev.owner, plain.owner)
        ep = ev.run(generator=_seed(9), record=True)
        extra = torch.zeros(6, device="cuda")
        extra[w] = 3
        _same(ep.denominator, plain.denominator + extra, "denominator")
        for k in WORLD + PER_ROW + PER_STEP + ROW_OUT + ("any_active", "summary_tensor", "policy_summary_tensor", "list_count",
                                                         "policy_goal_achieved_count", "policy_collided_count",
                                                         "policy_off_road_count", "policy_n_rows"):
            _same(getattr(ep, k), getattr(plain, k), "a wider mask: " + k)
        for k in ("goal_achieved", "collided", "off_road"):
            got, was = getattr(ep, "policy_frac_" + k), getattr(plain, "policy_frac_" + k)
            others = [v for v in range(6) if v != w]
            _same(got[:, others], was[:, others], "the other worlds' fractions of " + k)
            _same(got[:, w], getattr(ep, "policy_%s_count" % k)[:, w] / ep.denominator[w], "the wider world's fraction of " + k)
        assert float(ep.denominator[w]) == float(ctrl[w].sum()) + 3
    finally:
        sim.close()


def test_no_host_synchronisation_canaries_nbytes_and_evaluate():
    from gpudrive_lab_amd import ClosedLoopMultiPPO
    from gpudrive_lab_amd.ppo_rollout import EVALUATE_COLUMNS
    A = 64
    batches = [[SCENES[0], SCENES[1], SCENES[2]], [SCENES[2], SCENES[0], SCENES[1]]]
    sim = _sim(A, REMOVED, scenes=batches[0])
    try:
        pols = _policies(A)
        slot = torch.arange(A, device="cuda").expand(3, A)
        masks = {name: (pol, slot % 3 == p) for p, (name, pol) in enumerate(zip(NAMES, pols))}  # full grids: any scenes
        ev = ClosedLoopMultiPPO(sim, masks)
        assert ev.denominator.tolist() == [A] * 3
        first = ev.run(generator=_seed(21), record=True)  # (the first step of a simulator may build its launch plan)
        carved = _Carved()
        ev._new = carved.new
        g = _seed(21)
        torch.cuda.synchronize()
        ep = _no_sync(lambda: ev.run(generator=g, record=True))
        torch.cuda.synchronize()
        carved.check()
        assert set(carved.whole) >= {"owned_rows", "owned_start", "owned_count", "owned_scratch", "list_count", "policy_summary",
                                     "policy_n_rows", "policy_frac_collided", "actions", "summary", "any_active"}
        for k in WORLD + PER_ROW + PER_STEP + ROW_OUT + ("list_count", "policy_summary_tensor", "policy_frac_goal_achieved"):
            _same(getattr(ep, k), getattr(first, k), "two runs " + k)
        del ev._new
        assert ClosedLoopMultiPPO.nbytes(sim, masks, record=True, stochastic=True) == sum(
            n for _, n in carved.whole.values()) + ep.u.numel() * 4

        res = ev.evaluate(batches, generator=_seed(3))
        g = _seed(3)
        eps = []
        for b in batches:
            ev.resample(b)
            eps.append(ev.run(generator=g))
        assert res["scene"] == batches[0] + batches[1] and tuple(res["policies"]) == NAMES
        same = lambda got, want: (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(  # noqa: E731
            np.nan_to_num(got).view(np.int32), np.nan_to_num(want).view(np.int32)))
        for name, src in EVALUATE_COLUMNS:
            assert same(res[name], torch.cat([getattr(e, src) for e in eps]).cpu().numpy()), name
        for p, name in enumerate(NAMES):
            for k in MREF.METRIC_KEYS[3:]:
                assert same(res["policies"][name][k], torch.cat([getattr(e, "policy_" + k)[p] for e in eps]).cpu().numpy()), (name, k)
    finally:
        sim.close()


# ---- past one world per lane of the per-policy summary
def test_run_equals_the_restated_loop_on_258_worlds(big_twins):  # noqa: F811
    """W = 258: lane l of k_mp_summary's 256 adds worlds l and l + 256 of every policy, so lanes 0 and 1 add a second term.
    Three policies, owner = (world + slot) % 3, so that every policy has rows in worlds 256 and 257 and something to count
    there (asserted on the restated loop's outputs): a summary that stops at 256 worlds differs for every policy.  Every
    summed field is a count: integers whose total stays far below 2^24, so the float32 sums are exact in ANY order (asserted)
    -- what this case holds the summary to is that every world is added exactly once per policy, not the order."""
    from gpudrive_lab_amd import ClosedLoopMultiPPO
    rsim, tsim = big_twins
    A, W, P = 64, BIG_W, 3
    assert W > 256 and W % 256 == 2
    ctrl = rsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
    slot = torch.arange(A, device=ctrl.device).expand(W, A)
    world = torch.arange(W, device=ctrl.device).unsqueeze(1).expand(W, A)
    pols = {name: (pol, ctrl & ((world + slot) % P == p)) for p, (name, pol) in enumerate(zip(NAMES, _policies(A)))}
    ev = ClosedLoopMultiPPO(rsim, pols)
    ep = ev.run(generator=_seed(5), record=True)
    r = MREF.closed_loop(tsim, pols, _table(), u=ep.u)
    assert ev.num_agents == int(r["control_mask"].sum()) > 256 and tuple(ep.policy_n_rows.shape) == (P, W)
    _compare(ep, r, "258 worlds")
    flags = ("goal_achieved_count", "collided_count", "off_road_count")
    per = [{k: r["policies"][name][k].cpu().numpy() for k in flags + ("n_rows",)} for name in NAMES]
    print("MULTI 258 worlds: rows %d iterations %d policy_summary %s; worlds 256, 257: %s" % (
        ev.num_agents, r["iterations"], r["policy_summary"].tolist(), [{k: v[256:].tolist() for k, v in m.items()} for m in per]))
    for name, m in zip(NAMES, per):
        assert (m["n_rows"][256:] > 0).all(), (name, "no rows in world 256 or 257")
        assert sum(float(m[k][256:].sum()) for k in flags) > 0, (name, "nothing to count in worlds 256 and 257")
        for k in flags + ("n_rows",):
            v = m[k].astype(np.float64)
            assert (v == np.round(v)).all() and 0 <= v.sum() < 2 ** 24, (name, k, "not exactly representable")
            assert float(REF.ordered_sum(m[k])) == v.sum(), (name, k)
    cut = MREF.summary(per, wrong="first_256")
    assert (cut[:, :3] != r["policy_summary"][:, :3]).any(1).all() and (cut[:, 3] != r["policy_summary"][:, 3]).all(), \
        "a summary of the first 256 worlds is the same for some policy"
