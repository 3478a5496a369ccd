"""GPU suite: the live-row policy forward.

A row's result in the forward never depends on the rows that share its wave, so the forward on a row list must give every
listed row the FULL forward's bits and touch nothing else; `gd_live_rows` must give `torch.nonzero`'s list; the evaluator with
the list in the loop must give the evaluator's results.  Everything here is an exact comparison: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import policy_cases as PC
from tests.test_gpu_policy import _no_sync, _side_stream
from tests.test_gpu_ppo_rollout import (MATRIX, PER_ROW, PER_STEP, REMOVED, SCENES, WORLD, T, _Carved, _case, _compare,
                                        _loop, _policy, _same, _sim)

pytestmark = pytest.mark.gpu

CANARY = 0x5EEDBEEF  # no row index, no count
GUARD = 64


class _Carver:
    """Tensors carved from canary-filled int32 buffers with GUARD words either side (the allocator a LiveRows accepts)."""

    def __init__(self):
        self.whole = {}

    def new(self, name, shape, dtype, fill, device):
        assert dtype == torch.int32
        words = int(np.prod(shape))
        buf = torch.full((GUARD + words + GUARD,), CANARY, dtype=torch.int32, device=device)
        self.whole[name] = (buf, words)
        return buf[GUARD:GUARD + words].view(shape)

    def refill(self):
        for buf, _ in self.whole.values():
            buf.fill_(CANARY)

    def check(self, what):
        for name, (buf, words) in self.whole.items():
            assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + words:] == CANARY).all()), \
                "%s: words beside %s were written" % (what, name)


def _masks(n):
    g = torch.Generator(device="cuda").manual_seed(1000 + n % 997)
    z = torch.zeros(n, dtype=torch.bool, device="cuda")
    last, first = z.clone(), z.clone()
    last[n - 1:] = True
    first[:1] = True
    half = torch.rand(n, device="cuda", generator=g) < 0.5
    sparse = torch.rand(n, device="cuda", generator=g) < 0.02
    odd = torch.where(half, torch.where(sparse, 255, 2), 0).to(torch.uint8)  # a uint8 mask: 2 and 255 count as live
    return dict(zeros=z, ones=~z, last=last, first=first, half=half, sparse=sparse, bytes_2_and_255=odd)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 70001, 1 << 20])
def test_live_rows_equals_nonzero(n):
    from gpudrive_lab_amd.policy import LiveRows, live_rows, live_rows_scratch_ints
    carver = _Carver()
    lr = LiveRows(n, torch.device("cuda", torch.cuda.current_device()), new=carver.new)
    assert lr.scratch.numel() == live_rows_scratch_ints(n) == -(-n // 1024)
    for name, mask in _masks(n).items():
        what = "n=%d %s" % (n, name)
        want = torch.nonzero(mask).squeeze(1).to(torch.int32)
        k = int(want.numel())
        carver.refill()
        assert live_rows(mask, out=lr) is lr
        carver.check(what)
        assert int(lr.count) == k, (what, int(lr.count), k)
        assert torch.equal(lr.rows[:k], want), what + ": not nonzero's list"
        assert bool((lr.rows[k:] == CANARY).all()), what + ": rows past the count were written"
        first = [t.clone() for t in (lr.rows, lr.count, lr.scratch)]
        live_rows(mask, out=lr)
        for a, b in zip(first, (lr.rows, lr.count, lr.scratch)):
            assert torch.equal(a, b), what + ": two calls differ"
    if n == 1025:  # without out=: a fresh list, the same values; a bool view of the bytes, the same list
        mask = _masks(n)["half"]
        fresh = live_rows(mask)
        k = int(fresh.count)
        live_rows(mask.view(torch.uint8), out=lr)
        assert k == int(lr.count) and torch.equal(fresh.rows[:k], lr.rows[:k])
        with pytest.raises(ValueError, match="out must be a LiveRows of N = 1025"):
            live_rows(mask, out=LiveRows(1024, mask.device))


# ---- the forward on a row list against the full forward
N_F = 70
NA = 91
F_CANARY = 0x7FC0DEAD  # a NaN payload no kernel writes
LIST_SIZES = (3, 4, 5, 31, 32, 33, 64, 65)  # either side of the embed workgroup (4), the tail tile (32), the sample block (64)


def _lists():
    rng = np.random.default_rng(77)
    lists = {"empty": [], "last": [N_F - 1], "all": list(range(N_F))}
    for k in LIST_SIZES:
        lists["first%d" % k] = list(range(k))
        lists["any%d" % k] = sorted(rng.choice(N_F, k, replace=False).tolist())  # not contiguous
    lists["subset"] = np.nonzero(rng.random(N_F) < 0.4)[0].tolist()
    return lists


def _canary_outputs():
    f = torch.float32
    ints = lambda shape: torch.full(shape, F_CANARY, dtype=torch.int32, device="cuda")  # noqa: E731
    out = (torch.full((N_F,), F_CANARY, dtype=torch.int64, device="cuda"),) + tuple(ints((N_F,)).view(f) for _ in range(3))
    return out, ints((N_F, NA)).view(f)


def _bits(t):
    return t if t.dtype == torch.int64 else t.view(torch.int32)


def _check_listed(what, rows, got, got_logits, want, want_logits):
    listed = torch.zeros(N_F, dtype=torch.bool, device="cuda")
    listed[rows] = True
    for name, g, w in zip(("actions", "logprob", "entropy", "value", "logits"), got + (got_logits,), want + (want_logits,)):
        g, w = _bits(g), _bits(w)
        assert torch.equal(g[listed], w[listed]), "%s: %s of a listed row differs from the full forward" % (what, name)
        assert bool((g[~listed] == F_CANARY).all()), "%s: %s of a row that is not listed was written" % (what, name)
        if len(rows) == N_F:
            assert torch.equal(g, w), "%s: %s" % (what, name)


@pytest.mark.parametrize("a,ew", [(64, 6), (64, 9), (128, 6), (128, 9)])
def test_forward_on_a_row_list_equals_the_full_forward(a, ew):
    from gpudrive_lab_amd.dropout import DropoutRule
    from gpudrive_lab_amd.policy import DevicePolicy, LiveRows, live_rows
    sd = PC.state_dict(11, ew, NA)
    obs = torch.from_numpy(PC.observations(20 + N_F + a, N_F, a, ew)).cuda()
    u = torch.from_numpy(PC.uniforms(N_F, N_F)).cuda()
    pol = DevicePolicy.from_state_dict(sd, max_agents=a, ego_width=ew)
    rule = DropoutRule(0.25, 4321, device="cuda")
    dropped = DevicePolicy.from_state_dict(sd, max_agents=a, ego_width=ew, dropout_rule=rule)
    K = 9
    full = {}
    for det in (False, True):
        logits = torch.empty((N_F, NA), device="cuda")
        full[det] = (pol(obs, None if det else u, deterministic=det, logits_out=logits), logits)
    rule.seek(K)
    logits = torch.empty((N_F, NA), device="cuda")
    full["drop"] = (dropped(obs, u, logits_out=logits), logits)
    assert rule.call == K + 1 and not torch.equal(full["drop"][1], full[False][1]), "the rule masks nothing"
    assert not torch.equal(full[False][0][0], full[True][0][0]), "the draw changed nothing"

    lr = LiveRows(N_F, obs.device)
    out, logits_out = _canary_outputs()
    for name, rows in _lists().items():
        what = "A=%d ego=%d list %s" % (a, ew, name)
        mask = torch.zeros(N_F, dtype=torch.bool, device="cuda")
        mask[rows] = True
        live_rows(mask, out=lr)
        assert int(lr.count) == len(rows)
        for det in (False, True):
            for t in out + (logits_out,):
                _bits(t).fill_(F_CANARY)
            got = pol(obs, None if det else u, deterministic=det, out=out, logits_out=logits_out, rows=lr)
            assert all(g is o for g, o in zip(got, out))
            _check_listed(what + (" det" if det else ""), rows, got, logits_out, *full[det])
        for t in out + (logits_out,):
            _bits(t).fill_(F_CANARY)
        rule.seek(K)
        got = dropped(obs, u, out=out, logits_out=logits_out, rows=lr)
        assert rule.call == K + 1, what + ": the call index did not advance by one"
        _check_listed(what + " dropout", rows, got, logits_out, *full["drop"])

    # no host synchronisation with out= and a reused list; fresh outputs are zero where no row is listed
    _no_sync(lambda: pol(obs, u, out=out, logits_out=logits_out, rows=live_rows(mask, out=lr)))
    fresh = pol(obs, u, rows=lr)
    for g, w in zip(fresh, full[False][0]):
        assert torch.equal(g[mask], w[mask]) and bool((g[~mask] == 0).all())

    # an entry that is no row is skipped, a count above N is read as N (memory safety only)
    lr.rows.copy_(torch.arange(N_F, dtype=torch.int32, device="cuda"))
    lr.rows[5:6].fill_(-1)
    lr.rows[40:41].fill_(N_F)
    lr.count.fill_(N_F + 1000)
    for t in out + (logits_out,):
        _bits(t).fill_(F_CANARY)
    got = pol(obs, u, out=out, logits_out=logits_out, rows=lr)
    _check_listed("A=%d ego=%d entries that are no row" % (a, ew), [r for r in range(N_F) if r not in (5, 40)], got, logits_out,
                  *full[False])


# ---- run(compact=True) against run() and against the restated loop
ROW_OUT = ("actions", "logprob", "entropy", "value")


def _seed(s):
    return torch.Generator(device="cuda").manual_seed(s)


def _same_runs(c, e, what, n_steps=T):
    """run(compact=True) against run() with the same u, both with record=True: everything bit for bit.  The forward's four
    outputs are compared on the rows live at the last iteration when that is the run's last step: run() forwards all N rows at
    every step up to n_steps, also after the reference's `break`, so what it leaves for a row is the forward of step
    n_steps - 1; the compact run leaves a row the forward of its last live step.  The two are the same step exactly for the
    rows live before step n_steps - 1.  For every row the compact run's action must be the recorded index of its last live step."""
    for k in WORLD + PER_ROW + PER_STEP + ("any_active", "summary_tensor", "world_active", "bad_indices"):
        _same(getattr(c, k), getattr(e, k), "%s compact %s" % (what, k))
    steps = int(e.steps)
    assert int(c.steps) == steps
    if hasattr(e, "u"):
        _same(c.u, e.u, what + " u")
    rows = e.live_mask[:, n_steps - 1] if steps == n_steps else torch.zeros_like(e.live_mask[:, 0])
    for k in ROW_OUT:
        _same(getattr(c, k)[rows], getattr(e, k)[rows], "%s compact %s of the rows live at the last iteration" % (what, k))
    assert c.live_count.dtype == torch.int32 and tuple(c.live_count.shape) == (T,)
    _same(c.live_count[:steps], e.live_mask[:, :steps].sum(0).to(torch.int32), what + " live_count")
    ever = e.live_mask.any(1)
    last_live = (e.live_mask * torch.arange(1, T + 1, device="cuda")).argmax(1)
    _same(c.actions[ever], e.actions_idx[torch.arange(len(ever), device="cuda"), last_live][ever],
          what + " compact actions against the index recorded at each row's last live step")


@pytest.mark.parametrize("name", ["128-removed-linear", "64-removed-linear-init11"])
def test_compact_run_equals_run_and_the_restated_loop(name):
    """The matrix case of tests/test_gpu_ppo_rollout.py (its run(), its restated loop, both seeded alike and deterministic)
    against run(compact=True) on a third simulator of the same scenes."""
    from gpudrive_lab_amd import ClosedLoopPPO
    A, cb, roads, init = MATRIX[name]
    assert cb == REMOVED and roads == "linear"
    c = _case(name)
    r, N = c["r"], c["N"]
    last = r["iterations"] - 1
    counts = r["live_mask"].sum(0)
    if init == 0:  # asserted on the restated loop: a workload in which nothing dies cannot pass silently
        assert int(counts[0]) == N and int(counts[last]) < N / 2, counts.tolist()
    sim = _sim(A, cb, roads)
    try:
        ev = ClosedLoopPPO(sim, _policy(A), init_steps=init)
        ep = ev.run(generator=_seed(5), record=True, compact=True)
        det = ev.run(deterministic=True, record=True, compact=True)
        _same_runs(ep, c["ep"], name)
        _same_runs(det, c["det"], name + " deterministic")
        _compare(ep, r, name + " compact")
        _compare(det, c["rd"], name + " compact deterministic")
        if init == 0:  # the prefix
            K = 7
            part = ev.run(n_steps=K, generator=_seed(5), record=True, compact=True)
            _same(part.u, ep.u[:K], "the same seed")
            _same(part.live_count[:K], ep.live_count[:K], "prefix live_count")
            assert bool((part.live_count[K:] == 0).all()), "live_count was written past n_steps"
            for k in ("actions_idx", "live_mask"):
                _same(getattr(part, k)[:, :K], getattr(ep, k)[:, :K], "prefix " + k)
            _same(part.any_active[:K + 1], ep.any_active[:K + 1], "prefix any_active")
            _same_runs(part, ev.run(n_steps=K, generator=_seed(5), record=True), "seven steps", n_steps=K)
    finally:
        sim.close()


def test_compact_conditioned_rows_and_explicit_mask():
    """ego_width 9 against run() and the restated loop; then an explicit mask that leaves five worlds without a row."""
    from gpudrive_lab_amd import ClosedLoopPPO
    A = 64
    rsim, tsim = _sim(A, REMOVED), _sim(A, REMOVED)
    try:
        pol = _policy(A, ego_width=9)
        wt = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (6, A, 3)).astype(np.float32)).cuda()
        ev = ClosedLoopPPO(rsim, pol, reward_weights=wt)
        ep = ev.run(generator=_seed(9), record=True, compact=True)
        _same_runs(ep, ev.run(generator=_seed(9), record=True), "conditioned")
        _compare(ep, _loop(tsim, pol, u=ep.u, reward_weights=wt), "conditioned compact")

        pol = _policy(A)
        ctrl = rsim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        w = int(ctrl.sum(1).argmax())
        agents = ctrl[w].nonzero().squeeze(1)[:2].tolist()
        mask = torch.zeros_like(ctrl)
        mask[w, agents] = True
        mask[w, A - 1] = True  # a slot that holds no agent: done at once
        ev = ClosedLoopPPO(rsim, pol, mask=mask)
        assert ev.num_agents == 3
        ep = ev.run(generator=_seed(7), record=True, compact=True)
        _same_runs(ep, ev.run(generator=_seed(7), record=True), "explicit mask")
        _compare(ep, _loop(tsim, pol, mask=mask, u=ep.u), "explicit mask compact")
        empty = [v for v in range(6) if v != w]
        assert len(empty) == 5 and bool(torch.isnan(ep.frac_goal_achieved[empty]).all())
        assert int(ep.live_count[0]) == 3 and int(ep.live_count[1]) == 2
    finally:
        rsim.close()
        tsim.close()


def test_compact_run_on_258_worlds():
    """N > 256 rows: the list crosses the embed workgroups, the tail tiles and the sample blocks while rows die."""
    from gpudrive_lab_amd import ClosedLoopPPO
    W = 258
    scenes = SCENES[:3] * (W // 3)
    rsim, tsim = _sim(64, REMOVED, scenes=scenes), _sim(64, REMOVED, scenes=scenes)
    try:
        pol = _policy(64)
        ev = ClosedLoopPPO(rsim, pol)
        N = ev.num_agents
        assert N > 256
        ep = ev.run(generator=_seed(5), record=True, compact=True)
        _same_runs(ep, ev.run(generator=_seed(5), record=True), "258 worlds")
        r = _loop(tsim, pol, u=ep.u)
        _compare(ep, r, "258 worlds compact")
        counts = ep.live_count[:int(ep.steps)].tolist()
        assert counts[0] == N and counts[-1] < N / 2 and len({c // 64 for c in counts}) > 2, counts
    finally:
        rsim.close()
        tsim.close()


def test_compact_no_host_synchronisation_canaries_and_evaluate():
    from gpudrive_lab_amd import ClosedLoopPPO
    from gpudrive_lab_amd.ppo_rollout import EVALUATE_COLUMNS
    A = 64
    batches = [[SCENES[0], SCENES[1], SCENES[2]], [SCENES[2], SCENES[0], SCENES[1]]]
    sim = _sim(A, REMOVED, scenes=batches[0])
    try:
        ev = ClosedLoopPPO(sim, _policy(A))
        first = ev.run(generator=_seed(21), record=True, compact=True)  # (the first step may build the launch plan)
        carved = _Carved()
        ev._new = carved.new
        g = _seed(21)
        ep = _no_sync(lambda: ev.run(generator=g, record=True, compact=True))
        torch.cuda.synchronize()
        carved.check()
        assert set(carved.whole) >= {"rows", "rows_count", "rows_scratch", "live_count"}
        for k in WORLD + PER_ROW + PER_STEP + ROW_OUT + ("live_count",):
            _same(getattr(ep, k), getattr(first, k), "two runs " + k)
        del ev._new
        assert ClosedLoopPPO.nbytes(sim, ev.policy, record=True, stochastic=True, compact=True) == sum(
            n for _, n in carved.whole.values()) + ep.u.numel() * 4

        res = ev.evaluate(batches, generator=_seed(3), compact=True)
        want = ev.evaluate(batches, generator=_seed(3))
        assert res["scene"] == want["scene"] and set(res) == set(want)
        for name, _ in EVALUATE_COLUMNS:
            assert np.array_equal(np.isnan(res[name]), np.isnan(want[name])), name
            assert np.array_equal(np.nan_to_num(res[name]).view(np.int32), np.nan_to_num(want[name]).view(np.int32)), name
    finally:
        sim.close()


# ---- the training side: the rollout buffer keeps live rows only, so the forward may skip the others
def test_the_learner_rollout_is_the_same_with_the_forward_on_live_rows():
    """40 steps of DeviceLearnerEnv under AgentRemoved, stepped with the FULL forward's actions (so the test does not depend
    on what the step does with a dead row's stale action): the full forward's and the live-row forward's outputs, stored into
    two rollout buffers with the same rewards, terminals and masks, give bit-identical training batches."""
    from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table
    from gpudrive_lab_amd.policy import DevicePolicy, LiveRows, live_rows
    from gpudrive_lab_amd.rollout import DeviceRollout
    sim = _sim(64, REMOVED, scenes=SCENES[:3])
    steps = 40
    try:
        with _side_stream():
            env = DeviceLearnerEnv(sim)
            n = env.num_agents
            obs = env.reset()
            D = int(obs.shape[1])
            pol = DevicePolicy.from_state_dict(PC.state_dict(3, 6, action_table("classic").shape[0]), max_agents=64, ego_width=6)
            gen = _seed(7)
            obs, rewards, terminals, truncations, masks = env.step(torch.zeros(n, dtype=torch.int64, device="cuda"))
            lr = LiveRows(n, obs.device)
            part = tuple(torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int64,) + (torch.float32,) * 3)
            kept = []
            for _ in range(steps):
                u = torch.rand(n, device="cuda", generator=gen)
                full = pol(obs, u)
                pol(obs, u, rows=live_rows(masks, out=lr), out=part)
                kept.append((obs.clone(), full, tuple(t.clone() for t in part), rewards.clone(), terminals.clone(), masks.clone()))
                obs, rewards, terminals, truncations, masks = env.step(full[0])
            live = torch.stack([k[5] for k in kept])
            total = int(live.sum())
            assert bool((~live).any()), "no step had a dead row: the live-row forward skipped nothing"
            assert n < total < steps * n
            ros = [DeviceRollout(total, num_rows=n, obs_width=D) for _ in range(2)]
            for o, f, p, rw, tm, mk in kept:
                for ro, (actions, logprob, entropy, value) in zip(ros, (f, p)):
                    ro.store(o, value, actions, logprob, rw, tm, mk)
            batches = []
            for ro in ros:
                ro.sort_training_data()
                ro.compute_gae(0.99, 0.95)
                batches.append(ro.flatten_batch())
            assert len(batches[0]) == 7
            for name, a, b in zip(DeviceRollout.OUT_NAMES, *batches):
                _same(a, b, "flatten_batch " + name)
            assert len(torch.unique(batches[0][1])) > 1 and bool(torch.isfinite(batches[0][2]).all())
    finally:
        sim.close()

