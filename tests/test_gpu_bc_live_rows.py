"""GPU suite: the live-row BC forward.

No result of a sample in the BC forward depends on the samples beside it, so the forward on a row list must give every listed
row the FULL forward's bits and touch nothing else; the closed-loop driver with the list in the loop must give the driver's
results.  Everything here is an exact comparison: no tolerance anywhere.  (tests/test_gpu_bc_wide_edges.py runs the edge
configurations' lists on the 128-wide policy through `_row_lists_at_an_edge_configuration`.)"""
import numpy as np
import pytest
import torch

from tests import bc_cases as BC
from tests.test_gpu_bc_policy import _no_sync
from tests.test_gpu_bc_rollout import (LAST_SEEN, MATRIX, PER_ROW, PER_STEP, REMOVED, T, _Carved, _case, _compare, _loop, _same,
                                       _sim, _state_dict)

pytestmark = pytest.mark.gpu

CHUNK = 4
B_F = 11  # three chunks of four list positions, the last one short
F_CANARY = 0x7FC0DEAD  # a NaN payload no kernel writes
I_CANARY = 0x5EEDBEEF  # no row index, no count, no component
GUARD = 64
OUTPUTS = ("context", "means", "log_covariances", "covariances", "weights", "actions", "nll", "ego_attn_score", "component")


def _policy(A, R, sd=None, chunk_rows=CHUNK, cfg=BC.CFG, **width):
    from gpudrive_lab_amd.bc_policy import DeviceBCPolicy
    return DeviceBCPolicy.from_state_dict(sd if sd is not None else _state_dict(R), max_agents=A, num_stack=R,
                                          chunk_rows=chunk_rows, **cfg, **width)


class _Guarded:
    """int32 words between two guard bands of a canary; `view` is the words as the tensor a call takes."""

    def __init__(self, shape, dtype, canary):
        words = int(np.prod(shape))
        self.canary, self.words = canary, words
        self.buf = torch.full((GUARD + words + GUARD,), canary, dtype=torch.int32, device="cuda")
        self.view = self.buf[GUARD:GUARD + words].view(dtype).view(shape)

    def refill(self):
        self.buf.fill_(self.canary)

    def bits(self):
        return self.buf[GUARD:GUARD + self.words].view(self.view.shape)

    def check(self, what):
        assert bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.words:] == self.canary).all()), \
            what + ": words beside the array were written"


def _lists():
    """name -> rows, ascending and permuted: either side of the chunk of four, a list that ends a chunk, one that leaves the
    middle chunk's rows (4..7) out entirely, everything, nothing."""
    rng = np.random.default_rng(5)
    base = {"empty": [], "last": [10], "first3": [0, 1, 2], "first4": [0, 1, 2, 3], "first5": [0, 1, 2, 3, 4],
            "eight": [0, 2, 3, 4, 6, 7, 9, 10], "all": list(range(B_F)), "no_middle_chunk": [0, 1, 2, 3, 8, 9, 10]}
    lists = dict(base)
    for k, v in base.items():
        if len(v) > 1:
            lists[k + "_permuted"] = [v[i] for i in rng.permutation(len(v))]
    return lists


def _live_rows_of(rows, count=None):
    """A LiveRows holding `rows` (in this order), its arrays between guard bands."""
    from gpudrive_lab_amd.policy import LiveRows
    made = {}

    def new(name, shape, dtype, fill, device):
        made[name] = g = _Guarded(shape, dtype, I_CANARY)
        return g.view

    lr = LiveRows(B_F, torch.device("cuda", torch.cuda.current_device()), new=new)
    if rows:
        lr.rows[:len(rows)] = torch.tensor(rows, dtype=torch.int32, device="cuda")
    lr.count.fill_(len(rows) if count is None else count)
    return lr, made


def _forward_case(A, R, cfg=BC.CFG, **width):
    """width: network_dim=128 for the wide policy (tests/test_gpu_bc_wide_edges.py); nothing for the 64-wide one."""
    obs, pm, rm, expert, u, z, _ = BC.inputs(B_F, A, R)
    obs, pm, rm, expert, u, z = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (obs, pm, rm, expert, u, z))
    pol = _policy(A, R, sd=BC.state_dict(R, cfg, **width), cfg=cfg, **width)
    full = {det: pol.forward(obs, pm, rm, OUTPUTS, deterministic=det, u=u, z=z, expert_actions=expert) for det in (True, False)}
    assert not torch.equal(full[True]["actions"], full[False]["actions"]), "the draw changed nothing"
    outs = {}
    for name in OUTPUTS:
        dt = torch.int32 if name == "component" else torch.float32
        outs[name] = _Guarded(pol._OUT_SHAPES[name](pol, B_F), dt, I_CANARY if name == "component" else F_CANARY)
    return pol, (obs, pm, rm, expert, u, z), full, outs


def _check_listed(what, rows, outs, want):
    listed = torch.zeros(B_F, dtype=torch.bool, device="cuda")
    if rows:
        listed[rows] = True
    for name, g in outs.items():
        g.check("%s %s" % (what, name))
        got, w = g.bits(), want[name].view(torch.int32)
        assert torch.equal(got[listed], w[listed]), "%s: %s of a listed row differs from the full forward" % (what, name)
        assert bool((got[~listed] == g.canary).all()), "%s: %s of a row that is not listed was written" % (what, name)


@pytest.mark.parametrize("A,R", [(64, 5), (128, 5), (64, 1)])
def test_forward_on_a_row_list_equals_the_full_forward(A, R):
    pol, (obs, pm, rm, expert, u, z), full, outs = _forward_case(A, R)
    out = {k: g.view for k, g in outs.items()}
    for name, rows in _lists().items():
        lr, made = _live_rows_of(rows)
        for det in (True, False):
            what = "A=%d R=%d list %s%s" % (A, R, name, " det" if det else " drawn")
            for g in outs.values():
                g.refill()
            got = pol.forward(obs, pm, rm, OUTPUTS, deterministic=det, u=u, z=z, expert_actions=expert, out=out, rows=lr)
            assert all(got[k] is out[k] for k in OUTPUTS)
            _check_listed(what, rows, outs, full[det])
            for k, g in made.items():
                g.check(what + " " + k)
            assert int(lr.count) == len(rows) and lr.rows[:len(rows)].tolist() == rows, what + ": the list was written"

    # the public methods take rows= too; no host synchronisation with out= and a list made before
    lr, _ = _live_rows_of([1, 5, 10])
    for g in outs.values():
        g.refill()
    _no_sync(lambda: (pol(obs, pm, rm, deterministic=True, out=out["actions"], rows=lr),
                      pol.context(obs, pm, rm, out=out["context"], ego_attn_score=out["ego_attn_score"], rows=lr),
                      pol.gmm_params(obs, pm, rm, out=(out["means"], out["covariances"], out["weights"]), rows=lr),
                      pol.nll(obs, pm, rm, expert, out=out["nll"], rows=lr)))
    written = ("actions", "context", "ego_attn_score", "means", "covariances", "weights", "nll")
    _check_listed("A=%d R=%d the methods" % (A, R), [1, 5, 10], {k: outs[k] for k in written}, full[True])
    for k in ("log_covariances", "component"):
        assert bool((outs[k].buf == outs[k].canary).all()), k + " was not asked for"


@pytest.mark.parametrize("name", ["top", "c10"])
def test_forward_on_a_row_list_at_the_edge_configurations(name):
    """bc_cases.EDGE_CASES' largest model and the first mixture whose head outputs take a second trip: the rows of a list have
    the full forward's bits in every output, and nothing else is written."""
    _row_lists_at_an_edge_configuration(name, *BC.EDGE[name][1:])


def _row_lists_at_an_edge_configuration(name, A, R, cfg, **width):
    pol, (obs, pm, rm, expert, u, z), full, outs = _forward_case(A, R, cfg, **width)
    out = {k: g.view for k, g in outs.items()}
    assert full[True]["means"].shape == (B_F, 1, cfg["n_components"], 3)
    lists = _lists()
    for which in ("empty", "last", "first5", "eight_permuted", "all", "no_middle_chunk"):
        rows = lists[which]
        lr, made = _live_rows_of(rows)
        for det in (True, False):
            what = "%s list %s%s" % (name, which, " det" if det else " drawn")
            for g in outs.values():
                g.refill()
            pol.forward(obs, pm, rm, OUTPUTS, deterministic=det, u=u, z=z, expert_actions=expert, out=out, rows=lr)
            _check_listed(what, rows, outs, full[det])
            for k, g in made.items():
                g.check(what + " " + k)


def test_a_count_above_b_and_entries_that_are_no_row():
    """Memory safety only: a count above B is read as B; an entry of -1 and one of B are skipped, the other listed rows are
    written and nothing else."""
    A, R = 64, 1
    pol, (obs, pm, rm, expert, u, z), full, outs = _forward_case(A, R)
    out = {k: g.view for k, g in outs.items()}
    lr, made = _live_rows_of(list(range(B_F)), count=B_F + 1000)
    pol.forward(obs, pm, rm, OUTPUTS, deterministic=False, u=u, z=z, expert_actions=expert, out=out, rows=lr)
    _check_listed("a count above B", list(range(B_F)), outs, full[False])
    rows = [3, -1, 7, B_F, 0, 9]
    lr, made = _live_rows_of(rows)
    for g in outs.values():
        g.refill()
    pol.forward(obs, pm, rm, OUTPUTS, deterministic=False, u=u, z=z, expert_actions=expert, out=out, rows=lr)
    _check_listed("entries that are no row", [3, 7, 0, 9], outs, full[False])
    for k, g in made.items():
        g.check("entries that are no row " + k)


# ---- run(compact=True) against run() and against the restated loop
CONFIGS = ("128-5-delta-removed-linear", "64-1-classic-removed-linear")


def _same_runs(c, e, what, n_steps=T, record=True):
    """run(compact=True) against run(), everything but row_actions bit for bit."""
    for k in (PER_STEP if record else ()) + PER_ROW + LAST_SEEN + ("any_alive", "summary_tensor"):
        _same(getattr(c, k), getattr(e, k), "%s compact %s" % (what, k))
    assert int(c.steps) == int(e.steps)
    a, b = c.summary(), e.summary()  # (a NaN rate, 0 / 0 of a row that starts on its goal, equals itself here)
    assert a.keys() == b.keys() and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a), (what, a, b)
    assert bool((c.live_count[n_steps:] == 0).all()), what + ": live_count written past n_steps"


def _check_live_count_and_row_actions(c, what, n_steps=T):
    steps = int(c.steps)
    live = (~c.dead_mask[:, :steps]).sum(0).to(torch.int32)
    assert torch.equal(c.live_count[:steps], live), (what, c.live_count.tolist(), live.tolist())
    assert bool((c.live_count[steps:n_steps] == 0).all()), what + ": a list past the reference's break is not empty"
    # a row's action is the forward's of its last live step: what was recorded there, not zeros and not a later step's
    t = torch.arange(steps, device="cuda")
    last_live = torch.where(~c.dead_mask[:, :steps], t, -1).max(1).values
    assert bool((last_live >= 0).all())
    want = c.actions[torch.arange(c.actions.shape[0], device="cuda"), last_live]
    _same(c.row_actions, want, what + " row_actions")


_RUNS = {}


def _runs(name):
    """run(record=True) and run(record=True, compact=True) of one configuration with chunk_rows = 4, and the restated loop's
    outputs (test_gpu_bc_rollout's, computed once)."""
    if name not in _RUNS:
        from gpudrive_lab_amd import ClosedLoopBC
        A, R, model, cb, roads = MATRIX[name]
        r = _case(name)["r"]
        sim = _sim(A, model, cb, roads)
        try:
            loop = ClosedLoopBC(sim, _policy(A, R))
            e = loop.run(record=True)
            c = loop.run(record=True, compact=True)
            torch.cuda.synchronize()
        finally:
            sim.close()
        _RUNS[name] = (c, e, r)
    return _RUNS[name]


@pytest.mark.parametrize("name", CONFIGS)
def test_compact_run_equals_run_and_the_reference_loop(name):
    c, e, r = _runs(name)
    _compare(e, r, name + " run()")
    _compare(c, r, name + " compact")
    _same_runs(c, e, name)
    _check_live_count_and_row_actions(c, name)
    assert tuple(c.live_count.shape) == (T,) and c.live_count.dtype == torch.int32
    print("BC COMPACT %s: rows %d live_count %s" % (name, r["dead"].shape[0], c.live_count.tolist()))


def test_the_configurations_meet_the_conditions():
    """Asserted on the REFERENCE loop's outputs: the live count is below N at some step, no multiple of the chunk at some step,
    at most N - chunk at some step (a wholly empty chunk is launched), and above 0 at the last step in one configuration."""
    above_zero_at_the_end = False
    for name in CONFIGS:
        r = _case(name)["r"]
        N, steps = r["dead"].shape[0], r["iterations"]
        live = (~r["dead_mask"][:, :steps]).sum(0).tolist()
        assert any(v < N for v in live), (name, live)
        assert any(v % CHUNK != 0 for v in live), (name, live)
        assert any(v <= N - CHUNK for v in live), (name, live)
        above_zero_at_the_end |= steps == T and live[T - 1] > 0
    assert above_zero_at_the_end, "no configuration has a live row at the last step"


def test_the_draw_an_explicit_mask_and_seven_steps():
    from gpudrive_lab_amd import ClosedLoopBC
    A, R, model = 64, 5, "delta_local"
    sim = _sim(A, model, REMOVED, "linear")
    try:
        pol = _policy(A, R)
        loop = ClosedLoopBC(sim, pol)
        seed = lambda: torch.Generator(device="cuda").manual_seed(5)  # noqa: E731
        e = loop.run(deterministic=False, generator=seed(), record=True)
        c = loop.run(deterministic=False, generator=seed(), record=True, compact=True)
        _same(c.u, e.u, "u")
        _same(c.z, e.z, "z")
        _same_runs(c, e, "the draw")
        _check_live_count_and_row_actions(c, "the draw")
        assert not torch.equal(c.actions, loop.run(record=True, compact=True).actions), "the draw changed nothing"

        full = loop.run(record=True, compact=True)
        K = 7
        part = loop.run(n_steps=K, record=True, compact=True)
        _same_runs(part, loop.run(n_steps=K, record=True), "seven steps", n_steps=K)
        for k in PER_STEP:
            _same(getattr(part, k)[:, :K], getattr(full, k)[:, :K], "prefix " + k)
        _same(part.live_count[:K], full.live_count[:K], "prefix live_count")
        _check_live_count_and_row_actions(part, "seven steps", n_steps=K)

        ctrl = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        w = int(ctrl.sum(1).argmax())
        agents = ctrl[w].nonzero().squeeze(1)[:2].tolist()
        assert len(agents) == 2 and int(sim.shape_tensor().to_torch()[w, 0]) < A  # slot A - 1 of the world holds no agent
        mask = torch.zeros_like(ctrl)
        mask[w, agents] = True
        mask[w, A - 1] = True
        masked = ClosedLoopBC(sim, pol, mask=mask)
        assert masked.num_agents == 3
        c3 = masked.run(record=True, compact=True)
        _same_runs(c3, masked.run(record=True), "explicit mask")
        _check_live_count_and_row_actions(c3, "explicit mask")
    finally:
        sim.close()


def test_no_host_synchronisation_canaries_and_a_policy_under_training():
    from gpudrive_lab_amd import ClosedLoopBC, DeviceBC
    A, R, model = 64, 5, "delta_local"
    sim = _sim(A, model, REMOVED, "linear")
    try:
        bc = DeviceBC(_state_dict(R), max_agents=A, num_stack=R, batch_size=8, chunk_rows=CHUNK, partials=3, **BC.CFG)
        loop = ClosedLoopBC(sim, bc.policy)
        first = loop.run(record=True)  # (the first step of a simulator may build its launch plan)
        carved = _Carved()
        loop._new = carved.new
        ep = _no_sync(lambda: loop.run(record=True, compact=True))
        torch.cuda.synchronize()
        carved.check()
        assert set(carved.whole) >= {"window", "row_actions", "any_alive", "summary", "actions", "dead_mask", "dead", "rows",
                                     "rows_count", "rows_scratch", "live_count"}
        del loop._new
        _same_runs(ep, first, "two runs")
        _check_live_count_and_row_actions(ep, "canaries")

        obs, pm, rm = first.window[:8].contiguous(), torch.zeros((8, R, A - 1), dtype=torch.bool, device="cuda"), \
            torch.zeros((8, R, 200), dtype=torch.bool, device="cuda")
        pm[:, R - 1], rm[:, R - 1] = first.partner_mask[:8], first.road_mask[:8]
        bc.update(obs, torch.zeros((8, 1, 3), dtype=torch.float32, device="cuda"), pm, rm)
        after = loop.run(record=True)
        _same_runs(loop.run(record=True, compact=True), after, "after one update")
        assert not torch.equal(after.actions, first.actions), "the weights did not move the actions"
    finally:
        sim.close()
