"""GPU suite: the partner rows (partner_observations_tensor) and the packed heads on the constructed, moving worlds of
tests/partner_cases.py.  After the reset pass and after EVERY step the device's rows are held to the oracle (ints exact, state bit
for bit under the State model, rows within OBS_ATOL outside the pairs the reference calls marginal) AND to the float64 reference
of tests/partner_reference.py computed from the kernel's OWN exported tensors of that pass: the radius verdict outside the margin
mask, speed, size, type, id and both zero rows exact, x, y and heading within GPU_FACTOR times the oracle's measured distance
from the same reference (PC.ORACLE_PARTNER_MAX, measured and asserted in the CPU suite -- never a figure from a kernel's output).

partner_counts, partner_headings and partner_moves run once more with GPUDRIVE_SPLIT_PARTNER=1 on a side stream (k_partner_rows;
the set-up of tests/test_gpu_round3.py) and once more with GPUDRIVE_NO_POSE_SKIP=1 (the aligned store path on step passes too).
partner_counts, partner_radius, partner_moves and partner_slots128 run with the packed head attached in each of its three layouts
-- the direct pack, the learner rows, the conditioned learner rows -- beside a twin without it: the ego and partner columns of
every live row within the bound carried through each column's gain of the float64 packing of the reference rows, bit-equal to the
second-pass packing of the raw rows, the three weight columns exactly the weights given, and a sentinel written over every head
and behind the last row before each pass still in place wherever no row's head belongs.  A difference from the oracle on a pair
the reference calls marginal is not a kernel bug; the remedy is to move the case's geometry, not the band."""
import contextlib

import numpy as np
import pytest

from tests import parity as P
from tests import partner_cases as PC
from tests import partner_reference as PR
from tests import step_reference as SR

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in PC.CASE_LIST]
PACKED_RUNS = [(name, layout) for name in PC.PACKED for layout in PC.LAYOUTS]
SENTINEL_BITS = 0x7FC0DEAD      # a NaN payload no kernel writes
GUARD = 1 << 16                 # floats behind the last packed row
INTS = ["done_tensor", "info_tensor", "steps_remaining_tensor", "shape_tensor"]


def _against_the_oracle(run, p, gpu, orc, sim):
    P.compare_ints(gpu, orc, INTS)
    if run.case.model == SR.STATE:
        assert P.compare_state_bits(gpu, orc) > 0
        return PC.rows_against(run, p, sim, 0, P.OBS_ATOL)
    P.compare_state(gpu, orc)
    return PC.rows_against(run, p, sim, 0, P.FREE_OBS_ATOL)


def _summary(tag, seen, worst, premise, extra=""):
    print("PARTNER_GPU %s: passes %d, pairs %d, marginal %d (cap %d), marginal by design %d, exact verdicts at the radius %d, inside %d, outside %d; "
          "error / bound: %s%s; premise: %s" % (tag, seen["passes"], seen["pairs"], seen["marginal"], int(PC.MARGIN_AGENTS * seen["pairs"]), seen["designed"],
                                                seen["exact"], seen["inside"], seen["outside"],
                                                ", ".join("%s@%g %.2f" % (c, s, v) for (s, c), v in sorted(worst.items())), extra, premise))


def _hold(run, p, sim, seen, worst):
    e = PC.hold(run, p, PC.GPU_FACTOR, sim=sim)
    for k, v in e["ratio"].items():
        worst[k] = max(worst.get(k, 0.0), v)
    for k in ("pairs", "marginal", "designed", "exact", "inside", "outside"):
        seen[k] = max(seen[k], e[k])
    seen["passes"] += 1
    assert e["marginal"] <= PC.MARGIN_AGENTS * e["pairs"], "%d of %d pairs are marginal" % (e["marginal"], e["pairs"])
    if run.case.actions is PC._shift_actions and not run.passes[p]["reset"]:      # (every agent moved and turned: nothing may keep its bits)
        stale = PC.stale_floats(run, p, sim)
        assert stale == 0, "%s: %d x / y / heading floats hold the bits of the pass before" % (run.passes[p]["tag"], stale)


def _new_seen():
    return dict(passes=0, pairs=0, marginal=0, designed=0, exact=0, inside=0, outside=0)


def _run(O, monkeypatch, tmp_path, name, env=None, side_stream=False):
    import torch
    case = PC.CASES[name]
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    paths = PC.write_scenes(case, tmp_path)
    kw = case.params(PC.ALGO)
    nw = len(case.worlds)
    with (torch.cuda.stream(torch.cuda.Stream()) if side_stream else contextlib.nullcontext()):
        gpu = P.make_gpu_sim(paths[:nw], max_agents=case.slots, **kw)
        orc = P.make_oracle_sim(O, paths[:nw], max_agents=case.slots, **kw)
        try:
            run = PC.Run(case, [orc, gpu])
            run.scene_paths = paths
            worst, seen = {}, _new_seen()
            how = ", ".join("%s=%s" % kv for kv in sorted((env or {}).items()))
            skipped = [0]

            def check(p):
                tag = "%s%s, %s" % (name, " (%s)" % how if how else "", run.passes[p]["tag"])
                try:
                    skipped[0] += _against_the_oracle(run, p, gpu, orc, 1)
                except AssertionError as e:
                    late = PC.errors(run, p, PC.GPU_FACTOR, sim=1)
                    raise AssertionError("%s: against the oracle: %s [the reference calls %d of %d pairs marginal, %d more by design]" % (
                        tag, e, late["marginal"], late["pairs"], late["designed"]))
                _hold(run, p, 1, seen, worst)

            PC.script(run, check)
            premise = case.premise(run)
            extra = ""
            if side_stream:
                assert gpu.stat(0) > 0, "the step graph (with its fork and join) was not replayed"
                extra = "; %d steps replayed from the graph" % gpu.stat(0)
            _summary("%s%s" % (name, " (%s)" % how if how else ""), seen, worst, premise, extra)
            assert seen["passes"] == case.steps + 1 + len(case.events)
        finally:
            gpu.close()
            orc.close()


@pytest.mark.parametrize("name", NAMES)
def test_partner_rows_meet_oracle_and_reference_at_every_pass(oracle_mod, monkeypatch, tmp_path, name):
    _run(oracle_mod, monkeypatch, tmp_path, name)


@pytest.mark.parametrize("name", PC.SECOND_STREAM)
def test_partner_rows_written_on_the_second_stream(oracle_mod, monkeypatch, tmp_path, name):
    """GPUDRIVE_SPLIT_PARTNER=1 on a side stream: k_partner_rows writes the rows, forked and joined inside the captured step graph.
    (That the kernel ran is by construction -- the switch and a stream that is not the null stream -- and the replayed graph is
    counted; the engine reports no more.)"""
    _run(oracle_mod, monkeypatch, tmp_path, name, env={"GPUDRIVE_SPLIT_PARTNER": "1"}, side_stream=True)


@pytest.mark.parametrize("name", PC.SECOND_STREAM)
def test_partner_rows_without_the_pose_skip(oracle_mod, monkeypatch, tmp_path, name):
    """GPUDRIVE_NO_POSE_SKIP=1: step passes write every row, the id -2 rows included, through the aligned path."""
    _run(oracle_mod, monkeypatch, tmp_path, name, env={"GPUDRIVE_NO_POSE_SKIP": "1"})


# ------------------------------------------------------------------------------------------------------------------
# the packed heads
# ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(-1).view(__import__("torch").int32).cpu().numpy().view(np.uint32)


class _Heads:
    """One simulator with the packed head attached in one layout, its buffer guarded by a sentinel."""

    def __init__(self, layout, sim, case, shape):
        import torch
        self.layout, self.sim = layout, sim
        W, A = len(case.worlds), case.slots
        self.W, self.A, self.H = W, A, PR.head_width(A - 1)
        D = self.H + 200 * 13
        dev = sim._device
        live = np.arange(A)[None, :] < shape[:, 0:1]
        if layout == "direct":
            self.mask_np = np.ones((W, A), bool)
            self.pitch, self.n = D, W * A
            self.buf = torch.zeros(self.n * self.pitch + GUARD, dtype=torch.float32, device=dev)
            assert sim.direct_pack(only=False, out=self.buf[:self.n * self.pitch].view(W, A, D)) is not False
            self.weights = None
        else:
            self.mask_np = live & (np.arange(A)[None, :] % 3 != 1)          # two live agents of three have a learner row
            mask = torch.as_tensor(self.mask_np, device=dev)
            self.n = sim.set_learner_rows(mask)
            assert self.n == int(self.mask_np.sum()) > 0
            self.pitch = D + (3 if layout == "conditioned" else 0)
            self.buf = torch.zeros(self.n * self.pitch + GUARD, dtype=torch.float32, device=dev)
            self.weights = None
            if layout == "conditioned":
                self.weights = ((torch.arange(W * A * 3, dtype=torch.float32, device=dev) * 0.37) % 5.0 - 2.5).view(W, A, 3).contiguous()
            rows = sim.direct_pack_rows(only=False, out=self.buf, reward_weights=self.weights)
            assert tuple(rows.shape) == (self.n, self.pitch)
        self.slots = [(int(w), int(a)) for w, a in np.argwhere(self.mask_np)]       # row r: the slot it belongs to (row-major)
        self.width = self.H + (3 if layout == "conditioned" else 0)                  # floats of a row's head

    def rows(self):
        return self.buf[:self.n * self.pitch].view(self.n, self.pitch)

    def arm(self):
        """The sentinel over every row's head and behind the last row."""
        import torch
        bits = self.buf.view(torch.int32)
        bits[:self.n * self.pitch].view(self.n, self.pitch)[:, :self.width] = SENTINEL_BITS
        bits[self.n * self.pitch:] = SENTINEL_BITS
        torch.cuda.synchronize()

    def twin_rows(self, twin):
        """The second-pass packing of the twin's raw rows, in this layout."""
        import torch
        full = twin.packed_observations() if self.weights is None else twin.packed_observations(reward_weights=self.weights)
        torch.cuda.synchronize()
        return full.reshape(self.W * self.A, -1)[torch.as_tensor(self.mask_np.reshape(-1), device=full.device)]

    def check(self, run, p, twin, sim_index, tag):
        """Returns the worst error / bound of the heads against the reference."""
        import torch
        torch.cuda.synchronize()
        shape = run.passes[p]["snaps"][sim_index]["shape"]
        got, want = _bits(self.rows()).reshape(self.n, self.pitch), _bits(self.twin_rows(twin)).reshape(self.n, self.pitch)
        tail = _bits(self.buf[self.n * self.pitch:])
        assert (tail == SENTINEL_BITS).all(), "%s: %d floats behind the last row were written" % (tag, int((tail != SENTINEL_BITS).sum()))
        live = np.asarray([a < int(shape[w, 0]) for w, a in self.slots])
        head = got[:, :self.width]
        untouched = (head == SENTINEL_BITS).all(-1)
        assert not (head[live] == SENTINEL_BITS).any(), "%s: %d floats of live rows' heads were not written" % (tag, int((head[live] == SENTINEL_BITS).sum()))
        same = (got == want).all(-1)
        # a padding agent's row (direct pack only) is written by the passes that follow a rebuild, or not at all
        bad = np.nonzero(~np.where(live, same, untouched | same))[0]
        assert not len(bad), "%s: %d rows are not the second-pass packing of the raw rows bit for bit; first row %d (world %d, agent %d), column %d" % (
            tag, len(bad), bad[0], *self.slots[bad[0]], int(np.nonzero(got[bad[0]] != want[bad[0]])[0][0]))
        heads = self.rows().cpu().numpy()[:, :self.width]
        if self.layout == "conditioned":
            wt = self.weights.cpu().numpy()
            given = np.stack([wt[w, a] for w, a in self.slots])
            assert np.array_equal(heads[:, 6:9].view(np.uint32), given.view(np.uint32)), "%s: the weight columns are not the weights given" % tag
            heads = np.concatenate([heads[:, :6], heads[:, 9:]], -1)
        rows_live = np.nonzero(live)[0]
        worst, wrong = PC.head_errors(run, p, heads[rows_live], [self.slots[r] for r in rows_live], PC.GPU_FACTOR, sim_index)
        assert not wrong, "%s: packed heads beyond the carried bound: %s" % (tag, "; ".join(wrong[:3]))
        return worst


@pytest.mark.parametrize("key", PACKED_RUNS, ids=["%s-%s" % k for k in PACKED_RUNS])
def test_packed_heads_meet_the_reference_and_the_second_pass(oracle_mod, monkeypatch, tmp_path, key):
    name, layout = key
    case = PC.CASES[name]
    paths = PC.write_scenes(case, tmp_path)
    kw = case.params(PC.ALGO)
    nw = len(case.worlds)
    orc = P.make_oracle_sim(oracle_mod, paths[:nw], max_agents=case.slots, **kw)
    twin = P.make_gpu_sim(paths[:nw], max_agents=case.slots, **kw)
    gpu = P.make_gpu_sim(paths[:nw], max_agents=case.slots, **kw)
    try:
        heads = _Heads(layout, gpu, case, np.asarray(orc.shape_tensor()))
        heads.arm()
        run = PC.Run(case, [orc, twin, gpu])
        run.scene_paths = paths
        worst, seen, head_worst = {}, _new_seen(), [0.0]

        def check(p):
            tag = "%s (%s), %s" % (name, layout, run.passes[p]["tag"])
            _against_the_oracle(run, p, gpu, orc, 2)
            _hold(run, p, 2, seen, worst)
            a, b = run.passes[p]["snaps"][2]["rows"], run.passes[p]["snaps"][1]["rows"]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: the raw partner rows differ from the twin's" % tag
            head_worst[0] = max(head_worst[0], heads.check(run, p, twin, 2, tag))
            heads.arm()

        PC.script(run, check)
        _summary("%s (%s, %d rows)" % (name, layout, heads.n), seen, worst, case.premise(run), "; packed head error / bound %.2f" % head_worst[0])
        assert seen["passes"] == case.steps + 1 + len(case.events)
    finally:
        gpu.close()
        twin.close()
        orc.close()
