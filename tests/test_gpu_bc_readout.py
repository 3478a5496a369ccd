"""GPU suite: the probe read-outs inside the BC forward and the closed loop (gpudrive_lab_amd.bc_readout.ProbeReadout,
DeviceBCPolicy.hidden(layer=) / .read, ClosedLoopBC.run(attention=, readout=); gd_bc_hidden_layer, gd_bc_forward_readout,
gd_bc_forward_rows_readout, gd_bc_rollout_readout; csrc/bc_readout.hip, csrc/bc_readout_rule.hpp).

Weights are tests/bc_cases.state_dict(R); probes have seeded standard-normal weights and biases (`_head`).  What is exact is held
bit for bit: the taps against today's `hidden`, the read-outs against the probes' own `predict` where the tap is theirs, the
actions against the plain forward, the loop against the restated loop (tests/bc_rollout_reference.closed_loop) with the
stand-alone calls made per step on the same obs[~dead] batch.  The inner tap and the intervention have no kernel of their own to
be compared with, so they are held to float64 on the kernel's own input bits (`hidden('ro_attn', layer=0)`), on every row the
float64 statement decides (see test_inner_tap_and_intervention_against_float64)."""
import ctypes

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import bc_cases as BC
from tests import bc_readout_reference as RR
from tests import bc_rollout_reference as REF
from tests.test_gpu_bc_policy import _no_sync, _policy
from tests.test_gpu_bc_rollout import IGNORE, REMOVED, SCENES, _Env, _loop, _same, _sim
from tests.test_gpu_bc_rollout import _policy as _loop_policy

pytestmark = pytest.mark.gpu

T = 91
CANARY = 0xA5
EPS = 2.0 ** -24


def _head(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {"head.weight": (torch.randn(64, 64, generator=g) * scale).contiguous(), "head.bias": torch.randn(64, generator=g) * scale}


def _probe(bc, model, exp, seed, hd=None):
    from gpudrive_lab_amd import DeviceLinearProbe
    return DeviceLinearProbe(bc, hd if hd is not None else _head(seed), model=model, exp=exp)


def _inp(B, A, R, seed=1):
    obs, pm, rm, _, u, z, _ = BC.inputs(B, A, R, seed=seed)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (obs, pm, rm, u, z)]


def _canaried(shape):
    """A uint8 tensor of CANARY bytes inside a larger one of the same byte: (view, whole, offset)."""
    n = int(np.prod(shape))
    whole = torch.full((64 + n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    return whole[64:64 + n].view(shape), whole


def _guards_hold(whole, n):
    h = whole.cpu().numpy()
    return bool((h[:64] == CANARY).all() and (h[64 + n:] == CANARY).all())


# ---- 1. the tap at any layer

@pytest.mark.parametrize("A,R", [(64, 1), (64, 5), (128, 1), (128, 5)])
def test_hidden_layer_none_and_last_are_todays_hidden(A, R):
    B = 3
    bc = _policy(A, R, chunk_rows=2)  # a chunk boundary and a short last chunk
    obs, pm, rm, _, _ = _inp(B, A, R)
    nf, nb = BC.CFG["num_layer"]
    seen = {}
    for tap, last in (("fusion_attn", nf - 1), ("ro_attn", nb - 1)):
        today = bc.hidden(obs, pm, rm, tap=tap)
        _same(bc.hidden(obs, pm, rm, tap=tap, layer=None), today, "%s layer=None" % tap)
        _same(bc.hidden(obs, pm, rm, tap=tap, layer=last), today, "%s layer=%d" % (tap, last))
        for i in range(last + 1):
            seen[(tap, i)] = bc.hidden(obs, pm, rm, tap=tap, layer=i)
            assert bool(torch.isfinite(seen[(tap, i)]).all())
    # an inner layer is another tensor than its neighbours (the new argument selects something)
    assert not torch.equal(seen[("ro_attn", 0)], seen[("ro_attn", nb - 1)])
    assert not torch.equal(seen[("ro_attn", 0)], seen[("fusion_attn", nf - 1)])
    assert not torch.equal(seen[("fusion_attn", 0)], seen[("fusion_attn", nf - 1)])
    for bad in (-1, nb, 1.0, True):
        with pytest.raises(ValueError, match="layer"):
            bc.hidden(obs, pm, rm, tap="ro_attn", layer=bad)


@pytest.mark.parametrize("name", ["top", "deep_branch", "deep_fusion"])
def test_hidden_layer_at_the_edge_layer_counts(name):
    """(4, 4), (1, 4) and (4, 1) layers: layer=None and the block's last index are today's `hidden`, every inner index is another
    tensor, and the index one past the block is refused.  (The values: test_gpu_lp_probe holds every index to float64.)"""
    from tests import bc_grad_reference as GR
    B, A, R, cfg = BC.EDGE[name]
    bc = _policy(A, R, GR.state_dict(R, cfg), cfg, chunk_rows=2)
    obs, pm, rm, _, _ = _inp(B, A, R)
    for tap, n in zip(("fusion_attn", "ro_attn"), cfg["num_layer"]):
        today = bc.hidden(obs, pm, rm, tap=tap)
        _same(bc.hidden(obs, pm, rm, tap=tap, layer=None), today, "%s %s layer=None" % (name, tap))
        seen = [bc.hidden(obs, pm, rm, tap=tap, layer=i) for i in range(n)]
        _same(seen[-1], today, "%s %s layer=%d" % (name, tap, n - 1))
        for i in range(n):
            for j in range(i):
                assert not torch.equal(seen[i], seen[j]), (name, tap, i, j)
        with pytest.raises(ValueError, match="layer"):
            bc.hidden(obs, pm, rm, tap=tap, layer=n)


# ---- 2. where the tap is the probes' own, the read-out is their predict

@pytest.mark.parametrize("tap,model", [("fusion_attn", "early_lp"), ("ro_attn", "late_lp")])
def test_read_equals_the_probes_own_kernels(tap, model):
    from gpudrive_lab_amd import ProbeReadout
    B, A, R = 35, 64, 1  # an ego tile of 32 samples plus a tail of 3; chunk_rows 32: a second chunk of 3
    bc = _policy(A, R, chunk_rows=32)
    obs, pm, rm, _, _ = _inp(B, A, R)
    others = [_probe(bc, model, "other", 11), _probe(bc, model, "other", 12)]
    egos = [_probe(bc, model, "ego", 21)]
    ro = ProbeReadout(bc, tap=tap, layer=None, other=others, ego=egos)
    assert ro.names == ("other_pred", "ego_pred")
    r = bc.read(obs, pm, rm, ro)
    assert tuple(r["other_pred"].shape) == (B, 2, A - 1) and tuple(r["ego_pred"].shape) == (B, 1)
    assert r["other_pred"].dtype == torch.uint8 and "ego_pred_prime" not in r
    for q, pr in enumerate(others):
        want = pr.predict(obs, pm, rm)
        assert int(want.max()) < 64 and len(want.unique()) > 8
        _same(r["other_pred"][:, q], want.to(torch.uint8), "%s other[%d]" % (tap, q))
    _same(r["ego_pred"][:, 0], egos[0].predict(obs, pm, rm).to(torch.uint8), "%s ego[0]" % tap)
    _same(r["actions"], bc(obs, pm, rm, deterministic=True), "actions")
    # the stochastic draw too, and a probe that changes between two calls is followed in place
    u, z = _inp(B, A, R)[3:]
    _same(bc.read(obs, pm, rm, ro, deterministic=False, u=u, z=z)["actions"], bc(obs, pm, rm, u=u, z=z), "drawn actions")
    others[0].load_state_dict(_head(99))
    _same(bc.read(obs, pm, rm, ro)["other_pred"][:, 0], others[0].predict(obs, pm, rm).to(torch.uint8), "after load_state_dict")


@pytest.mark.parametrize("A", [64, 128])
@pytest.mark.parametrize("tap,model", [("fusion_attn", "early_lp"), ("ro_attn", "late_lp")])
def test_read_of_eight_pairs_equals_the_probes_own_kernels(tap, model, A):
    """bc_readout_rule::MAX_PROBES = 8 probes in either list, every head another: `ROArgs.opacked` / `oweight` / `epacked` at
    3 .. 7 and other_pred's stride q * (A - 1) up to q = 7.  Column q of other_pred and ego_pred is probe q's own `predict`; the
    prime of pair p is the prime of a read-out built from pair p alone (so `oweight[p]` is the p-th).  At A = 128 a slot has 4
    partner tiles, the last with 31 rows: its last column, 126, is written (the outputs start as canaries) and equal."""
    from gpudrive_lab_amd import ProbeReadout
    B, R = 35, 1
    bc = _policy(A, R, chunk_rows=32)
    obs, pm, rm, _, _ = _inp(B, A, R)
    others = [_probe(bc, model, "other", 110 + q) for q in range(8)]
    egos = [_probe(bc, model, "ego", 120 + q) for q in range(8)]
    labels = torch.from_numpy(RR.labels_with(B, ())).cuda()
    ro = ProbeReadout(bc, tap=tap, layer=None, other=others, ego=egos, labels=labels)
    out, wholes = {}, {}
    for k in ro.names:
        out[k], wholes[k] = _canaried((B,) + ro.row_shape(k))
    r = bc.read(obs, pm, rm, ro, out=out)
    assert tuple(r["other_pred"].shape) == (B, 8, A - 1) and tuple(r["ego_pred"].shape) == tuple(r["ego_pred_prime"].shape) == (B, 8)
    for k in ro.names:
        assert _guards_hold(wholes[k], out[k].numel()), k
        assert bool((r[k] < 64).all()), "%s was not written whole" % k
    seen = []
    for q in range(8):
        want = others[q].predict(obs, pm, rm).to(torch.uint8)
        _same(r["other_pred"][:, q], want, "%s A=%d other[%d]" % (tap, A, q))
        _same(r["other_pred"][:, q, A - 2], want[:, A - 2], "the last partner column")
        _same(r["ego_pred"][:, q], egos[q].predict(obs, pm, rm).to(torch.uint8), "%s A=%d ego[%d]" % (tap, A, q))
        one = bc.read(obs, pm, rm, ProbeReadout(bc, tap=tap, layer=None, other=[others[q]], ego=[egos[q]], labels=labels))
        _same(r["ego_pred_prime"][:, q], one["ego_pred_prime"][:, 0], "%s A=%d the prime of pair %d alone" % (tap, A, q))
        seen.append(torch.cat([r["other_pred"][:, q].flatten(), r["ego_pred"][:, q], r["ego_pred_prime"][:, q]]))
    for q in range(8):
        for j in range(q):  # distinct heads give distinct columns: a probe read in another's place shows
            assert not torch.equal(seen[q], seen[j]), (q, j)
        assert not torch.equal(r["ego_pred_prime"][:, q], r["ego_pred"][:, q]), "pair %d: the intervention changed no class" % q
    assert A - 2 == {64: 62, 128: 126}[A] and (A - 1 + 31) // 32 == {64: 2, 128: 4}[A] and (A - 1) % 32 == 31
    assert int(ro.bad_labels.item()) == 0
    _same(r["actions"], bc(obs, pm, rm, deterministic=True), "actions")


def test_read_makes_no_host_synchronisation_and_no_allocation_with_out():
    from gpudrive_lab_amd import ProbeReadout
    B, A, R = 5, 64, 1
    bc = _policy(A, R, chunk_rows=4)
    obs, pm, rm, _, _ = _inp(B, A, R)
    ro = ProbeReadout(bc, "ro_attn", 0, other=[_probe(bc, "late_lp", "other", 1)], ego=[_probe(bc, "late_lp", "ego", 2)], labels=7)
    fresh = bc.read(obs, pm, rm, ro)
    out, wholes = {"actions": torch.empty_like(fresh["actions"])}, {}
    for k in ro.names:
        out[k], wholes[k] = _canaried(tuple(fresh[k].shape))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = _no_sync(lambda: bc.read(obs, pm, rm, ro, out=out))
    assert torch.cuda.memory_allocated() == before
    for k in ("actions",) + ro.names:
        assert got[k].data_ptr() == out[k].data_ptr()
        _same(got[k], fresh[k], k)
    for k in ro.names:
        assert _guards_hold(wholes[k], out[k].numel()), k
        assert bool((out[k] < 64).all()), "%s was not written whole" % k


# ---- 3. the inner tap and the intervention against float64

def _decided(x, W, b, got, what):
    """x [n, 64] float32 (the kernel's own input bits), W [64, 64], b [64]: the rows float64 decides, and got on them."""
    x64, W64, b64 = x.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    logits = x64 @ W64.T + b64
    E = 66 * EPS * (np.abs(x64)[:, None, :] * np.abs(W64)[None, :, :]).sum(-1) + 66 * EPS * np.abs(b64)  # [n, 64]
    top = logits.argmax(-1)
    r = np.arange(len(x))
    gap = logits[r, top][:, None] - logits
    need = E[r, top][:, None] + E
    need[r, top] = -1.0  # the top against itself
    decided = (gap > need).all(-1)
    wrong = decided & (got.astype(np.int64) != top)
    assert not wrong.any(), "%s: %d decided rows differ, first %d: %d vs %d" % (what, wrong.sum(), wrong.argmax(), got[wrong.argmax()],
                                                                              top[wrong.argmax()])
    return int(decided.sum()), len(x)


def test_inner_tap_and_intervention_against_float64():
    """('ro_attn', 0) -- the layer intervention.py hooks -- with two pairs and per-row labels.  The kernel's input bits are
    `hidden('ro_attn', layer=0)`; the logits are restated in float64 from them, and a row is decided when top - logit_c >
    E_top + E_c for every class c, E_c = 66 * 2^-24 * (sum_k |W_ck x_k| + |b_c|): the n u bound of a dot product of length 64
    plus the bias in any order (n = 66).  Every decided row must match; at most 1 % may be undecided.  The probes' weights are
    standard normal (scale 1.0): the bound and the gaps both scale with the weights, so the undecided share does not depend on
    the scale, and for 64 independent normal logits the chance that the two largest lie within 2 E ~ 1e-4 of their spread is
    of the order 1e-4.  Observed on an MI355X: 0 of 4550 rows undecided (printed below)."""
    from gpudrive_lab_amd import ProbeReadout
    B, A, R = 35, 64, 5
    bc = _policy(A, R, chunk_rows=32)
    obs, pm, rm, _, _ = _inp(B, A, R)
    heads = {k: _head(s) for k, s in (("o0", 31), ("o1", 32), ("e0", 41), ("e1", 42))}
    others = [_probe(bc, "late_lp", "other", 0, heads["o0"]), _probe(bc, "early_lp", "other", 0, heads["o1"])]
    egos = [_probe(bc, "late_lp", "ego", 0, heads["e0"]), _probe(bc, "early_lp", "ego", 0, heads["e1"])]
    labels = torch.from_numpy(np.random.default_rng(5).integers(0, 64, B)).cuda()
    ro = ProbeReadout(bc, "ro_attn", 0, other=others, ego=egos, labels=labels)
    r = {k: v.cpu().numpy() for k, v in bc.read(obs, pm, rm, ro).items()}
    h = bc.hidden(obs, pm, rm, tap="ro_attn", layer=0).cpu().numpy()
    lab = labels.cpu().numpy()
    n_dec = n_all = 0
    for q in range(2):
        Wo, bo = (heads["o%d" % q][k].numpy() for k in ("head.weight", "head.bias"))
        We, be = (heads["e%d" % q][k].numpy() for k in ("head.weight", "head.bias"))
        prime = (h[:, 0] + Wo[lab]).astype(np.float32)  # one float32 add per feature
        for x, W, b, got, what in ((h[:, 1:].reshape(-1, 64), Wo, bo, r["other_pred"][:, q].reshape(-1), "other_pred[%d]" % q),
                                   (h[:, 0], We, be, r["ego_pred"][:, q], "ego_pred[%d]" % q),
                                   (prime, We, be, r["ego_pred_prime"][:, q], "ego_pred_prime[%d]" % q)):
            d, n = _decided(x, W, b, got, what)
            n_dec, n_all = n_dec + d, n_all + n
    share = 1.0 - n_dec / n_all
    print("BC READOUT undecided %d of %d rows (%.4f %%)" % (n_all - n_dec, n_all, 100 * share))
    assert share <= 0.01
    assert (r["ego_pred_prime"] != r["ego_pred"]).any(), "the intervention changed no class"
    assert int(ro.bad_labels.item()) == 0


# ---- 4. exact corollaries

def test_zero_rows_bad_labels_and_twin_probes():
    from gpudrive_lab_amd import ProbeReadout
    B, A, R = 35, 64, 1
    bc = _policy(A, R, chunk_rows=32)
    obs, pm, rm, _, _ = _inp(B, A, R)
    ho = _head(51)
    ho["head.weight"][10] = 0.0  # label 10 adds nothing
    others = [_probe(bc, "late_lp", "other", 0, ho), _probe(bc, "late_lp", "other", 52), _probe(bc, "late_lp", "other", 0, ho)]
    egos = [_probe(bc, "late_lp", "ego", 61), _probe(bc, "late_lp", "ego", 62), _probe(bc, "late_lp", "ego", 61)]
    r = bc.read(obs, pm, rm, ProbeReadout(bc, "ro_attn", 0, other=others, ego=egos, labels=10))
    _same(r["ego_pred_prime"][:, 0], r["ego_pred"][:, 0], "a zero weight row")
    assert not torch.equal(r["ego_pred_prime"][:, 1], r["ego_pred"][:, 1]), "a non-zero row changed no class"
    for k in ("other_pred", "ego_pred", "ego_pred_prime"):  # identical weights at positions 0 and 2
        _same(r[k][:, 0], r[k][:, 2], "twin probes %s" % k)
    # labels outside 0 .. 63: no intervention, counted once per row
    lab = np.random.default_rng(3).integers(0, 64, B)
    bad = np.zeros(B, bool)
    for i, v in ((0, -1), (3, 64), (31, 1 << 40), (32, -(1 << 40)), (34, 255)):  # both chunks, both ego tiles
        lab[i], bad[i] = v, True
    ro = ProbeReadout(bc, "ro_attn", 0, other=others, ego=egos, labels=torch.from_numpy(lab).cuda())
    r2 = bc.read(obs, pm, rm, ro)
    badt = torch.from_numpy(bad).cuda()
    _same(r2["ego_pred_prime"][badt], r2["ego_pred"][badt], "out-of-range labels")
    assert int(ro.bad_labels.item()) == int(bad.sum())
    bc.read(obs, pm, rm, ro)
    assert int(ro.bad_labels.item()) == 2 * int(bad.sum()), "the counter accumulates over calls"
    every = ProbeReadout(bc, "ro_attn", 0, other=others, ego=egos, labels=64)  # an int: every row's label
    r3 = bc.read(obs, pm, rm, every)
    _same(r3["ego_pred_prime"], r3["ego_pred"], "label 64 for every row")
    assert int(every.bad_labels.item()) == B


# ---- 5. the row list

def test_read_on_a_row_list_writes_listed_rows_only():
    from gpudrive_lab_amd import ProbeReadout
    from gpudrive_lab_amd.policy import live_rows
    B, A, R = 35, 64, 1
    bc = _policy(A, R, chunk_rows=8)
    obs, pm, rm, _, _ = _inp(B, A, R)
    lab = np.random.default_rng(9).integers(0, 64, B)
    lab[[2, 5]] = -1, 64  # row 2 is listed, row 5 is not
    mk = lambda: ProbeReadout(bc, "ro_attn", 0, other=[_probe(bc, "late_lp", "other", 71)], ego=[_probe(bc, "late_lp", "ego", 72)],  # noqa: E731
                              labels=torch.from_numpy(lab).cuda())
    full_ro, list_ro = mk(), mk()
    full = bc.read(obs, pm, rm, full_ro)
    mask = torch.zeros(B, dtype=torch.bool, device="cuda")
    mask[[0, 2, 3, 9, 17, 33, 34]] = True
    lr = live_rows(mask)
    with pytest.raises(ValueError, match="rows= needs out="):
        bc.read(obs, pm, rm, list_ro, rows=lr, out={"actions": torch.empty_like(full["actions"])})
    out = {"actions": torch.full_like(full["actions"], 7.0)}
    wholes = {}
    for k in list_ro.names:
        out[k], wholes[k] = _canaried(tuple(full[k].shape))
    got = _no_sync(lambda: bc.read(obs, pm, rm, list_ro, rows=lr, out=out))
    for k in ("actions",) + list_ro.names:
        _same(got[k][mask], full[k][mask], "listed rows of %s" % k)
    assert bool((got["actions"][~mask] == 7.0).all())
    for k in list_ro.names:
        assert bool((got[k][~mask] == CANARY).all()), "%s: a row that is not listed was written" % k
        assert _guards_hold(wholes[k], out[k].numel()), k
    assert int(full_ro.bad_labels.item()) == 2 and int(list_ro.bad_labels.item()) == 1  # only listed rows count


# ---- 5b. more than one ego tile to a chunk

def _pairs(bc, labels):
    from gpudrive_lab_amd import ProbeReadout
    return ProbeReadout(bc, "ro_attn", 0, other=[_probe(bc, "late_lp", "other", 91), _probe(bc, "early_lp", "other", 92)],
                        ego=[_probe(bc, "late_lp", "ego", 93), _probe(bc, "early_lp", "ego", 94)], labels=labels)


@pytest.mark.parametrize("B,chunk", sorted(RR.TILE_CASES))
def test_a_rows_classes_do_not_depend_on_its_tile_or_chunk(B, chunk):
    """chunk_rows = 128 is every caller's default and no stand-alone call ran above 32: B = 130 gives 4 ego tiles, two slots
    per lane in the bad-label count and a second chunk of 2; B = chunk = 70 gives 3 ego tiles, the last with 6 live lanes, and
    lanes 0 .. 5 a second slot.  Every output is held bit for bit to the same read through a policy of chunk_rows = 32 -- one
    ego tile to a chunk, the tiling the float64 test and the probes' own kernels hold.  The labels outside 0 .. 63 sit where
    RR.TILE_CASES says, all at once and one at a time, and `bad_labels` is the exact number each time."""
    A, R = 64, 1
    bc, small = _policy(A, R, chunk_rows=chunk), _policy(A, R, chunk_rows=32)
    obs, pm, rm, _, _ = _inp(B, A, R)
    bad_rows = RR.TILE_CASES[(B, chunk)]
    assert -(-min(B, chunk) // 32) >= 3 and min(B, chunk) > 64 and all(0 <= r < B for r in bad_rows)
    for rows in (bad_rows,) + tuple((r,) for r in bad_rows) + ((),):
        lab = torch.from_numpy(RR.labels_with(B, rows)).cuda()
        ro, ros = _pairs(bc, lab), _pairs(small, lab)
        r, want = bc.read(obs, pm, rm, ro), small.read(obs, pm, rm, ros)
        what = "B=%d chunk=%d bad labels at %s" % (B, chunk, list(rows))
        for k in ("actions",) + ro.names:
            _same(r[k], want[k], "%s %s" % (what, k))
        assert int(ro.bad_labels.item()) == len(rows) == int(ros.bad_labels.item()), (what, int(ro.bad_labels.item()))
        badt = torch.zeros(B, dtype=torch.bool, device="cuda")
        badt[list(rows)] = True
        _same(r["ego_pred_prime"][badt], r["ego_pred"][badt], what + ": a bad label is no intervention")
        late = torch.arange(B, device="cuda") % chunk >= 32  # the rows of the ego tiles from the second on
        assert bool((r["ego_pred_prime"][late & ~badt] != r["ego_pred"][late & ~badt]).any()), what + ": no class changed in a later tile"


def test_a_row_list_of_more_than_64_rows():
    """The list instantiation at a chunk of 128 positions with more than 64 listed rows: four ego tiles, listed rows in the
    later ones, and a listed and an unlisted bad label at slots >= 64.  Listed rows equal the full read through chunk_rows = 32;
    rows that are not listed keep the canary; only listed rows count."""
    from gpudrive_lab_amd.policy import live_rows
    B, A, R = 130, 64, 1
    bc, small = _policy(A, R, chunk_rows=128), _policy(A, R, chunk_rows=32)
    obs, pm, rm, _, _ = _inp(B, A, R)
    mask_np, lab, listed_bad, unlisted_bad = RR.list_case(B)
    mask = torch.from_numpy(mask_np).cuda()
    assert int(mask.sum()) > 64 and all(mask_np[r] for r in listed_bad) and not any(mask_np[r] for r in unlisted_bad)
    position = np.cumsum(mask_np) - 1
    assert position[listed_bad[0]] == 0 and position[listed_bad[1]] >= 64 and unlisted_bad[0] >= 64
    labels = torch.from_numpy(lab).cuda()
    full_ro, list_ro = _pairs(small, labels), _pairs(bc, labels)
    full = small.read(obs, pm, rm, full_ro)
    out, wholes = {"actions": torch.full_like(full["actions"], 7.0)}, {}
    for k in list_ro.names:
        out[k], wholes[k] = _canaried(tuple(full[k].shape))
    got = _no_sync(lambda: bc.read(obs, pm, rm, list_ro, rows=live_rows(mask), out=out))
    for k in ("actions",) + list_ro.names:
        _same(got[k][mask], full[k][mask], "listed rows of %s" % k)
    assert bool((got["actions"][~mask] == 7.0).all())
    for k in list_ro.names:
        assert bool((got[k][~mask] == CANARY).all()), "%s: a row that is not listed was written" % k
        assert _guards_hold(wholes[k], out[k].numel()), k
    assert int(full_ro.bad_labels.item()) == 3 and int(list_ro.bad_labels.item()) == 2  # only listed rows count


# ---- 6. in the loop

LOOP = {  # name -> (A, R, dynamics, collision behaviour, labels, stochastic too)
    "128-5-removed": (128, 5, "delta_local", REMOVED, "rows", False),
    "128-5-ignore": (128, 5, "delta_local", IGNORE, 10, False),
    "64-1-removed": (64, 1, "delta_local", REMOVED, "rows", True),
    "64-1-removed-67-rows": (64, 1, "delta_local", REMOVED, "rows", False),
}
# The scenes of a case (the others: SCENES, 26 rows).  The three scenes give 2, 3 and 8 rows at A = 64, so N > 64 needs nine
# worlds, and nine are the fewest: eight times the largest scene and the second largest once, 67 rows -- three ego tiles to the
# loop's one chunk, the last with 3 live lanes, and three lanes with a second slot in the bad-label count.
LOOP_SCENES = {"64-1-removed-67-rows": [SCENES[2]] * 8 + [SCENES[1]]}
NEW = ("ego_attn_score", "other_pred", "ego_pred", "ego_pred_prime")
_CACHE = {}


class _Tapped:
    """The policy the restated loop calls: the real forward, and on the same obs[~dead] batch the stand-alone calls whose
    results the episode must hold -- context(ego_attn_score=) and read(...) -- kept per step.  `dead_mask` (the device run's,
    asserted equal to the restated loop's afterwards) tells which rows the batch holds, for the per-row labels."""

    def __init__(self, pol, make, labels, dead_mask):
        self.pol, self.make, self.labels, self.dead_mask = pol, make, labels, dead_mask
        self.steps, self.bad = [], 0

    def __call__(self, obs, pm, rm, deterministic=False, u=None, z=None):
        t = len(self.steps)
        rows = ~self.dead_mask[:, t]
        B, A = int(obs.shape[0]), self.pol.max_agents
        assert int(rows.sum()) == B
        score = torch.empty((B, 4, A - 1), dtype=torch.float32, device="cuda")
        self.pol.context(obs, pm, rm, ego_attn_score=score)
        ro = self.make(self.labels[rows].contiguous() if isinstance(self.labels, torch.Tensor) else self.labels)
        r = self.pol.read(obs, pm, rm, ro, deterministic=deterministic, u=u, z=z)
        actions = self.pol(obs, pm, rm, deterministic=deterministic, u=u, z=z)
        _same(r["actions"], actions, "read's actions at step %d" % t)
        self.bad += int(ro.bad_labels.item())
        self.steps.append((rows, dict(r, ego_attn_score=score)))
        return actions

    def expected(self, N, shapes):
        out = {k: torch.full((T, N) + s, 0.0 if k == "ego_attn_score" else 255,
                             dtype=torch.float32 if k == "ego_attn_score" else torch.uint8, device="cuda") for k, s in shapes.items()}
        for t, (rows, r) in enumerate(self.steps):
            for k in shapes:
                out[k][t, rows] = r[k]
        return out


def _loop_case(name):
    if name not in _CACHE:
        from gpudrive_lab_amd import ClosedLoopBC, ProbeReadout
        A, R, model, cb, labels, stochastic = LOOP[name]
        with _Env("linear"):
            scenes = LOOP_SCENES.get(name, SCENES)
            rsim, tsim = _sim(A, model, cb, "linear", scenes=scenes), _sim(A, model, cb, "linear", scenes=scenes)
            try:
                pol = _loop_policy(A, R)
                others = [_probe(pol, "late_lp", "other", 81), _probe(pol, "early_lp", "other", 82)]
                egos = [_probe(pol, "late_lp", "ego", 83), _probe(pol, "early_lp", "ego", 84)]
                make = lambda lab: ProbeReadout(pol, "ro_attn", 0, other=others, ego=egos, labels=lab)  # noqa: E731
                loop = ClosedLoopBC(rsim, pol)
                N = loop.num_agents
                if labels == "rows":
                    lab = np.random.default_rng(N).integers(0, 64, N)
                    lab[0], lab[N - 1] = 64, -1
                    labels = torch.from_numpy(lab).cuda()
                c = dict(N=N, A=A, loop_mask=loop.mask.clone(), row_slot=loop.row_slot.clone(), chunk_rows=pol.chunk_rows)
                c["plain"] = loop.run(record=True)
                c["plain_compact"] = loop.run(record=True, compact=True)
                ro, roc = make(labels), make(labels)
                c["ep"] = loop.run(attention=True, readout=ro, record=True)
                c["epc"] = loop.run(attention=True, readout=roc, record=True, compact=True)
                c["attn_only"] = loop.run(attention=True)
                c["readout_only"] = loop.run(readout=make(labels), compact=True)
                torch.cuda.synchronize()
                c["bad"] = (int(ro.bad_labels.item()), int(roc.bad_labels.item()))
                tapped = _Tapped(pol, make, labels, c["ep"].dead_mask)
                c["r"] = _loop(tsim, tapped, model, R)
                c["shapes"] = dict(ego_attn_score=(4, A - 1), **{k: ro.row_shape(k) for k in ro.names})
                c["want"], c["want_bad"] = tapped.expected(N, c["shapes"]), tapped.bad
                if stochastic:
                    seed = lambda: torch.Generator(device="cuda").manual_seed(5)  # noqa: E731
                    c["s_plain"] = loop.run(deterministic=False, generator=seed(), record=True)
                    c["s_ep"] = loop.run(deterministic=False, generator=seed(), record=True, attention=True, readout=make(labels))
                    torch.cuda.synchronize()
                    st = _Tapped(pol, make, labels, c["s_ep"].dead_mask)
                    c["s_r"] = _loop(tsim, st, model, R, deterministic=False, u=c["s_ep"].u, z=c["s_ep"].z)
                    c["s_want"] = st.expected(N, c["shapes"])
            finally:
                rsim.close()
                tsim.close()
        _CACHE[name] = c
    return _CACHE[name]


def _same_fields(a, b, what, skip=()):
    """Every tensor field of episode b is in a with the same bits."""
    for k, v in b.__dict__.items():
        if isinstance(v, torch.Tensor) and k not in skip:
            _same(getattr(a, k), v, "%s %s" % (what, k))


@pytest.mark.parametrize("name", sorted(LOOP))
def test_run_with_the_read_outs_equals_the_restated_loop(name):
    c = _loop_case(name)
    ep, epc, r, N, want = c["ep"], c["epc"], c["r"], c["N"], c["want"]
    _same(ep.dead_mask, r["dead_mask"], "dead_mask")  # (what _Tapped took the batches' rows from)
    iters = r["iterations"]
    dead = ep.dead_mask.t()  # [T, N]
    print("BC READOUT LOOP %s: rows %d iterations %d live row-steps %d dead row-steps %d bad %s"
          % (name, N, iters, int((~dead[:iters]).sum()), int(dead[:iters].sum()), c["bad"]))
    assert bool(dead[:iters].any()) and bool((~dead[:iters]).any()), "the case has no dead or no live row-step"
    # how many rows a chunk of the loop's forward holds: run() reads all N rows in chunks of chunk_rows (dead rows dropped
    # inside the launch), run(compact=True) the live rows of the step
    live_most = int((~dead[:iters]).sum(1).max())
    print("BC READOUT LOOP %s: N %d, most live rows in a step %d, chunk_rows %d" % (name, N, live_most, c["chunk_rows"]))
    assert c["chunk_rows"] == 128 and live_most <= N <= c["chunk_rows"], "one chunk per step: the chunk holds N rows"
    if name in LOOP_SCENES:
        assert N == 67 and live_most > 64, "more than two ego tiles, and a second slot per lane in the bad-label count"
        late = (~dead[:iters])[:, 32:].any(1)
        assert bool(late.any()) and bool((ep.ego_pred_prime[:iters][late][:, 32:] != 255).any()), "no live row in a later ego tile"
    else:
        assert N == 26, "26 rows: one ego tile per chunk (the case of 67 rows has three)"
    for k in c["shapes"]:
        assert tuple(getattr(ep, k).shape) == (T, N) + c["shapes"][k]
        _same(getattr(ep, k), want[k], "%s %s" % (name, k))
        _same(getattr(epc, k), want[k], "%s compact %s" % (name, k))
        fill = 0.0 if k == "ego_attn_score" else 255
        assert bool((getattr(ep, k)[dead] == fill).all()) and bool((getattr(ep, k)[iters:] == fill).all()), k
        assert bool((getattr(ep, k)[~dead] != fill).flatten(1).any(1).all()), "%s: a live row holds only the fill" % k
    assert c["bad"] == (c["want_bad"], c["want_bad"]) and (c["want_bad"] > 0) == (LOOP[name][4] == "rows")
    # every field the episode had before is the plain run's
    _same_fields(ep, c["plain"], name)
    _same_fields(epc, c["plain_compact"], name + " compact", skip=("live_rows",))
    # each option alone
    _same(c["attn_only"].ego_attn_score, want["ego_attn_score"], "attention alone")
    assert not hasattr(c["attn_only"], "ego_pred") and not hasattr(c["readout_only"], "ego_attn_score")
    for k in c["shapes"]:
        if k != "ego_attn_score":
            _same(getattr(c["readout_only"], k), want[k], "readout alone %s" % k)


def test_run_with_the_read_outs_and_the_draw():
    c = _loop_case("64-1-removed")
    _same_fields(c["s_ep"], c["s_plain"], "the draw")
    _same(c["s_ep"].dead_mask, c["s_r"]["dead_mask"], "the draw dead_mask")
    _same(c["s_ep"].actions, c["s_r"]["actions"], "the draw actions")
    for k in c["shapes"]:
        _same(getattr(c["s_ep"], k), c["s_want"][k], "the draw %s" % k)
    assert not torch.equal(c["s_ep"].actions, c["ep"].actions), "the draw changed nothing"


def test_world_importance_is_the_reference_scatter():
    """importance_weight.py:75-78 on the recorded dead_mask.  The reference hands masked_scatter the scores of ALL live rows and
    lets it consume them in order, which assigns a world the wrong rows' scores as soon as an earlier world has several live
    rows; the source below is the scores of the rows of the worlds that are filled, which is what the three lines mean."""
    c = _loop_case("128-5-removed")
    ep, N, A = c["ep"], c["N"], c["A"]
    mask = c["loop_mask"]
    W = mask.shape[0]
    found = False
    for t in range(T):
        dead_agent_mask = torch.ones((W, A), dtype=torch.bool, device="cuda")
        dead_agent_mask[mask] = ep.dead_mask[:, t]
        live_per_world = (~dead_agent_mask).sum(dim=-1)
        if not (bool((live_per_world == 1).any()) and bool((live_per_world != 1).any())):
            continue
        found = True
        world_mask = live_per_world == 1
        rows_live = ~ep.dead_mask[:, t]
        row_world = torch.div(c["row_slot"].long(), A, rounding_mode="floor")
        importance_weight = ep.ego_attn_score[t][rows_live & world_mask[row_world]]
        world_importance_weight = torch.zeros((W, 4, A), device="cuda")
        multi_head_mask = dead_agent_mask.unsqueeze(1).repeat(1, 4, 1)
        world_importance_weight[world_mask] = world_importance_weight[world_mask].masked_scatter(multi_head_mask[world_mask],
                                                                                                 importance_weight)
        got = _no_sync(lambda: ep.world_importance(t))
        _same(got, world_importance_weight, "world_importance(%d)" % t)
        assert bool((got[world_mask] != 0).any()) and bool((got[~world_mask] == 0).all())
    assert found, "no step has a world with one live row beside a world with none or several"
    with pytest.raises(ValueError, match="attention=True"):
        c["plain"].world_importance(0)


def test_run_makes_no_host_synchronisation():
    from gpudrive_lab_amd import ClosedLoopBC, ProbeReadout
    A, R = 64, 1
    with _Env("linear"):
        sim = _sim(A, "delta_local", REMOVED, "linear")
        try:
            pol = _loop_policy(A, R)
            ro = ProbeReadout(pol, "ro_attn", 0, other=[_probe(pol, "late_lp", "other", 1)], ego=[_probe(pol, "late_lp", "ego", 2)],
                              labels=3)
            loop = ClosedLoopBC(sim, pol)
            first = loop.run(n_steps=3, attention=True, readout=ro)  # (the first step of a simulator may build its launch plan)
            for compact in (False, True):
                ep = _no_sync(lambda: loop.run(n_steps=3, attention=True, readout=ro, compact=compact))
                for k in NEW:
                    _same(getattr(ep, k), getattr(first, k), "compact=%s %s" % (compact, k))
            assert bool((first.ego_pred[3:] == 255).all()) and bool((first.ego_attn_score[3:] == 0).all())
        finally:
            sim.close()


# ---- 7. the C calls refuse before any launch

def test_c_level_refusals_launch_nothing():
    from gpudrive_lab_amd import ProbeReadout
    B, A, R = 3, 64, 1
    bc = _policy(A, R, chunk_rows=2)
    obs, pm, rm, _, _ = _inp(B, A, R)
    ro = ProbeReadout(bc, "ro_attn", 0, other=[_probe(bc, "late_lp", "other", 1)], ego=[_probe(bc, "late_lp", "ego", 2)],
                      labels=torch.zeros(B + 1, dtype=torch.int64, device="cuda")[:B])
    L = _capi.lib()
    actions = torch.full((B, 1, 3), 7.0, device="cuda")
    outs, wholes = {}, {}
    for k in ro.names:
        outs[k], wholes[k] = _canaried((B,) + ro.row_shape(k))

    def call(policy=None, **change):
        s, _ = ro.bind((B,), outs)
        for k, v in change.items():
            setattr(s, k, v)
        p = policy if policy is not None else bc.c_struct()
        o = _capi.GdBCOutputs(actions=actions.data_ptr())
        rc = L.gd_bc_forward_readout(ctypes.byref(p), obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), B, 1, None, None, None,
                                     ctypes.byref(o), ctypes.byref(s), None)
        return rc, L.gd_last_error().decode()

    detached = bc.c_struct()
    detached.scratch = None
    for kw, match in ((dict(other_pred=None), "output of a non-zero count is null"), (dict(ego_pred_prime=None), "output of a non-zero"),
                      (dict(layer=2), "layer must be in"), (dict(layer=-1), "layer must be in"), (dict(tap=2), "tap must be"),
                      (dict(labels=ro.labels.data_ptr() + 4), "labels must be 8-byte aligned"),
                      (dict(policy=detached), "blob and scratch are required"), (dict(n_other=9), r"must be in \[0, 8\]"),
                      (dict(n_ego=0), "intervene needs"), (dict(bad_labels=None), "bad_labels is required"),
                      (dict(other_stride=A - 2), "stride is below")):
        rc, msg = call(**kw)
        assert rc == _capi.GD_ERR_INVALID and "gd_bc_forward_readout" in msg, (kw, rc, msg)
        import re
        assert re.search(match, msg), (kw, msg)
    torch.cuda.synchronize()
    assert bool((actions == 7.0).all())
    for k in ro.names:
        assert bool((wholes[k] == CANARY).all()), "%s was written by a refused call" % k
    rc, msg = call()
    assert rc == _capi.GD_OK, msg
    torch.cuda.synchronize()
    assert bool((actions != 7.0).any()) and all(bool((outs[k] < 64).all()) for k in ro.names)
