"""Which of two faults a BC entry point reports.  The six gd_bc_forward*, the four gd_bc_rollout* and the two gd_bc_hidden*
entries share one checked forward, one checked loop and one body (csrc/engine.cpp); merging entry points can silently change
the order in which they refuse, so every call here carries two faults at once and the fault that is checked first must be the
one in `gd_last_error`, word for word, behind the entry's own name.

No GPU: every pointer is a fake non-null address (4096) and the simulator is one too; each call is refused before anything
is read through them.  The last case of the loops (n_steps = 92 behind buffers that are all there) is the last check that does
not dereference the simulator.  The strings were taken from the library as it was before the entries were merged."""
import ctypes as C

import pytest

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import bc_policy as BP

PTR = 4096
R, LAYERS, HL, NC, A, CHUNK = 5, (4, 3), 2, 6, 64, 8

FORWARDS = ("gd_bc_forward", "gd_bc_forward_rows", "gd_bc_forward_readout", "gd_bc_forward_rows_readout", "gd_bc_forward_dim",
            "gd_bc_forward_rows_dim")
ROLLOUTS = ("gd_bc_rollout", "gd_bc_rollout_compact", "gd_bc_rollout_readout", "gd_bc_rollout_dim")
HIDDEN = ("gd_bc_hidden", "gd_bc_hidden_layer")

MAX_AGENTS = "max_agents must be 64 or 128"
NETWORK_DIM = "network_dim must be 64 or 128"
TAP = "readout: tap must be GD_LP_TAP_FUSION or GD_LP_TAP_RO"
NO_READOUT = "readout is required"
NO_ROWS = "rows and count are required"
NULL = "null argument"
LIST_RESERVED = "the row list's reserved must be 0"
NO_READS = "reads needs ego_attn_score or readout"
READOUT_128 = "reads->readout must be NULL unless network_dim is 64 (the probes read 64-wide tokens)"
NO_BUFFERS = "every buffer but the per-step records is required"
STEPS = "an episode has 91 steps, n_steps must be in [1, 91]"
HIDDEN_TAP = "tap must be GD_LP_TAP_FUSION or GD_LP_TAP_RO"
HIDDEN_LAYER = "layer must be in [0, layers of the tapped block)"
HIDDEN_OUT = "out is required, 16-byte aligned"


def policy(dim=64, **over):
    """A gd_bc_policy_dim that every check accepts at `dim` (its base is the gd_bc_policy of the entries without a width);
    over: fields of either struct to spoil."""
    p = _capi.GdBCPolicyDim()
    b = p.base
    b.max_agents, b.num_stack, b.fusion_layers, b.branch_layers, b.head_layers, b.n_components = A, R, *LAYERS, HL, NC
    b.clip_value, b.chunk_rows, b.blob, b.scratch = -20.0, CHUNK, PTR, PTR
    b.blob_floats = int(BP.pack_index(R, LAYERS, HL, NC, network_dim=dim).size)
    b.scratch_floats = BP.scratch_floats(A, CHUNK, dim)
    p.network_dim, p.reserved = dim, 0
    for k, v in over.items():
        setattr(p if k in ("network_dim", "reserved") else b, k, v)
    return p


def readout(**over):
    """A gd_bc_readout that bc_readout_problem accepts: one 'ego' probe after ro_attn's first layer."""
    r = _capi.GdBCReadout()
    r.tap, r.layer, r.n_ego, r.ego_pred, r.ego_stride = _capi.LP_TAP_RO, 0, 1, PTR, 1
    r.ego[0].packed = PTR
    for k, v in over.items():
        setattr(r, k, v)
    return r


def row_list(**over):
    r = _capi.GdBCRolloutRows()
    r.rows = r.count = r.scratch = PTR
    for k, v in over.items():
        setattr(r, k, v)
    return r


def reads(ro=None, score=None):
    x = _capi.GdBCRolloutReads()
    x.ego_attn_score = score
    if ro is not None:
        x.readout = C.pointer(ro)
    return x


def buffers(full):
    """gd_bc_rollout_buffers with no buffer at all, or with every buffer there and a valid n_rows."""
    b = _capi.GdBCRolloutBuffers()
    if full:
        for name, kind in b._fields_:
            if kind is C.c_void_p:
                setattr(b, name, PTR)
        b.n_rows, b.deterministic = 4, 1
    return b


def forward(entry, p, ro=None, rows=PTR, count=PTR, n=4):
    """The call of a forward entry: ro and rows / count go to the entries that take them."""
    L, o = _capi.lib(), _capi.GdBCOutputs()
    args = [C.byref(p) if entry.endswith("_dim") else C.byref(p.base), PTR, PTR, PTR, n, 1, None, None, None, C.byref(o)]
    if "readout" in entry:
        args.append(None if ro is None else C.byref(ro))
    if "rows" in entry:
        args += [rows, count]
    return getattr(L, entry)(*args, None)


def rollout(entry, p, b, r=None, x=None, n_steps=91, sim=PTR):
    """The call of a loop entry: r and x go to the entries that take them."""
    L = _capi.lib()
    args = [sim, C.byref(p) if entry.endswith("_dim") else C.byref(p.base), C.byref(b)]
    if entry != "gd_bc_rollout":
        args.append(None if r is None else C.byref(r))
    if entry in ("gd_bc_rollout_readout", "gd_bc_rollout_dim"):
        args.append(None if x is None else C.byref(x))
    return getattr(L, entry)(*args, n_steps)


def hidden(entry, p, tap, layer, out):
    L = _capi.lib()
    args = [C.byref(p.base), PTR, PTR, PTR, 4, tap] + ([layer] if entry == "gd_bc_hidden_layer" else []) + [out, None]
    return getattr(L, entry)(*args)


BAD_POLICY, BAD_TAP = dict(max_agents=65), dict(tap=7)

# (entry, the call with two faults, the fault that must be reported)
CASES = [
    # the policy over n
    ("gd_bc_forward", lambda e: forward(e, policy(**BAD_POLICY), n=0), MAX_AGENTS),
    # a bad network_dim over a bad max_agents
    ("gd_bc_forward_dim", lambda e: forward(e, policy(network_dim=96, **BAD_POLICY)), NETWORK_DIM),
    ("gd_bc_forward_rows_dim", lambda e: forward(e, policy(network_dim=96, **BAD_POLICY)), NETWORK_DIM),
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(network_dim=96, **BAD_POLICY), buffers(True)), NETWORK_DIM),
    # the _dim struct over the row list, and NULL arguments over the _dim struct
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(128, reserved=1), buffers(True), r=row_list(reserved=1)), "reserved must be 0"),
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(network_dim=96), buffers(True), sim=None), NULL),
    # a bad policy over a bad read-out tap
    ("gd_bc_forward_readout", lambda e: forward(e, policy(**BAD_POLICY), ro=readout(**BAD_TAP)), MAX_AGENTS),
    ("gd_bc_forward_rows_readout", lambda e: forward(e, policy(**BAD_POLICY), ro=readout(**BAD_TAP)), MAX_AGENTS),
    # a bad read-out over NULL rows
    ("gd_bc_forward_rows_readout", lambda e: forward(e, policy(), ro=readout(**BAD_TAP), rows=None, count=None), TAP),
    # a bad policy over NULL rows
    ("gd_bc_forward_rows", lambda e: forward(e, policy(**BAD_POLICY), rows=None, count=None), MAX_AGENTS),
    ("gd_bc_forward_rows_readout", lambda e: forward(e, policy(**BAD_POLICY), ro=readout(), rows=None, count=None), MAX_AGENTS),
    ("gd_bc_forward_rows_dim", lambda e: forward(e, policy(128, **BAD_POLICY), rows=None, count=None), MAX_AGENTS),
    # a NULL read-out where one is required (over NULL rows where both are), a NULL list where one is required
    ("gd_bc_forward_readout", lambda e: forward(e, policy(), ro=None), NO_READOUT),
    ("gd_bc_forward_rows_readout", lambda e: forward(e, policy(), ro=None, rows=None, count=None), NO_READOUT),
    ("gd_bc_forward_rows_readout", lambda e: forward(e, policy(), ro=readout(), rows=None), NO_ROWS),
    ("gd_bc_forward_rows", lambda e: forward(e, policy(), count=None), NO_ROWS),
    ("gd_bc_forward_rows_dim", lambda e: forward(e, policy(128), rows=None, count=None), NO_ROWS),
    ("gd_bc_rollout_compact", lambda e: rollout(e, policy(), buffers(False), r=None, n_steps=0), NULL),
    ("gd_bc_rollout_readout", lambda e: rollout(e, policy(), buffers(False), r=row_list(reserved=1), x=None), NULL),
    # the row list's reserved over empty reads (over missing buffers where the entry takes no reads)
    ("gd_bc_rollout_compact", lambda e: rollout(e, policy(), buffers(False), r=row_list(reserved=1)), LIST_RESERVED),
    ("gd_bc_rollout_readout", lambda e: rollout(e, policy(), buffers(True), r=row_list(reserved=1), x=reads()), LIST_RESERVED),
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(128), buffers(True), r=row_list(reserved=1), x=reads()), LIST_RESERVED),
    # empty reads over missing buffers
    ("gd_bc_rollout_readout", lambda e: rollout(e, policy(), buffers(False), x=reads()), NO_READS),
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(128), buffers(False), r=row_list(), x=reads()), NO_READS),
    # a read-out at 128 over missing buffers
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(128), buffers(False), x=reads(readout())), READOUT_128),
    # missing buffers over n_steps = 0
    ("gd_bc_rollout", lambda e: rollout(e, policy(), buffers(False), n_steps=0), NO_BUFFERS),
    ("gd_bc_rollout_compact", lambda e: rollout(e, policy(), buffers(False), r=row_list(), n_steps=0), NO_BUFFERS),
    ("gd_bc_rollout_readout", lambda e: rollout(e, policy(), buffers(False), x=reads(score=PTR), n_steps=0), NO_BUFFERS),
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(128), buffers(False), n_steps=0), NO_BUFFERS),
    # n_steps = 92 behind buffers that are all there: the last check that does not dereference the simulator
    ("gd_bc_rollout", lambda e: rollout(e, policy(), buffers(True), n_steps=92), STEPS),
    ("gd_bc_rollout_compact", lambda e: rollout(e, policy(), buffers(True), r=row_list(), n_steps=92), STEPS),
    ("gd_bc_rollout_readout", lambda e: rollout(e, policy(), buffers(True), r=row_list(), x=reads(readout(**BAD_TAP)), n_steps=92),
     STEPS),
    ("gd_bc_rollout_dim", lambda e: rollout(e, policy(128), buffers(True), r=row_list(), x=reads(score=PTR), n_steps=92), STEPS),
    # the hidden states: the policy, then the tap, then the layer (gd_bc_hidden_layer only), then out
    ("gd_bc_hidden", lambda e: hidden(e, policy(**BAD_POLICY), 7, None, None), MAX_AGENTS),
    ("gd_bc_hidden", lambda e: hidden(e, policy(), 7, None, None), HIDDEN_TAP),
    ("gd_bc_hidden", lambda e: hidden(e, policy(), _capi.LP_TAP_RO, None, 8), HIDDEN_OUT),
    ("gd_bc_hidden_layer", lambda e: hidden(e, policy(**BAD_POLICY), 7, -1, None), MAX_AGENTS),
    ("gd_bc_hidden_layer", lambda e: hidden(e, policy(), 7, -1, None), HIDDEN_TAP),
    ("gd_bc_hidden_layer", lambda e: hidden(e, policy(), _capi.LP_TAP_RO, -1, None), HIDDEN_LAYER),
    ("gd_bc_hidden_layer", lambda e: hidden(e, policy(), _capi.LP_TAP_RO, LAYERS[1], None), HIDDEN_LAYER),
    ("gd_bc_hidden_layer", lambda e: hidden(e, policy(), _capi.LP_TAP_FUSION, LAYERS[1], None), HIDDEN_OUT),
]


def test_every_entry_is_in_the_table():
    assert {c[0] for c in CASES} == set(FORWARDS + ROLLOUTS + HIDDEN)
    assert set(FORWARDS + ROLLOUTS + HIDDEN) <= set(_capi.SYMBOLS)


@pytest.mark.parametrize("entry,call,fault", CASES, ids=["%02d-%s" % (i, c[0]) for i, c in enumerate(CASES)])
def test_the_first_fault_is_the_one_reported(entry, call, fault):
    assert call(entry) == _capi.GD_ERR_INVALID
    assert _capi.lib().gd_last_error().decode() == entry + ": " + fault


def test_the_shared_list_check_in_the_ppo_loop():
    """gd_policy_rollout_rows has gd_bc_rollout_rows' fields and gd_policy_rollout_compact the same check of them, in the same
    order, before anything of the policy or the buffers is read."""
    L = _capi.lib()
    p, b = C.byref(_capi.GdPolicy()), _capi.GdPolicyRolloutBuffers()
    for over, fault in ((dict(count=None, scratch=None), NO_ROWS),
                        (dict(scratch=None, live_count=2), "scratch is required and must be 4-byte aligned"),
                        (dict(live_count=2, reserved=1), "live_count must be 4-byte aligned"),
                        (dict(reserved=1), LIST_RESERVED)):
        r = _capi.GdPolicyRolloutRows()
        r.rows = r.count = r.scratch = PTR
        for k, v in over.items():
            setattr(r, k, v)
        assert L.gd_policy_rollout_compact(PTR, p, C.byref(b), C.byref(r), 0) == _capi.GD_ERR_INVALID
        assert L.gd_last_error().decode() == "gd_policy_rollout_compact: " + fault
    assert L.gd_policy_rollout_compact(PTR, p, C.byref(b), None, 0) == _capi.GD_ERR_INVALID
    assert L.gd_last_error().decode() == "gd_policy_rollout_compact: null argument"
