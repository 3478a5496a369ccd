"""CPU tests of the probe read-outs (gd_bc_hidden_layer, gd_bc_forward_readout, gd_bc_forward_rows_readout,
gd_bc_rollout_readout; gpudrive_lab_amd.bc_readout.ProbeReadout): the surface, the structs against the header, the rule
(csrc/bc_readout_rule.hpp as a host program) against numpy float32 on constructed logits, every refusal that needs no device,
and the byte count."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from gpudrive_lab_amd import _capi
from tests import bc_readout_reference as RR
from tests.conftest import ROOT
from tests.test_bc_live_rows import OK4, OK16, ODD, _buffers, _policy_struct, _refused
from tests.test_bc_rollout import _stub_policy

HEADER = open(os.path.join(ROOT, "include", "gpudrive_amd.h")).read()
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {"gd_bc_hidden_layer": 9, "gd_bc_forward_readout": 12, "gd_bc_forward_rows_readout": 14, "gd_bc_rollout_readout": 6}


def _declared_args(name):
    decl = re.search(r"^int %s\((.*?)\);" % name, HEADER, flags=re.S | re.M).group(1)
    return [a.strip() for a in decl.split(",")]


def _struct_fields(name):
    body = HEADER[HEADER.index("typedef struct %s {" % name):HEADER.index("} %s;" % name)]
    code = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"[ *](\w+)(?:\[\w+\])?[,;]", code)


# ---- the surface

def test_the_symbols_are_declared_exported_and_bound():
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = _capi.lib()
    for name, n_args in NAMES.items():
        assert len(_declared_args(name)) == n_args, (name, _declared_args(name))
        assert name in _capi.SYMBOLS and name in exported
        assert len(getattr(L, name).argtypes) == n_args, name
    # the forwards' arguments with the read-out after `out`; gd_bc_hidden's with the layer after the tap
    fwd, rows = _declared_args("gd_bc_forward"), _declared_args("gd_bc_forward_rows")
    assert _declared_args("gd_bc_forward_readout") == fwd[:-1] + ["const gd_bc_readout *readout"] + fwd[-1:]
    assert _declared_args("gd_bc_forward_rows_readout") == rows[:10] + ["const gd_bc_readout *readout"] + rows[10:]
    hid = _declared_args("gd_bc_hidden")
    assert _declared_args("gd_bc_hidden_layer") == hid[:6] + ["int32_t layer"] + hid[6:]
    ro = _declared_args("gd_bc_rollout_compact")
    assert _declared_args("gd_bc_rollout_readout") == ro[:-1] + ["const gd_bc_rollout_reads *reads"] + ro[-1:]
    assert L.gd_bc_forward_readout.argtypes[10]._type_ is _capi.GdBCReadout
    assert L.gd_bc_forward_rows_readout.argtypes[10]._type_ is _capi.GdBCReadout
    at = L.gd_bc_rollout_readout.argtypes
    assert at[3]._type_ is _capi.GdBCRolloutRows and at[4]._type_ is _capi.GdBCRolloutReads


def test_the_structs_have_the_headers_fields():
    P, R, X = _capi.GdBCReadoutProbe, _capi.GdBCReadout, _capi.GdBCRolloutReads
    assert [f[0] for f in P._fields_] == _struct_fields("gd_bc_readout_probe") == ["packed", "weight"] and ctypes.sizeof(P) == 16
    names = [f[0] for f in R._fields_]
    assert names == _struct_fields("gd_bc_readout"), "the header declares other fields, or in another order"
    assert names == ["tap", "layer", "n_other", "n_ego", "intervene", "reserved", "other", "ego", "labels", "label", "other_pred",
                     "ego_pred", "ego_pred_prime", "other_stride", "ego_stride", "prime_stride", "bad_labels"]
    # six int32, 2 x 8 probes of two pointers, then eight-byte members only
    assert [getattr(R, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 152] + [280 + 8 * i for i in range(9)]
    assert ctypes.sizeof(R) == 352 and _capi.BC_READOUT_MAX == 8 and "enum { GD_BC_READOUT_MAX = 8 };" in HEADER
    assert [f[0] for f in X._fields_] == _struct_fields("gd_bc_rollout_reads") == ["ego_attn_score", "readout"]
    assert ctypes.sizeof(X) == 16


def test_exported_from_the_package():
    import gpudrive_lab_amd
    from gpudrive_lab_amd.bc_readout import ProbeReadout
    assert gpudrive_lab_amd.ProbeReadout is ProbeReadout


# ---- the rule

def _rule_host(sanitize=False):
    """The compiled host program; sanitize: a second, stand-alone executable with -fsanitize=address,undefined."""
    out = os.path.join(tempfile.gettempdir(), "gd_bc_readout_rule_host%s_%d" % ("_san" if sanitize else "", os.getuid()))
    src = os.path.join(HERE, "bc_readout_rule_host.cpp")
    hdrs = [os.path.join(ROOT, "gpudrive_lab_amd", "csrc", h) for h in ("bc_readout_rule.hpp", "lp_rule.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [src] + hdrs):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out, src])
    return out


def _run_rule(logits, w, h, labels, sanitize=False):
    n, m = len(logits), len(h)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, m], np.int32).tobytes() + np.asarray(logits, np.float32).tobytes() + np.asarray(w, np.float32).tobytes()
                    + np.asarray(h, np.float32).tobytes() + np.asarray(labels, np.int64).tobytes())
        subprocess.check_call([_rule_host(sanitize), fin, fout])
        raw = open(fout, "rb").read()
    assert len(raw) == n + m + 4 * 64 * m + 4
    cls, ok = np.frombuffer(raw[:n], np.uint8), np.frombuffer(raw[n:n + m], np.uint8)
    hp = np.frombuffer(raw[n + m:n + m + 4 * 64 * m], np.float32).reshape(m, 64)
    return cls, ok, hp, int(np.frombuffer(raw[-4:], np.int32)[0])


def test_the_rule_against_numpy_float32():
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((40, 64)).astype(np.float32)
    logits[0] = 0.0                                   # every class ties: the first
    logits[1, [5, 9, 63]] = 7.0                       # three-way tie of the maximum: 5
    logits[2, 63] = 9.0                               # the last class
    logits[3, [0, 1]] = logits[3].max() + 1           # a tie at the front
    logits[4] = -np.float32(3e38)
    logits[4, 17] = -np.float32(2.9e38)               # huge negatives
    logits[5] = np.nan                                # a NaN is never greater: 0
    logits[6, 10], logits[6, 11] = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))  # one ulp apart: 11
    logits[6, 12:] = -1.0
    logits[6, :10] = -1.0
    w = (rng.standard_normal((64, 64)) * 3).astype(np.float32)
    w[10] = 0.0
    h = rng.standard_normal((12, 64)).astype(np.float32)
    h[3] = np.float32(1e8)                            # the add rounds: 1e8 + w is not exact
    labels = np.array([0, 63, 10, 5, -1, 64, 1 << 40, -(1 << 40), 33, 7, 255, 62], np.int64)
    cls, ok, hp, bad = _run_rule(logits, w, h, labels)
    want = np.array([int(np.argmax(np.nan_to_num(z, nan=-np.inf))) if not np.isnan(z).all() else 0 for z in logits])
    assert np.array_equal(cls, want) and list(cls[:7]) == [0, 5, 63, 0, 17, 0, 11]
    good = (labels >= 0) & (labels < 64)
    assert np.array_equal(ok.astype(bool), good) and bad == int((~good).sum()) == 5
    for i in range(len(h)):
        expect = (np.float32(h[i]) + np.float32(w[labels[i]])) if good[i] else h[i]  # np.float32(h) + np.float32(v), or h's own bits
        assert expect.dtype == np.float32 and np.array_equal(hp[i].view(np.int32), expect.view(np.int32)), i
    assert np.array_equal(hp[2].view(np.int32), h[2].view(np.int32))  # label 10: a zero row adds nothing
    assert not np.array_equal(hp[3], h[3] + w[labels[3]].astype(np.float64))  # (the rounding above happened)


def test_the_rule_host_program_under_the_sanitizers():
    """Labels far outside the weight matrix: the stand-alone program never indexes it with them."""
    rng = np.random.default_rng(1)
    logits, w, h = (rng.standard_normal(s).astype(np.float32) for s in ((9, 64), (64, 64), (6, 64)))
    labels = np.array([63, 64, -1, np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0], np.int64)
    plain, san = _run_rule(logits, w, h, labels), _run_rule(logits, w, h, labels, sanitize=True)
    assert all(np.array_equal(a, b) for a, b in zip(plain[:3], san[:3])) and plain[3] == san[3] == 4


# ---- the launch by chunk, tile and lane, and the wrong rules the larger cases are built to see

WRONG = ("bad_first_64", "prime_tile0", "probe_cap3", "stride_A")


def _tokens(B, A, seed=2):
    return np.random.default_rng(seed).standard_normal((B, A, 64)).astype(np.float32)


def _old_cases():
    """The calls of test_gpu_bc_readout.py before the larger cases: at most 32 rows to a chunk, at most 3 probes to a list."""
    lab35 = RR.labels_with(35, (0, 3, 31, 32, 34), seed=3)
    lab_list = RR.labels_with(35, (2, 5), seed=9)
    return {"2+1, no labels": dict(B=35, A=64, n=(2, 1), labels=None, chunk_rows=32),
            "3+3, bad labels in both chunks": dict(B=35, A=64, n=(3, 3), labels=lab35, chunk_rows=32),
            "2+2 at R = 5": dict(B=35, A=64, n=(2, 2), labels=RR.labels_with(35, ()), chunk_rows=32),
            "1+1 on a list": dict(B=35, A=64, n=(1, 1), labels=lab_list, chunk_rows=8, rows=[0, 2, 3, 9, 17, 33, 34]),
            "1+1, one label": dict(B=5, A=64, n=(1, 1), labels=7, chunk_rows=4)}


def _new_cases():
    mask, lab, _, _ = RR.list_case()
    out = {"%d rows in chunks of %d" % k: dict(B=k[0], A=64, n=(2, 2), labels=RR.labels_with(k[0], bad), chunk_rows=k[1])
           for k, bad in RR.TILE_CASES.items()}
    out["a list of more than 64 rows"] = dict(B=130, A=64, n=(2, 2), labels=lab, chunk_rows=128, rows=np.nonzero(mask)[0])
    for A in (64, 128):
        out["8+8 at A = %d" % A] = dict(B=35, A=A, n=(8, 8), labels=RR.labels_with(35, ()), chunk_rows=32)
    return out


def _read(c, wrong=None):
    h = _tokens(c["B"], c["A"])
    return RR.read(h, RR.probe_heads(c["n"][0], 31), RR.probe_heads(c["n"][1], 41), labels=c["labels"], chunk_rows=c["chunk_rows"],
                   rows=c.get("rows"), wrong=wrong)


def _equal(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_the_restated_launch_does_not_depend_on_the_chunk():
    """What the GPU cases hold the device to: a row's classes are the same whichever tile or chunk it sits in, the count is the
    number of rows read whose label is no class, and rows that are not listed keep the fill."""
    for name, c in dict(_old_cases(), **_new_cases()).items():
        r = _read(c)
        one = _read(dict(c, chunk_rows=1))
        assert _equal(r, one), name
        rows = np.arange(c["B"]) if c.get("rows") is None else np.asarray(c["rows"])
        lab = None if c["labels"] is None else np.broadcast_to(np.asarray(c["labels"]), (c["B"],))
        assert r["bad"] == (0 if lab is None else int(((lab[rows] < 0) | (lab[rows] > 63)).sum())), name
        unlisted = np.setdiff1d(np.arange(c["B"]), rows)
        for k in ("other_pred", "ego_pred", "ego_pred_prime"):
            if k in r:
                assert (r[k][rows] < 64).all() and (r[k][unlisted] == RR.FILL).all(), (name, k)
    for k, bad in RR.TILE_CASES.items():
        assert _read(_new_cases()["%d rows in chunks of %d" % k])["bad"] == len(bad)
    _, _, listed_bad, unlisted_bad = RR.list_case()
    assert _read(_new_cases()["a list of more than 64 rows"])["bad"] == len(listed_bad) == 2 and len(unlisted_bad) == 1


@pytest.mark.parametrize("wrong", WRONG)
def test_a_rule_that_is_right_on_the_old_cases_is_caught_by_the_case_built_for_it(wrong):
    """Each wrong rule changes no byte and no count on the calls the suite made before, and differs on the new case named for
    it.  'stride_A' is the exception the old cases already saw: it is the right rule only with ONE 'other' probe (q = 0), and
    is asserted to differ on the old calls with two and three; the new case takes the stride to q = 7 and to A = 128."""
    old, new = _old_cases(), _new_cases()
    for name, c in old.items():
        same = _equal(_read(c, wrong), _read(c))
        assert same == (wrong != "stride_A" or c["n"][0] == 1), (wrong, name)
    caught = {"bad_first_64": ("130 rows in chunks of 128", "70 rows in chunks of 70", "a list of more than 64 rows"),
              "prime_tile0": ("130 rows in chunks of 128", "70 rows in chunks of 70", "a list of more than 64 rows"),
              "probe_cap3": ("8+8 at A = 64", "8+8 at A = 128"), "stride_A": ("8+8 at A = 64", "8+8 at A = 128")}[wrong]
    for name in caught:
        right, bad = _read(new[name]), _read(new[name], wrong)
        assert not _equal(right, bad), (wrong, name)
        if wrong == "bad_first_64":
            assert bad["bad"] < right["bad"] and all(np.array_equal(right[k], bad[k]) for k in right if k != "bad")
        if wrong == "prime_tile0":
            rows = np.arange(new[name]["B"]) if new[name].get("rows") is None else new[name]["rows"]
            late = rows[np.arange(len(rows)) % new[name]["chunk_rows"] >= 32]
            assert (bad["ego_pred_prime"][late] == RR.FILL).all() and np.array_equal(bad["ego_pred"], right["ego_pred"])
        if wrong == "probe_cap3":
            for k in ("other_pred", "ego_pred", "ego_pred_prime"):
                assert np.array_equal(bad[k][:, :4], right[k][:, :4]) and all((bad[k][:, q] != right[k][:, q]).any() for q in range(4, 8))
        if wrong == "stride_A":
            A = new[name]["A"]
            assert np.array_equal(bad["other_pred"][:, 0], right["other_pred"][:, 0])
            assert all((bad["other_pred"][:, q] != right["other_pred"][:, q]).any() for q in range(1, 8))
            assert np.array_equal(bad["other_pred"][0, 7, 7:], right["other_pred"][0, 7, :A - 1 - 7]), "column j of probe 7 at 7 + j"
    # each bad label of the tile cases decides the count under some rule: without the slots from 64 on the count drops by the
    # labels that sit there, and those only
    for k, rows in RR.TILE_CASES.items():
        c = new["%d rows in chunks of %d" % k]
        in_first_64 = sum(1 for r in rows if r % k[1] < 64)
        assert _read(c, "bad_first_64")["bad"] == in_first_64 < len(rows)


# ---- the refusals of ProbeReadout that need no device

def _policy(A=64, R=1, num_layer=(3, 2)):
    pol = _stub_policy(A, R)
    pol.num_layer, pol.device = num_layer, torch.device("cpu")
    return pol


def _probe(pol, exp, model="late_lp", K=64):
    from gpudrive_lab_amd.lp_probe import DeviceLinearProbe
    p = object.__new__(DeviceLinearProbe)
    p.policy, p.exp, p.model, p.in_features = pol, exp, model, K
    return p


def test_probe_readout_refuses_before_any_device_call():
    from gpudrive_lab_amd.bc_readout import ProbeReadout
    pol = _policy()
    o, e = _probe(pol, "other"), _probe(pol, "ego")
    ok = ProbeReadout(pol, "ro_attn", 0, other=[o, o], ego=[e])
    assert ok.names == ("other_pred", "ego_pred") and ok.layer == 0 and ok.row_shape("other_pred") == (2, 63) and ok.row_nbytes() == 127
    assert ProbeReadout(pol, "ro_attn", None, ego=[e]).layer == 1 and ProbeReadout(pol, "fusion_attn", None, ego=[e]).layer == 2
    both = ProbeReadout(pol, "ro_attn", 0, other=[o], ego=[e], labels=10)
    assert both.names == ("other_pred", "ego_pred", "ego_pred_prime") and both.row_nbytes() == 65 and int(both.bad_labels) == 0
    with pytest.raises(ValueError, match="policy must be a DeviceBCPolicy"):
        ProbeReadout(object(), other=[o])
    with pytest.raises(ValueError, match="tap must be"):
        ProbeReadout(pol, "rg_attn", other=[o])
    for tap, layer in (("ro_attn", 2), ("ro_attn", -1), ("fusion_attn", 3), ("ro_attn", 0.0), ("ro_attn", True), ("ro_attn", "0")):
        with pytest.raises(ValueError, match="layer must be None or an int"):
            ProbeReadout(pol, tap, layer, other=[o])
    with pytest.raises(ValueError, match="at least one probe"):
        ProbeReadout(pol, "ro_attn", 0)
    with pytest.raises(ValueError, match="other holds 9 probes"):
        ProbeReadout(pol, "ro_attn", 0, other=[o] * 9)
    with pytest.raises(ValueError, match="ego holds 9 probes"):
        ProbeReadout(pol, "ro_attn", 0, ego=[e] * 9)
    ProbeReadout(pol, "ro_attn", 0, other=[o] * 8, ego=[e] * 8)
    with pytest.raises(ValueError, match=r"other\[1\] has exp 'ego'"):
        ProbeReadout(pol, "ro_attn", 0, other=[o, e])
    with pytest.raises(ValueError, match=r"ego\[0\] has exp 'other'"):
        ProbeReadout(pol, "ro_attn", 0, ego=[o])
    with pytest.raises(ValueError, match=r"other\[0\] must be a DeviceLinearProbe"):
        ProbeReadout(pol, "ro_attn", 0, other=["probe"])
    with pytest.raises(ValueError, match="must be a list"):
        ProbeReadout(pol, "ro_attn", 0, other=o)
    with pytest.raises(ValueError, match=r"ego\[0\] probes another policy object"):
        ProbeReadout(pol, "ro_attn", 0, ego=[_probe(_policy(), "ego")])
    with pytest.raises(ValueError, match=r"other\[0\] has in_features 12"):
        ProbeReadout(pol, "ro_attn", 0, other=[_probe(pol, "other", "baseline", 12)])
    with pytest.raises(ValueError, match=r"len\(other\) == len\(ego\)"):
        ProbeReadout(pol, "ro_attn", 0, other=[o, o], ego=[e], labels=3)
    with pytest.raises(ValueError, match=r"len\(other\) == len\(ego\)"):
        ProbeReadout(pol, "ro_attn", 0, ego=[e], labels=torch.zeros(4, dtype=torch.int64))
    for labels in (3.0, "3", torch.zeros(4, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int64), torch.zeros(8, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match="labels must be"):
            ProbeReadout(pol, "ro_attn", 0, other=[o], ego=[e], labels=labels)
    rows = ProbeReadout(pol, "ro_attn", 0, other=[o], ego=[e], labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels has 4 entries, the call 5 rows"):
        rows.bind((5,), None)


def test_hidden_and_run_refuse_before_any_device_call():
    from gpudrive_lab_amd.bc_policy import obs_width
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    pol = _policy()
    pol.obs_width = obs_width(64)
    obs = torch.zeros(2, 1, pol.obs_width)
    pm, rm = torch.zeros(2, 1, 63, dtype=torch.bool), torch.zeros(2, 1, 200, dtype=torch.bool)
    for layer in (2, -1, 1.5):
        with pytest.raises(ValueError, match="layer must be None or an int"):
            pol.hidden(obs, pm, rm, tap="ro_attn", layer=layer)
    with pytest.raises(ValueError, match="readout must be a ProbeReadout of this policy"):
        pol.read(obs, pm, rm, "readout")
    loop = object.__new__(ClosedLoopBC)
    loop.policy = pol
    with pytest.raises(ValueError, match="readout must be a bc_readout.ProbeReadout"):
        loop.run(readout="readout")
    from gpudrive_lab_amd.bc_readout import ProbeReadout
    other_pol = _policy()
    with pytest.raises(ValueError, match="readout reads another policy object"):
        loop.run(readout=ProbeReadout(other_pol, "ro_attn", 0, ego=[_probe(other_pol, "ego")]))


def test_nbytes_counts_the_new_arrays():
    from gpudrive_lab_amd.bc_readout import ProbeReadout
    from gpudrive_lab_amd.bc_rollout import ClosedLoopBC
    pol = _policy(128, 5)
    ro = ProbeReadout(pol, "ro_attn", 0, other=[_probe(pol, "other")] * 2, ego=[_probe(pol, "ego")] * 2, labels=1)
    base = ClosedLoopBC.row_nbytes(128, 5)
    assert ClosedLoopBC.row_nbytes(128, 5, attention=True) - base == 91 * (4 * 127 * 4 + 1)
    assert ClosedLoopBC.row_nbytes(128, 5, record=True, attention=True) - ClosedLoopBC.row_nbytes(128, 5, record=True) == 91 * 4 * 127 * 4
    assert ClosedLoopBC.row_nbytes(128, 5, readout=ro) - base == 91 * (2 * 127 + 2 + 2)
    assert 832 * 91 * 4 * 127 * 4 == 153_846_784  # the docstring's 154 MB at N = 832


# ---- the C calls: every refusal comes before the first launch, so no pointer below is ever read (none points anywhere)

def _readout(**kw):
    r = _capi.GdBCReadout()
    r.tap, r.layer, r.n_other, r.n_ego, r.intervene = _capi.LP_TAP_RO, 0, 1, 1, 1
    r.other[0].packed, r.other[0].weight, r.ego[0].packed = OK16, OK4, OK16
    r.labels, r.other_pred, r.ego_pred, r.ego_pred_prime, r.bad_labels = OK16, OK4 + 1, OK4 + 2, OK4 + 3, OK4
    r.other_stride, r.ego_stride, r.prime_stride = 63, 1, 1
    for k, v in kw.items():
        setattr(r, k, v)
    return r


READOUT_REFUSALS = ((dict(tap=2), "tap must be"), (dict(layer=1), "layer must be in"), (dict(layer=-1), "layer must be in"),
                    (dict(n_other=9), r"must be in \[0, 8\]"), (dict(n_ego=-1), r"must be in \[0, 8\]"),
                    (dict(n_other=0, n_ego=0, intervene=0), "at least one probe"), (dict(reserved=1), "reserved must be 0"),
                    (dict(intervene=2), "intervene must be 0 or 1"), (dict(n_other=0), "intervene needs n_other == n_ego"),
                    (dict(other_pred=None), "output of a non-zero count is null"), (dict(ego_pred=None), "output of a non-zero count"),
                    (dict(ego_pred_prime=None), "output of a non-zero count"), (dict(other_stride=62), "stride is below"),
                    (dict(ego_stride=0), "stride is below"), (dict(labels=OK16 + 4), "labels must be 8-byte aligned"),
                    (dict(bad_labels=None), "bad_labels is required"), (dict(bad_labels=ODD), "bad_labels is required"))


def test_the_forwards_refuse_a_bad_readout():
    L = _capi.lib()
    p, o = _policy_struct(), _capi.GdBCOutputs(actions=OK4)
    head = (OK4, OK4 + 1, OK4 + 3, 11, 1, None, None, None, ctypes.byref(o))

    def fwd(r, pp=p):
        return L.gd_bc_forward_readout(ctypes.byref(pp), *head, ctypes.byref(r) if r is not None else None, None)

    def rows(r, rows_=OK4, count=OK4):
        return L.gd_bc_forward_rows_readout(ctypes.byref(p), *head, ctypes.byref(r) if r is not None else None, rows_, count, None)

    for call, who in ((fwd, "gd_bc_forward_readout"), (rows, "gd_bc_forward_rows_readout")):
        _refused(call(None), who + ": readout is required")
        for kw, match in READOUT_REFUSALS:
            _refused(call(_readout(**kw)), who + ": readout: .*" + match)
        bad = _readout()
        bad.other[0].packed = OK16 + 4
        _refused(call(bad), who + ": readout: a probe's packed is required, 16-byte aligned")
        bad = _readout()
        bad.ego[0].packed = None
        _refused(call(bad), who + ": readout: a probe's packed is required")
        bad = _readout()
        bad.other[0].weight = None
        _refused(call(bad), who + ": readout: an 'other' probe's weight is required with intervene")
    detached = _policy_struct()
    detached.scratch = None
    _refused(fwd(_readout(), detached), "gd_bc_forward_readout: blob and scratch are required")
    _refused(rows(_readout(), rows_=None), "gd_bc_forward_rows_readout: rows and count are required")
    # gd_bc_hidden_layer: the layer's range per block (the stub policy has one layer in each)
    hid = lambda tap, layer, out=OK16: L.gd_bc_hidden_layer(ctypes.byref(p), OK4, OK4 + 1, OK4 + 3, 11, tap, layer, out, None)  # noqa: E731
    for tap in (0, 1):
        for layer in (1, -1):
            _refused(hid(tap, layer), "gd_bc_hidden_layer: layer must be in")
    _refused(hid(2, 0), "gd_bc_hidden_layer: tap must be")
    _refused(hid(0, 0, None), "gd_bc_hidden_layer: out is required")


def test_gd_bc_rollout_readout_refuses_before_the_simulator_is_read():
    L = _capi.lib()
    sim = ctypes.create_string_buffer(4096)
    p, b = _policy_struct(), _buffers()
    good_rows = _capi.GdBCRolloutRows(rows=OK4, count=OK4, scratch=OK4)

    def call(sim=sim, pp=ctypes.byref(p), bb=ctypes.byref(b), rr=None, xx=True, n_steps=91, score=OK4, readout=None):
        x = _capi.GdBCRolloutReads()
        x.ego_attn_score = score
        if readout is not None:
            x.readout = ctypes.pointer(readout)
        return L.gd_bc_rollout_readout(sim, pp, bb, ctypes.byref(rr) if rr is not None else None, ctypes.byref(x) if xx else None, n_steps)

    who = "gd_bc_rollout_readout: "
    for kw in (dict(sim=None), dict(pp=None), dict(bb=None), dict(xx=False)):
        _refused(call(**kw), who + "null argument")
    _refused(call(score=None), who + "reads needs ego_attn_score or readout")
    _refused(call(score=ODD), who + "ego_attn_score must be 4-byte aligned")
    _refused(call(rr=_capi.GdBCRolloutRows(rows=OK4, count=OK4)), who + "scratch is required")
    _refused(call(rr=_capi.GdBCRolloutRows(rows=None, count=OK4, scratch=OK4)), who + "rows and count are required")
    for rr in (None, good_rows):
        _refused(call(rr=rr, n_steps=92), who + r"an episode has 91 steps")
        _refused(call(rr=rr, bb=ctypes.byref(_buffers(dead=None))), who + "every buffer but the per-step records is required")
    assert sim.raw == bytes(4096)
