#!/usr/bin/env python3
"""Generates tests/golden/lp_dataset_golden.npz: what THE REFERENCE'S OWN FutureDataset
(gpudrive/integrations/il/linear_probing/dataloader.py) makes of the kept rows of tests/lp_cases.py at 128 agent slots -- the
arrays the two files written by ExpertEpisode.save() would hand it.  tests/test_lp_dataset.py requires the numpy rule of
tests/lp_cases.py, the yardstick of the device linear-probing dataset, to give the same.

Held, per kept row and time ([6, 91, ...]; the window does not enter them):
  exp='other', F in lp_cases.FUTURE_STEPS: other_pos as uint8 and aux_mask bit-packed;
  exp='ego', F in (1, 5, 35, 90): ego_pos as uint8 and future_valid_mask, and once more at F = 35 with lp_cases.EGO_RANGE;
and for about eight sample positions of (rollout_len, pred_len) = (5, 1), F = 35, both experiments, the whole 8-tuple of
__getitem__ with obs at COLS, to pin order, shapes and dtypes.  Authoring only; needs a checkout of the reference:

    python tests/golden/make_lp_dataset_golden.py <path to the reference checkout>

dataloader.py is loaded by file path between stub `gpudrive` / `gpudrive.env` packages around its constants.py, as
make_il_dataset_golden.py does."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import il_cases, lp_cases  # noqa: E402

A = 128
D = il_cases.width(A)
# il_dataset_golden's subset: the ego block, partner 0's columns 1 and 2 among them, 16-byte boundaries, the row's end
COLS = np.array([0, 3, 4, 5, 6, 7, 8, 11, 12, 255, 256, 767, 768, 769, 1023, 1024, 2047, 2048, 3000, D - 8, D - 5, D - 4, D - 2,
                 D - 1])
EGO_STEPS = (1, 5, 35, 90)
R, P, F_ITEMS = 5, 1, 35


def load_reference(ref):
    def from_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    for name in ("gpudrive", "gpudrive.env"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    from_path("gpudrive.env.constants", os.path.join(ref, "gpudrive", "env", "constants.py"))
    return from_path("reference_lp_dataloader",
                     os.path.join(ref, "gpudrive", "integrations", "il", "linear_probing", "dataloader.py"))


def positions(vi):
    """About eight positions into valid_indices: the ends, a window crossing t = 0, idx2 + F on both sides of 91, the
    neighbours of the dead stretches and of the switch of the edge row's partner columns."""
    M = len(vi)
    want = {0, M - 1, M // 2}
    want.update(np.nonzero(vi[:, 1] < R - 1)[0][:1].tolist())
    for row, idx2 in ((0, 90 - F_ITEMS), (0, 91 - F_ITEMS), (1, 39 - F_ITEMS), (3, 7), (5, lp_cases.SWITCH_TIME - 1),
                      (5, lp_cases.SWITCH_TIME - F_ITEMS)):  # (idx1 counts the kept rows)
        hit = np.nonzero((vi[:, 0] == row) & (vi[:, 1] == idx2))[0]
        want.update(hit.tolist())
    return np.array(sorted(want))


def main():
    ref = load_reference(sys.argv[1])
    case = lp_cases.make_case(A)
    keep = case["keep"]
    saved = {k: v[keep] for k, v in case.items() if k != "keep"}
    saved["partner_mask"] = saved["partner_mask"].astype(np.int64)  # save()'s dtype

    def dataset(**kw):
        return ref.FutureDataset(saved["obs"], saved["actions"], saved["ego_global_pos"], saved["ego_global_rot"],
                                 saved["dead_mask"], saved["partner_mask"], saved["road_mask"], **kw)

    out = dict(cols=COLS, future_steps=np.array(lp_cases.FUTURE_STEPS), ego_steps=np.array(EGO_STEPS),
               ego_range=np.array(lp_cases.EGO_RANGE), window=np.array([R, P, F_ITEMS]))
    for F in lp_cases.FUTURE_STEPS:
        ds = dataset(future_step=F, exp="other")
        assert ds.other_pos.shape == (keep.sum(), il_cases.T, A - 1) and 0 <= ds.other_pos.min() and ds.other_pos.max() < 64
        out["other_f%d_pos" % F] = ds.other_pos.astype(np.uint8)
        out["other_f%d_mask" % F] = np.packbits(ds.aux_mask, axis=-1)
    for F in EGO_STEPS:
        ds = dataset(future_step=F, exp="ego")
        out["ego_f%d_pos" % F] = ds.ego_pos.astype(np.uint8)
        out["ego_f%d_mask" % F] = ds.future_valid_mask.astype(bool)
    ds = dataset(future_step=F_ITEMS, exp="ego", xy_range=lp_cases.EGO_RANGE)
    out["ego_range_pos"] = ds.ego_pos.astype(np.uint8)
    out["ego_range_mask"] = ds.future_valid_mask.astype(bool)
    for exp in ("other", "ego"):
        ds = dataset(rollout_len=R, pred_len=P, future_step=F_ITEMS, exp=exp)
        vi = np.array(ds.valid_indices, np.int64).reshape(-1, 2)
        pos = positions(vi)
        items = [ds[int(p)] for p in pos]
        assert all(len(it) == 8 for it in items)
        key = "items_%s_" % exp
        out[key + "pos"] = pos
        out[key + "obs"] = np.stack([it[0][:, COLS] for it in items]).astype(np.float32).view(np.int32)
        out[key + "actions"] = np.stack([it[1] for it in items]).astype(np.float32).view(np.int32)
        out[key + "valid_mask"] = np.stack([it[2] for it in items]).astype(bool)
        out[key + "ego_mask"] = np.stack([it[3] for it in items]).astype(bool)
        out[key + "partner_mask"] = np.packbits(np.stack([it[4] for it in items]), axis=-1)
        out[key + "road_mask"] = np.packbits(np.stack([it[5] for it in items]), axis=-1)
        out[key + "future_mask"] = np.stack([it[6] for it in items]).astype(bool)
        out[key + "future_pos"] = np.stack([it[7] for it in items]).astype(np.uint8)
        # what a consumer sees of each element: its shape and dtype kind as the reference hands them over
        out[key + "shapes"] = np.array([str([tuple(np.shape(x)) for x in items[0]])])
        out[key + "kinds"] = np.array(["".join(np.asarray(x).dtype.kind for x in items[0])])
        print(exp, "samples", len(vi), "positions", pos.tolist(), out[key + "shapes"][0], out[key + "kinds"][0])
    path = os.path.join(ROOT, "tests", "golden", "lp_dataset_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
