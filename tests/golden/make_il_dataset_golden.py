#!/usr/bin/env python3
"""Generates tests/golden/il_dataset_golden.npz: what THE REFERENCE'S OWN ExpertDataset
(gpudrive/integrations/il/dataloader.py) makes of the kept rows of tests/il_cases.py at 128 agent slots -- the arrays a file
written by ExpertEpisode.save() would hand it.  tests/test_il_dataset.py requires the numpy rule of tests/il_cases.py, the
yardstick of the device expert dataset, to give the same.

Per window (rollout_len, pred_len) of il_cases.WINDOWS: the full valid_indices, and for about eight sample positions (the
first and the last, windows that cross t = 0, ones next to the dead stretches) the whole actions, both masks and data_idx
and obs at COLS.  Authoring only; needs a checkout of the reference:

    python tests/golden/make_il_dataset_golden.py <path to the reference checkout>

dataloader.py is loaded by file path between stub `gpudrive` / `gpudrive.env` packages around its constants.py: importing
the package proper needs the compiled simulator."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import il_cases  # noqa: E402

A = 128
D = il_cases.width(A)
# ego, both sides of the ego / partner boundary, both sides of several 16-byte (4-column) boundaries, the partner / road
# boundary (6 + 127 * 6 = 768), the row's end
COLS = np.array([0, 3, 4, 5, 6, 7, 8, 11, 12, 255, 256, 767, 768, 769, 1023, 1024, 2047, 2048, 3000, D - 8, D - 5, D - 4, D - 2,
                 D - 1])


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
    return from_path("reference_il_dataloader", os.path.join(ref, "gpudrive", "integrations", "il", "dataloader.py"))


def positions(vi, R):
    """About eight positions into valid_indices: the ends, windows crossing t = 0, neighbours of the dead stretches."""
    M = len(vi)
    want = {0, M - 1, M // 2}
    crossing = np.nonzero(vi[:, 1] < R - 1)[0]
    want.update(crossing[:2].tolist())
    # idx1 counts the kept rows: 1 is dead from t = 40 (its last sample), 3 is dead for its first 7 steps (its first sample
    # and the first whose window is clear of them), 4 has invalid steps around t = 64 (the last sample up to there)
    for row, pick in ((1, lambda h: h[-1]), (3, lambda h: h[0]), (3, lambda h: h[min(R, len(h) - 1)]),
                      (4, lambda h: h[vi[h, 1] <= 64][-1])):
        hit = np.nonzero(vi[:, 0] == row)[0]
        if len(hit):
            want.add(int(pick(hit)))
    return np.array(sorted(want))[:9]


def main():
    ref = load_reference(sys.argv[1])
    case = il_cases.make_case(A)
    keep = case["keep"]
    saved = dict(obs=case["obs"][keep], actions=case["actions"][keep], dead_mask=case["dead_mask"][keep],
                 partner_mask=case["partner_mask"][keep].astype(np.int64), road_mask=case["road_mask"][keep])  # save()'s dtypes
    out = dict(cols=COLS, windows=np.array(il_cases.WINDOWS))
    for R, P in il_cases.WINDOWS:
        ds = ref.ExpertDataset(saved["obs"], saved["actions"], saved["dead_mask"], saved["partner_mask"], saved["road_mask"],
                               rollout_len=R, pred_len=P)
        vi = np.array(ds.valid_indices, np.int64).reshape(-1, 2)
        pos = positions(vi, R)
        items = [ds[int(p)] for p in pos]
        key = "r%d_p%d_" % (R, P)
        out[key + "valid_indices"] = vi.astype(np.int16)  # (rows < 7, times < 91)
        out[key + "pos"] = pos
        out[key + "obs"] = np.stack([it[0][:, COLS] for it in items]).astype(np.float32).view(np.int32)
        out[key + "actions"] = np.stack([it[1] for it in items]).astype(np.float32).view(np.int32)
        out[key + "partner_mask"] = np.packbits(np.stack([it[2] for it in items]), axis=-1)
        out[key + "road_mask"] = np.packbits(np.stack([it[3] for it in items]), axis=-1)
        out[key + "data_idx"] = np.stack([it[4].numpy() for it in items]).astype(np.int64)
        assert out[key + "obs"].shape == (len(pos), R, len(COLS)) and out[key + "actions"].shape == (len(pos), P, 3)
        print("window", (R, P), "samples", len(vi), "positions", pos.tolist())
    path = os.path.join(ROOT, "tests", "golden", "il_dataset_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
