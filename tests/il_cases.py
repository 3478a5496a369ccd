"""Shared inputs and the yardstick of the device expert dataset's tests (tests/test_il_dataset.py,
tests/test_gpu_il_dataset.py, tests/golden/make_il_dataset_golden.py).

The inputs come from integer arithmetic alone (no random stream), so that every element of a gathered batch names its
source: obs[n, t, j] = float32((n * 91 + t) * 4096 + j), exact below 2^24.

The rule is the windowed mode of the reference's ExpertDataset restated in vectorised numpy from its description (not
transcribed): with R = rollout_len, P = pred_len, T = 91,
  valid[n, t] = !dead_mask[n, t] && !(|a1| > 0.5f || |a0| > 5.f || |a2| > 0.2f), strict, in fp32 (a NaN stays valid);
  the samples are the (n, idx2), idx2 in [0, T - P], of kept rows with valid[n, idx2 + P - 1], in row-major order;
  idx1 is the ordinal of row n among the kept rows;
  a sample is obs and both masks at times idx2 - R + 1 .. idx2 (zeros / True where the time is negative; partner_mask is
  `stored == 2`), the actions at times idx2 .. idx2 + P - 1, and (idx1, idx2).
tests/golden/il_dataset_golden.npz pins this rule to the reference's own class."""
import numpy as np

T = 91
ROADS = 200
N_ROWS = 7
WINDOWS = [(5, 1), (10, 5), (1, 1), (90, 1), (1, 90), (3, 2)]  # (rollout_len, pred_len)
# rows: 0 the thresholds, 1 dropped (keep = False), 2 dead from t = 40, 3 dead throughout, 4 dead for its first 7 steps,
# 5 invalid actions around the two ballot passes' boundary and at both ends, 6 plain
DROPPED_ROW, DEAD_FROM_40, DEAD_ALWAYS, DEAD_FIRST_7 = 1, 2, 3, 4


def width(A):
    return 6 + (A - 1) * 6 + ROADS * 13


def _above(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def make_case(A, n_rows=N_ROWS):
    """The recorder's arrays for n_rows rows (numpy; dtypes as ExpertEpisode holds them) plus keep."""
    D = width(A)
    nt = (np.arange(n_rows)[:, None] * T + np.arange(T)[None, :]).astype(np.int64)  # [N, T]
    obs = (nt[:, :, None] * 4096 + np.arange(D)[None, None, :]).astype(np.float32)
    n, t = np.arange(n_rows)[:, None], np.arange(T)[None, :]
    actions = np.empty((n_rows, T, 3), np.float32)  # all inside the thresholds ...
    actions[..., 0] = ((n * 7 + t * 3) % 11 - 5) * np.float32(0.5)
    actions[..., 1] = ((n + t) % 5 - 2) * np.float32(0.125)
    actions[..., 2] = ((n * 3 + t) % 7 - 3) * np.float32(0.03125)
    # ... but where a threshold is hit exactly (valid), passed by one ulp (invalid) or a NaN stands (valid)
    r = actions[0]
    r[10, 0], r[11, 0], r[12, 0], r[13, 0] = 5.0, _above(5.0), -5.0, -_above(5.0)
    r[20, 1], r[21, 1], r[22, 1], r[23, 1] = 0.5, _above(0.5), -0.5, -_above(0.5)
    r[30, 2], r[31, 2], r[32, 2], r[33, 2] = np.float32(0.2), _above(0.2), -np.float32(0.2), -_above(0.2)
    r[50, 0], r[51, 1], r[52, 2] = np.nan, np.nan, np.nan
    if n_rows > 5:
        r = actions[5]
        r[0, 0], r[63, 1], r[64, 2], r[66, 0], r[89, 1], r[90, 2] = 6.0, 1.0, -0.25, -7.0, -0.75, 0.5
    dead = np.zeros((n_rows, T), bool)
    if n_rows > DEAD_FIRST_7:
        dead[DEAD_FROM_40, 40:] = True
        dead[DEAD_ALWAYS] = True
        dead[DEAD_FIRST_7, :7] = True
    k = np.arange(A - 1)[None, None, :]
    partner = ((nt[:, :, None] * 7 + k * 5 + (k * k) // 3) % 3).astype(np.uint8)
    k = np.arange(ROADS)[None, None, :]
    road = (nt[:, :, None] * 3 + k + k // 7) % 4 == 0
    keep = np.ones(n_rows, bool)
    if n_rows > DROPPED_ROW:
        keep[DROPPED_ROW] = False
    return dict(obs=obs, actions=actions, dead_mask=dead, partner_mask=partner, road_mask=road, keep=keep)


def split(case, sizes):
    """The case cut into consecutive shards of the given row counts."""
    out, lo = [], 0
    for n in sizes:
        out.append({k: v[lo:lo + n] for k, v in case.items()})
        lo += n
    assert lo == case["keep"].shape[0]
    return out


def valid_steps(case):
    a = np.abs(case["actions"].astype(np.float32))
    bad = (a[..., 1] > np.float32(0.5)) | (a[..., 0] > np.float32(5.0)) | (a[..., 2] > np.float32(0.2))
    return ~case["dead_mask"] & ~bad


def index(case, R, P):
    """(valid_indices [M, 2] int64 of (idx1, idx2), rows [M]: the source row n of every sample)."""
    assert R >= 1 and P >= 1 and R + P <= T
    v = valid_steps(case)[:, P - 1:] & case["keep"][:, None]  # column idx2 tests time idx2 + P - 1
    rows, idx2 = np.nonzero(v)
    ordinal = np.cumsum(case["keep"]) - 1
    return np.stack([ordinal[rows], idx2], 1).astype(np.int64), rows


def batch(case, R, P, sel, cols=None):
    """The five arrays of the batch at index positions `sel` (obs as int32 bit patterns; obs at columns `cols` only, if
    given).  A position outside the index gives the all-padding sample."""
    vi, rows = index(case, R, P)
    sel = np.asarray(sel, np.int64)
    ok = (sel >= 0) & (sel < len(vi))
    pos = np.where(ok, sel, 0)
    if len(vi) == 0:
        vi, rows = np.zeros((1, 2), np.int64), np.zeros(1, np.int64)
    n, idx2 = rows[pos], vi[pos, 1]
    times = idx2[:, None] - R + 1 + np.arange(R)[None, :]
    pad = (times < 0) | ~ok[:, None]
    tc = np.clip(times, 0, T - 1)
    obs = case["obs"] if cols is None else case["obs"][:, :, cols]
    obs = obs[n[:, None], tc].view(np.int32).copy()
    obs[pad] = 0
    ta = np.clip(idx2[:, None] + np.arange(P)[None, :], 0, T - 1)
    actions = case["actions"][n[:, None], ta].view(np.int32).copy()
    actions[~ok] = 0
    partner = case["partner_mask"][n[:, None], tc] == 2
    partner[pad] = True
    road = case["road_mask"][n[:, None], tc].copy()
    road[pad] = True
    data_idx = np.where(ok[:, None], vi[pos], -1).astype(np.int64)
    return obs, actions, partner, road, data_idx
