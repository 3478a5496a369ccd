"""Shared inputs and the yardstick of the linear-probing dataset's tests (tests/test_lp_dataset.py,
tests/test_gpu_lp_dataset.py, tests/golden/make_lp_dataset_golden.py).

The inputs are tests/il_cases.make_case's seven rows with three changes, all from integer arithmetic and IEEE add / multiply /
divide alone (no random stream, no transcendental): ego poses are added, partner columns 1 and 2 of obs (the relative
position, normalised by 1000 m) are overwritten with values inside +-0.08 (as made they are large integers and every label
would clip to 7), and partner_mask becomes one that leaves a partner unmasked at both ends of a future step often enough.

The rule is the reference's FutureDataset restated in vectorised numpy from its description (not transcribed).  T = 91,
F = future_step, valid = il_cases.valid_steps, (n, t) a source row and a current time, everything in fp32 in this order, cos
and sin evaluated in double and rounded to fp32:
  cls(v, b) = clip(#{i: b[i] <= double(v)} - 1, 0, 7), 7 for a NaN;  label(x, y) = cls(x, xb) * 8 + cls(y, yb);
  norm(v) = 2 * ((v - (-1000)) / 2000) - 1;  xb, yb = numpy.linspace(lo, hi, 9), (-0.05, 0.05) by default;
  ego:   future_valid_mask = valid[n, t] & (t + F < T) & valid[n, t + F]; where t + F >= T the label is label(0, 0); else
         d = pos[t + F] - pos[t], c, s = cos, sin(rot[t]): label(norm(d.x * c + d.y * s), norm((-d.x) * s + d.y * c));
  other: per partner column j, aux_mask = (pm[n, t, j] != 0) | (t + F >= T) | (pm[n, t + F, j] != 0); where it is true the
         label is label(0, 0); else p = obs[n, t + F, 6 + 6j + 1 .. + 3) * 1000, e = pos[t + F], c, s = cos, sin(rot[t + F]),
         g = ((e.x + p.x * c) - p.y * s, (e.y + p.x * s) + p.y * c), d = g - pos[t], c2, s2 = cos, sin(-rot[t]):
         label(norm(d.x * c2 + d.y * s2), norm((-d.x) * s2 + d.y * c2)).
A sample (n, idx2) of il_cases.index takes these at t = idx2, valid_mask = valid[n, idx2 + P - 1] and ego_mask[r] =
valid[n, idx2 - R + 1 + r] (False where the time is negative); obs, actions, partner_mask and road_mask are il_cases.batch's.
tests/golden/lp_dataset_golden.npz pins this rule to the reference's own class."""

import numpy as np

from tests import il_cases

T = il_cases.T
FUTURE_STEPS = (1, 35, 90)
EGO_RANGE = ((-0.025, 0.05), (-0.025, 0.025))  # an xy_range for exp='ego' (the one linear_probing's notes give for F = 35)
# rows (il_cases': 0 the thresholds, 1 dropped, 2 dead from t = 40, 3 dead throughout, 4 dead for its first 7 steps, 5 invalid
# actions, 6 plain): 0 a slow turn with one NaN position, 1 and 5 turns at other speeds, 5's heading from beyond -pi,
# 2 a fast turn whose heading passes pi, 4 stationary, 6 the edge row
NAN_ROW, NAN_TIME = 0, 45
PI_ROW, STATIONARY_ROW, EDGE_ROW = 2, 4, 6
SWITCH_TIME, OFF_THEN_ON, ON_THEN_OFF = 50, 3, 4  # partner columns of the edge row whose mask switches between 0 and 2


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def make_case(A, n_rows=il_cases.N_ROWS):
    assert n_rows == il_cases.N_ROWS
    case = il_cases.make_case(A, n_rows)
    PM = A - 1
    t = np.arange(T, dtype=np.float64)
    pos = np.zeros((n_rows, T, 2))
    rot = np.zeros((n_rows, T))
    # turns: a parabola-like path at a speed and a curvature per row, a heading that drifts linearly
    for n, (v, k, r0, w) in {0: (0.3, 0.05, 0.25, 0.01), 1: (0.9, -0.2, -1.0, -0.015), 2: (1.6, 0.35, 3.0, 0.004),
                             3: (0.5, 0.1, 0.5, 0.0), 5: (1.1, -0.3, -3.1, -0.002)}.items():
        pos[n, :, 0] = 100.0 * n + v * t * (1.0 - t / 400.0)
        pos[n, :, 1] = -50.0 * n + k * t * t / 100.0
        rot[n] = r0 + w * t
    pos[STATIONARY_ROW] = (321.5, -87.25)
    rot[STATIONARY_ROW] = 0.7 + 0.01 * t
    pos, rot = _f32(pos), _f32(rot)
    pos[NAN_ROW, NAN_TIME, 0] = np.nan
    # the edge row: rot = 0, even times at the origin, odd times at k * 12.5 m (a bin edge after norm) or one of its two
    # fp32 neighbours, so that every odd F sees +- those displacements exactly
    h = np.arange(T) // 2
    for axis, (k, variant) in enumerate((((h % 9) - 4, (h // 9) % 3), (((2 * h + 3) % 9) - 4, (h // 3) % 3))):
        e = (k * 12.5).astype(np.float32)
        e = np.where(variant == 1, np.nextafter(e, np.float32(-np.inf)), np.where(variant == 2, np.nextafter(e, np.float32(np.inf)), e))
        pos[EDGE_ROW, :, axis] = np.where(np.arange(T) % 2 == 1, e, np.float32(0))
    assert abs(rot[PI_ROW, 0]) < np.pi < abs(rot[PI_ROW, -1]) and rot[5, 0] < -3.0 and rot[5, -1] < -np.pi

    n, tt, j = np.arange(n_rows)[:, None, None], np.arange(T)[None, :, None], np.arange(PM)[None, None, :]
    px = ((n * 37 + j * 53) % 121 - 60 + (tt * (j % 5 - 2)) / 10.0) / 1000.0
    py = ((n * 29 + j * 71 + 13) % 121 - 60 + (tt * ((j + n) % 7 - 3)) / 15.0) / 1000.0
    assert np.abs(px).max() < 0.08 and np.abs(py).max() < 0.08
    case["obs"][:, :, 6 + 1:6 + 6 * PM:6] = _f32(px)
    case["obs"][:, :, 6 + 2:6 + 6 * PM:6] = _f32(py)
    pm = np.array([0, 0, 0, 1, 2], np.uint8)[(n * 5 + j * 7 + (j * j) // 3 + tt // 23) % 5]
    pm[EDGE_ROW, :, OFF_THEN_ON] = np.where(np.arange(T) < SWITCH_TIME, 0, 2)
    pm[EDGE_ROW, :, ON_THEN_OFF] = np.where(np.arange(T) < SWITCH_TIME, 2, 0)
    case["partner_mask"] = np.ascontiguousarray(pm)
    case["ego_global_pos"], case["ego_global_rot"] = pos, rot[:, :, None].copy()
    return case


split = il_cases.split


def bins(xy_range=None):
    (xlo, xhi), (ylo, yhi) = xy_range if xy_range is not None else ((-0.05, 0.05), (-0.05, 0.05))
    return np.linspace(xlo, xhi, 9), np.linspace(ylo, yhi, 9)


def cls(v, b):
    v = np.asarray(v)
    n = (b <= v[..., None].astype(np.float64)).sum(-1)
    return np.clip(np.where(np.isnan(v), 9, n) - 1, 0, 7)


def label(x, y, xy_range=None):
    xb, yb = bins(xy_range)
    return (cls(x, xb) * 8 + cls(y, yb)).astype(np.int64)


def future(case, F, exp, dtype=np.float32):
    """(mask, x, y) for every (n, t): the future mask and the pair the label is the class of, [N, T] for 'ego' and
    [N, T, A - 1] for 'other'.  dtype float32 is the rule; float64 the same formulas without fp32 rounding."""
    assert 1 <= F <= T - 1 and exp in ("ego", "other")
    f = dtype
    pos, rot = case["ego_global_pos"].astype(f), case["ego_global_rot"][..., 0].astype(f)
    N = pos.shape[0]
    t = np.arange(T)
    ahead = (t + F < T)[None, :]
    tf = np.minimum(t + F, T - 1)

    def cos_sin(a):
        a = a.astype(np.float64)
        return np.cos(a).astype(f), np.sin(a).astype(f)

    def norm(v):
        return f(2) * ((v - f(-1000)) / f(2000)) - f(1)

    with np.errstate(invalid="ignore"):
        if exp == "ego":
            valid = il_cases.valid_steps(case)
            mask = valid & ahead & valid[:, tf]
            dx, dy = pos[:, tf, 0] - pos[:, :, 0], pos[:, tf, 1] - pos[:, :, 1]
            c, s = cos_sin(rot)
            rx, ry = dx * c + dy * s, (-dx) * s + dy * c
            zero = np.broadcast_to(~ahead, (N, T))
        else:
            PM = case["partner_mask"].shape[2]
            pm = case["partner_mask"] != 0
            mask = pm | ~ahead[..., None] | pm[:, tf]
            px = case["obs"][:, tf, 6 + 1:6 + 6 * PM:6].astype(f) * f(1000)
            py = case["obs"][:, tf, 6 + 2:6 + 6 * PM:6].astype(f) * f(1000)
            c, s = (a[..., None] for a in cos_sin(rot[:, tf]))
            fut = pos[:, tf]
            gx, gy = (fut[..., 0, None] + px * c) - py * s, (fut[..., 1, None] + px * s) + py * c
            dx, dy = gx - pos[..., 0, None], gy - pos[..., 1, None]
            c2, s2 = (a[..., None] for a in cos_sin(-rot))
            rx, ry = dx * c2 + dy * s2, (-dx) * s2 + dy * c2
            zero = mask
        x, y = np.where(zero, f(0), norm(rx)), np.where(zero, f(0), norm(ry))
    return mask, x, y


def labels(case, F, exp, xy_range=None):
    """(mask, label int64) for every (n, t)."""
    mask, x, y = future(case, F, exp)
    return mask, label(x, y, xy_range)


def near_edge(case, F, exp, xy_range=None, tol=1e-6):
    """Where the pair recomputed in float64 lies within tol of a bin edge: the only places where a label may differ from
    the rule's (one fp32 rounding there moves the value across the edge)."""
    _, x, y = future(case, F, exp, np.float64)
    xb, yb = bins(xy_range)
    with np.errstate(invalid="ignore"):
        return (np.abs(x[..., None] - xb).min(-1) < tol) | (np.abs(y[..., None] - yb).min(-1) < tol)


def batch(case, R, P, F, exp, sel, xy_range=None, cols=None, _all=None):
    """The eight arrays of the batch at index positions `sel` (obs and actions as int32 bit patterns, obs at columns `cols`
    only if given)."""
    obs, actions, partner, road, _ = il_cases.batch(case, R, P, sel, cols)
    vi, rows = il_cases.index(case, R, P)
    sel = np.asarray(sel, np.int64)
    ok = (sel >= 0) & (sel < len(vi))
    pos = np.where(ok, sel, 0)
    if len(vi) == 0:
        vi, rows = np.zeros((1, 2), np.int64), np.zeros(1, np.int64)
    n, idx2 = rows[pos], vi[pos, 1]
    valid = il_cases.valid_steps(case)
    valid_mask = ok & valid[n, idx2 + P - 1]
    times = idx2[:, None] - R + 1 + np.arange(R)[None, :]
    ego_mask = ok[:, None] & (times >= 0) & valid[n[:, None], np.clip(times, 0, T - 1)]
    mask, lab = _all if _all is not None else labels(case, F, exp, xy_range)
    mask, lab = mask[n, idx2].copy(), lab[n, idx2].copy()
    mask[~ok] = exp == "other"
    lab[~ok] = label(np.float32(0), np.float32(0), xy_range)
    return obs, actions, valid_mask, ego_mask, partner, road, mask, lab
