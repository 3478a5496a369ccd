"""Float64 statement of the partner rows (partner_observations_tensor) and of the packed head made from them,
written from the definition, numpy only.

It reads the tensors every simulator exports -- the absolute self rows (position, rotation, size, id), the self rows (speed and,
for the packed head, the ego columns), info_tensor[..., 4] (the entity type), shape_tensor -- plus observationRadius, and states
the A - 1 rows of every live agent of one world.  The float32 inputs are taken as exact, so the same function checks the oracle
on the CPU and the kernels on the GPU.  No oracle, no engine internals.

  collectPartnerObsSystem (reference src/sim.cpp:188-240; OtherAgents order src/level_gen.cpp:450-464): slot k of ego i is agent
    j = k < i ? k : k + 1; position = R(-yaw_i) (p_j - p_i) with plain cos / sin, heading = wrap(yaw_j - yaw_i), speed = j's
    self-row speed (the length of its 3-vector velocity), size, type and id j's; length() > radius gives
    PartnerObservation::zero() (all zero, id -1); slots >= n - 1 give zero_nonexist() (all zero, id -2).  Headings are compared
    modulo 2 pi: for an exactly opposite partner the sign of pi belongs to the quaternion product, the exported rotations cannot
    tell +pi from -pi, so no sign is pinned here (as tests/road_reference.py pins none).
  the packed head (gpudrive env_torch.py get_obs with norm_obs; tests/parity.py pack_observation_f64 restates it): ego 6 columns
    of the self row | 6 columns per partner row, in float64.

MARGIN.  Float32 rounding can turn one verdict: length() > radius.  A pair with |distance - radius| < band may go either way --
unless the verdict is exact in any IEEE arithmetic (`exact_verdict`): the two agents stand on the same exported point (the
difference is 0 and so is every rotation of it), or the ego's rotation is the identity, p_j - p_i is exact in float32 and either
one component is 0 or x*x, y*y, their sum and its root are all exact, like a 3-4-5 offset.  `near` is that mask, [n, n - 1].

`variant=` breaks one rule (VARIANTS); only the CPU suite uses it, to show that the constructed worlds tell the rules apart."""
import numpy as np

from tests import geom_reference as GR
from tests import parity as P

f32 = np.float32
f64 = np.float64
PI = float(np.pi)
ZERO = np.asarray([0, 0, 0, 0, 0, 0, 0, 0, -1], f64)               # PartnerObservation::zero(), src/types.hpp
ZERO_NONEXIST = np.asarray([0, 0, 0, 0, 0, 0, 0, 0, -2], f64)      # PartnerObservation::zero_nonexist()
SPEED, X, Y, HEADING, LENGTH, WIDTH, HEIGHT, TYPE, ID = range(9)
EXACT_COLS = [SPEED, LENGTH, WIDTH, HEIGHT, TYPE, ID]
VARIANTS = ("ge_radius", "no_ego_skip", "rotate_plus_yaw", "heading_reversed", "no_heading_wrap", "relative_speed", "ego_size",
            "ids_swapped", "radius_on_unskipped_pair")


def snapshot(sim):
    """Copies of the tensors the reference reads, and of the rows it states."""
    g = GR._np
    return dict(shape=g(sim.shape_tensor()).copy(), abs_obs=g(sim.absolute_self_observation_tensor()).copy(),
                self_obs=g(sim.self_observation_tensor()).copy(), etype=g(sim.info_tensor())[..., 4].copy(),
                rows=g(sim.partner_observations_tensor()).copy())


def wrap(a):
    a = np.asarray(a, f64)
    return a - 2 * PI * np.round(a / (2 * PI))


def angular_distance(a, b):
    return np.abs(wrap(np.asarray(a, f64) - np.asarray(b, f64)))


def partner_of(n):
    """[n, n - 1] int: the agent in slot k of ego i (every other agent in index order)."""
    k = np.arange(max(n - 1, 0))[None, :]
    i = np.arange(n)[:, None]
    return np.where(k < i, k, k + 1)


def exact_verdict(pos, quat, J):
    """[n, n - 1] bool: length() > radius has the same answer in any IEEE arithmetic (see MARGIN).  pos [n, 2] and quat [n, 4]
    are the exported float32 values."""
    pos64 = np.asarray(pos, f64)
    dx, dy = pos64[J, 0] - pos64[:, None, 0], pos64[J, 1] - pos64[:, None, 1]
    same_point = (dx == 0) & (dy == 0)
    identity = (np.asarray(quat, f32) == np.asarray([1, 0, 0, 0], f32)).all(-1)[:, None]
    rep = lambda v: v.astype(f32).astype(f64) == v
    sx, sy = dx * dx, dy * dy
    root = np.sqrt(sx + sy)
    pythagorean = rep(sx) & rep(sy) & rep(sx + sy) & rep(root) & (root * root == sx + sy)
    return same_point | (identity & rep(dx) & rep(dy) & ((dx == 0) | (dy == 0) | pythagorean))


def partner_reference(inp, w, radius, band, variant=None):
    """World w of a snapshot.  Returns dict(n, J [n, n - 1], rows [n, A - 1, 9] float64, obs [n, n - 1, 9] (every pair's row
    before the radius), dist, inside, exact, near [n, n - 1])."""
    n = int(inp["shape"][w, 0])
    slots = inp["rows"].shape[2] if "rows" in inp else inp["abs_obs"].shape[1] - 1
    ab = np.asarray(inp["abs_obs"][w, :n], f64)
    x, y, yaw = ab[:, 0], ab[:, 1], GR.yaw_of(inp["abs_obs"][w, :n, 3:7])
    speed = np.asarray(inp["self_obs"][w, :n, 0], f64)
    size, ids, etype = ab[:, 10:13], ab[:, 13], np.asarray(inp["etype"][w, :n], f64)
    J = partner_of(n)
    Jrow = np.minimum(np.arange(max(n - 1, 0))[None, :] + 0 * J, n - 1) if variant == "no_ego_skip" else J
    i = np.arange(n)[:, None] + 0 * J
    dx, dy = x[Jrow] - x[i], y[Jrow] - y[i]
    turn = yaw[i] if variant == "rotate_plus_yaw" else -yaw[i]
    c, s = np.cos(turn), np.sin(turn)
    obs = np.zeros((n, max(n - 1, 0), 9), f64)
    obs[..., X], obs[..., Y] = c * dx - s * dy, s * dx + c * dy
    rel = yaw[i] - yaw[Jrow] if variant == "heading_reversed" else yaw[Jrow] - yaw[i]
    obs[..., HEADING] = rel if variant == "no_heading_wrap" else wrap(rel)
    obs[..., SPEED] = np.abs(speed[Jrow] - speed[i]) if variant == "relative_speed" else speed[Jrow]
    obs[..., LENGTH:HEIGHT + 1] = size[i] if variant == "ego_size" else size[Jrow]
    obs[..., TYPE], obs[..., ID] = etype[Jrow], ids[Jrow]
    dist = np.hypot(obs[..., X], obs[..., Y])
    if variant == "radius_on_unskipped_pair":      # the radius tested before the rotation, on agent k instead of agent j
        K = np.arange(max(n - 1, 0))[None, :] + 0 * J
        verdict_dist = np.hypot(x[K] - x[i], y[K] - y[i])
    else:
        verdict_dist = dist
    inside = verdict_dist < radius if variant == "ge_radius" else verdict_dist <= radius
    exact = exact_verdict(inp["abs_obs"][w, :n, 0:2], inp["abs_obs"][w, :n, 3:7], J)
    near = (np.abs(dist - radius) < band) & ~exact
    out_row, pad_row = (ZERO_NONEXIST, ZERO) if variant == "ids_swapped" else (ZERO, ZERO_NONEXIST)
    rows = np.tile(pad_row, (n, slots, 1))
    rows[:, :max(n - 1, 0)] = np.where(inside[..., None], obs, out_row)
    return dict(n=n, J=J, rows=rows, obs=obs, dist=dist, inside=inside, exact=exact, near=near, pad_row=pad_row, out_row=out_row)


def is_zero_row(rows, which=ZERO):
    return (np.asarray(rows, f64) == which).all(-1)


def same_heading_pairs(quat):
    """[n, n] bool from the exported (w, x, y, z) float32 rotations: the pairs for which (w, z) of inverse(ego) * other, computed
    in plain float32 products and sums, has w * z == 0 -- equal headings (z == 0) and exactly opposite ones (w == 0)."""
    q = np.asarray(quat, f32)
    ew, ez, rw, rz = q[:, None, 0], q[:, None, 3], q[None, :, 0], q[None, :, 3]
    pw = (ew * rw).astype(f32) + (ez * rz).astype(f32)
    pz = (ew * rz).astype(f32) - (ez * rw).astype(f32)
    return (pw.astype(f32) * pz.astype(f32)) == 0, pw == 0


# ------------------------------------------------------------------------------------------------------------------
# the packed head
# ------------------------------------------------------------------------------------------------------------------
def head_width(slots):
    return 6 + slots * 6


def packed_head(self_obs, rows):
    """[..., 6 + (A - 1) * 6] float64: ego columns | partner columns of P.pack_observation_f64."""
    slots = rows.shape[-2]
    none = np.zeros(rows.shape[:-2] + (1, 9), f64)
    return P.pack_observation_f64(self_obs, rows, none)[..., :head_width(slots)]


def head_gain(slots):
    return P.pack_column_gain(slots + 1)[:head_width(slots)]
