"""Float64 references of the two observation kernels that had none: the BEV rasteriser and the LiDAR model, written from
their definitions with plain cos / sin rotations in the plane, numpy only.

Both read the tensors every simulator exports and nothing else (`read_inputs`): shape_tensor, the 11-float agent state
(position, quaternion), absolute_self_observation_tensor (sizes), info_tensor (agent type), controlled_state_tensor,
action_tensor (head angle, column 2) and map_observation_tensor (road x, y, the three scales, heading, type).  The float32
inputs are taken as exact.  The same functions therefore check the oracle on the CPU and the kernels on the GPU.

Each function also returns a MARGIN MASK computed from the reference alone (DELTA = 1e-3 m): the cells / rays whose value
hangs on a comparison that float32 rounding can turn.  Outside the mask the float32 implementations must agree with the
reference exactly (cell value, hit / miss, entity type).

BEV rule (reference src/sim.cpp:462-555, src/rasterizer.hpp:12-78): the first 200 roads in road order whose centre is within
the observation radius of the ego, then the partners within the radius in slot order, are painted as rotated rectangles in
the ego frame, later paints over earlier ones.  A road is handed over with its FIRST SCALE (the segment's half length) as
"length" and its second scale, floored at one cell, as "width"; the rasteriser halves both.  The centre cell is truncated and
clamped; the cells tested are the square of box_radius = ceil(sqrt(2) * max half side / cell) cells around it; a cell is
painted when its centre's local coordinates lie within the half extents + 1e-3.

LiDAR model (the rules above ray_box in oracle/gd_oracle.c): 50 rays per plane at half * (2 idx / 50 - 1) + head_angle from
the agent's heading axis; planes at z + 0.5, + 0.1, - 0.1 above the agent's z; an entity is eligible on a plane whose height
its z range contains (agents [z, z + 1.4]; road edges 1.1 +- d2, stop signs 1 +- d2, other roads 0.9 +- d2); entities are
2-D boxes (agents: half extents 0.7 * size / 2, roads: their first two scales); front faces only, 0 < t <= 200; the nearest
hit wins, equal distances go to the lowest entity row (agents in slot order, then roads in road order)."""
import numpy as np

RES = 200
K_ROADS = 200
PAINT_EPS = 1e-3
DELTA = 1e-3          # metres: the width of every margin band
Z_DELTA = 1e-6        # plane height against a z bound
CELL_DELTA = 1e-6     # centre cell coordinate against an integer
N_RAYS = 50
LIDAR_RANGE = 200.0
PLANE_OFFSETS = (0.5, 0.1, -0.1)
VEHICLE_SCALE = np.float32(0.7)
ET_ROAD_EDGE, ET_STOP_SIGN = 1, 6


def _np(t):
    if hasattr(t, "to_torch"):
        t = t.to_torch()
    if hasattr(t, "detach"):
        return t.detach().cpu().numpy()
    return np.asarray(t)


def read_inputs(sim):
    """Copies of the tensors the references read, from the oracle (get_state) or the HIP simulator (debug_get_state)."""
    state = sim.get_state() if hasattr(sim, "get_state") else sim.debug_get_state()
    return dict(shape=_np(sim.shape_tensor()).copy(), state=np.array(state, np.float32),
                abs_obs=_np(sim.absolute_self_observation_tensor()).copy(), info=_np(sim.info_tensor()).copy(),
                controlled=_np(sim.controlled_state_tensor()).copy(), action=_np(sim.action_tensor()).copy(),
                map_obs=_np(sim.map_observation_tensor()).copy())


def yaw_of(q):
    """Heading of a (w, x, y, z) rotation about the vertical axis."""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def _to_frame(x, y, ox, oy, yaw):
    """(x, y) in the frame at (ox, oy) turned by yaw."""
    c, s = np.cos(yaw), np.sin(yaw)
    dx, dy = x - ox, y - oy
    return c * dx + s * dy, -s * dx + c * dy


# ------------------------------------------------------------------------------------------------------------------
# BEV
# ------------------------------------------------------------------------------------------------------------------
def bev_entities(inp, w, a, radius):
    """The rectangles of agent a's raster in paint order: rows (cx, cy, yaw, length, width, type) in the ego frame, the
    number of them that are roads, and whether a discrete decision (in / out of the radius) sits on a knife edge."""
    n, R = (int(v) for v in inp["shape"][w])
    st = inp["state"][w].astype(np.float64)
    ex, ey, eyaw = st[a, 0], st[a, 1], yaw_of(st[a, 3:7])
    mo = inp["map_obs"][w, :R].astype(np.float64)
    rx, ry = _to_frame(mo[:, 0], mo[:, 1], ex, ey, eyaw)
    dist = np.hypot(rx, ry)
    sel = np.nonzero(dist <= radius)[0][:K_ROADS]
    seen = R if len(sel) < K_ROADS else int(sel[-1]) + 1   # roads behind the 200th in reach decide nothing
    knife = bool((np.abs(dist[:seen] - radius) < DELTA).any())
    minw = 2 * radius / RES
    rows = [(rx[r], ry[r], mo[r, 5] - eyaw, mo[r, 2], max(mo[r, 3], minw), int(mo[r, 6])) for r in sel]
    n_roads = len(rows)
    for j in range(n):
        if j == a:
            continue
        px, py = _to_frame(st[j, 0], st[j, 1], ex, ey, eyaw)
        d = np.hypot(px, py)
        knife = knife or bool(abs(d - radius) < DELTA)
        if d <= radius:
            rows.append((px, py, yaw_of(st[j, 3:7]) - eyaw, float(inp["abs_obs"][w, j, 10]), float(inp["abs_obs"][w, j, 11]),
                         int(inp["info"][w, j, 4])))
    return np.asarray(rows, np.float64).reshape(-1, 6), n_roads, knife


def paint_rectangles(rows, radius):
    """Paint the rectangles in order.  Returns (grid [RES, RES] of types indexed [y, x], margin mask, knife)."""
    grid = np.zeros((RES, RES), np.int32)
    margin = np.zeros((RES, RES), bool)
    knife = False
    cell = 2 * radius / RES
    for cx, cy, yaw, length, width, etype in rows:
        fx, fy = (cx + radius) / cell, (cy + radius) / cell
        knife = knife or abs(fx - np.rint(fx)) < CELL_DELTA or abs(fy - np.rint(fy)) < CELL_DELTA
        gx = min(max(int(np.trunc(fx)), 0), RES - 1)
        gy = min(max(int(np.trunc(fy)), 0), RES - 1)
        half_l, half_w = length / 2, width / 2
        brf = np.sqrt(2.0) * max(half_l, half_w) / cell
        knife = knife or abs(brf - np.rint(brf)) < CELL_DELTA
        br = int(np.ceil(brf))
        x0, x1, y0, y1 = max(gx - br, 0), min(gx + br, RES - 1), max(gy - br, 0), min(gy + br, RES - 1)
        ldx = (np.arange(x0, x1 + 1) * cell - radius - cx)[None, :]
        ldy = (np.arange(y0, y1 + 1) * cell - radius - cy)[:, None]
        c, s = np.cos(-yaw), np.sin(-yaw)
        ax, ay = np.abs(ldx * c - ldy * s), np.abs(ldx * s + ldy * c)
        tx, ty = half_l + PAINT_EPS, half_w + PAINT_EPS
        sub = grid[y0:y1 + 1, x0:x1 + 1]
        sub[(ax <= tx) & (ay <= ty)] = int(etype)
        margin[y0:y1 + 1, x0:x1 + 1] |= ((np.abs(ax - tx) < DELTA) & (ay <= ty + DELTA)) | \
                                       ((np.abs(ay - ty) < DELTA) & (ax <= tx + DELTA))
    return grid, margin, bool(knife)


def bev_reference(inp, w, a, radius):
    """Agent a's raster.  Returns a dict: grid [200, 200] int (indexed [y, x]), margin [200, 200] bool, usable (False when a
    discrete decision sits on a knife edge: the raster must not be used), n_roads, n_partners."""
    radius = float(np.float32(radius))
    rows, n_roads, knife_r = bev_entities(inp, w, a, radius)
    grid, margin, knife_c = paint_rectangles(rows, radius)
    return dict(grid=grid, margin=margin, usable=not (knife_r or knife_c), n_roads=n_roads, n_partners=len(rows) - n_roads)


# ------------------------------------------------------------------------------------------------------------------
# LiDAR
# ------------------------------------------------------------------------------------------------------------------
def lidar_half_angle(half_angle):
    """The half cone the simulators use: the float32 parameter, or float32 pi / 3 when it is not positive."""
    h = np.float32(half_angle)
    return float(h) if h > 0 else float(np.float32(np.float32(np.pi) / np.float32(3)))


def lidar_entities(inp, w):
    """The boxes of world w in entity-row order (agents, then roads): dict of float64 arrays cx, cy, yaw, hx, hy, zlo, zhi and
    int type; n agents first."""
    n, R = (int(v) for v in inp["shape"][w])
    st = inp["state"][w, :n].astype(np.float64)
    size = inp["abs_obs"][w, :n, 10:12].astype(np.float32)
    half = ((size / np.float32(2)) * VEHICLE_SCALE).astype(np.float64)   # the entity's stored scale (float32 arithmetic)
    mo = inp["map_obs"][w, :R].astype(np.float64)
    rtype = mo[:, 6].astype(np.int64)
    zc = np.where(rtype == ET_ROAD_EDGE, 1.1, np.where(rtype == ET_STOP_SIGN, 1.0, 0.9))
    cat = np.concatenate
    return dict(n=n, cx=cat([st[:, 0], mo[:, 0]]), cy=cat([st[:, 1], mo[:, 1]]), yaw=cat([yaw_of(st[:, 3:7]), mo[:, 5]]),
                hx=cat([half[:, 0], mo[:, 2]]), hy=cat([half[:, 1], mo[:, 3]]),
                zlo=cat([st[:, 2], zc - mo[:, 4]]), zhi=cat([st[:, 2] + 2 * 0.7, zc + mo[:, 4]]),
                type=cat([inp["info"][w, :n, 4].astype(np.int64), rtype]))


def plane_masks(ents, oz):
    """[3, E] bool: entity eligible on the plane; and [3, E] bool: the plane's height within Z_DELTA of one of its z bounds."""
    rz = np.asarray([oz + o for o in PLANE_OFFSETS])[:, None]
    elig = (rz >= ents["zlo"][None, :]) & (rz <= ents["zhi"][None, :])
    near = (np.abs(rz - ents["zlo"][None, :]) < Z_DELTA) | (np.abs(rz - ents["zhi"][None, :]) < Z_DELTA)
    return elig, near


def _slab(lox, loy, ldx, ldy, hx, hy):
    """Ray lo + t ld against the box |x| <= hx, |y| <= hy: (tmin, tmax); an empty interval has tmax < tmin."""
    tmin = np.full(np.broadcast(lox, ldx).shape, -np.inf)
    tmax = np.full(tmin.shape, np.inf)
    for lo, ld, h in ((lox, ldx, hx), (loy, ldy, hy)):
        lo, ld, h = np.broadcast_to(lo, tmin.shape), np.broadcast_to(ld, tmin.shape), np.broadcast_to(h, tmin.shape)
        par = ld == 0
        safe = np.where(par, 1.0, ld)
        t1, t2 = (-h - lo) / safe, (h - lo) / safe
        a, b = np.minimum(t1, t2), np.maximum(t1, t2)
        outside = par & ((lo < -h) | (lo > h))
        a = np.where(par, np.where(outside, np.inf, -np.inf), a)
        b = np.where(par, np.where(outside, -np.inf, np.inf), b)
        tmin, tmax = np.maximum(tmin, a), np.minimum(tmax, b)
    return tmin, tmax


def _hits(tmin, tmax):
    return (tmax >= tmin) & (tmin > 0) & (tmin <= LIDAR_RANGE)


def ray_angles(half, head):
    return half * (2 * np.arange(N_RAYS) / N_RAYS - 1) + head


def lidar_reference(inp, w, a, half_angle, ents=None):
    """Agent a's returns.  Returns a dict: out [3, 50, 4] float64 (depth, type, x, y; zeros for a miss), margin [3, 50] bool,
    row [3, 50] int (the entity row hit, -1 for a miss)."""
    ents = ents or lidar_entities(inp, w)
    half = lidar_half_angle(half_angle)
    st = inp["state"][w, a].astype(np.float64)
    ox, oy, oz, eyaw = st[0], st[1], st[2], yaw_of(st[3:7])
    head = float(inp["action"][w, a, 2]) if inp["controlled"][w, a, 0] else 0.0
    theta = ray_angles(half, head)
    dx, dy = np.cos(theta + eyaw)[:, None], np.sin(theta + eyaw)[:, None]
    c, s = np.cos(ents["yaw"])[None, :], np.sin(ents["yaw"])[None, :]
    rx, ry = (ox - ents["cx"])[None, :], (oy - ents["cy"])[None, :]
    lox, loy = c * rx + s * ry, -s * rx + c * ry
    ldx, ldy = c * dx + s * dy, -s * dx + c * dy
    hx, hy = ents["hx"][None, :], ents["hy"][None, :]
    tmin, tmax = _slab(lox, loy, ldx, ldy, hx, hy)
    hit = _hits(tmin, tmax)
    # the same test on the box grown and shrunk by DELTA: where the answers differ the ray grazes the box
    tmin_g, tmax_g = _slab(lox, loy, ldx, ldy, hx + DELTA, hy + DELTA)
    grown = _hits(tmin_g, tmax_g)
    shrunk = _hits(*_slab(lox, loy, ldx, ldy, np.maximum(hx - DELTA, 0), np.maximum(hy - DELTA, 0)))
    inrange = (tmin > -DELTA) & (tmin < LIDAR_RANGE + DELTA)
    graze = ((np.abs(tmax - tmin) < DELTA) & inrange) | (grown != hit) | (shrunk != hit)
    edge_t = (tmax >= tmin - DELTA) & ((np.abs(tmin) < DELTA) | (np.abs(tmin - LIDAR_RANGE) < DELTA))
    soft = graze | edge_t                                    # [50, E]
    elig, near_z = plane_masks(ents, oz)
    elig[:, a] = False
    near_z[:, a] = False
    out = np.zeros((3, N_RAYS, 4))
    margin = np.zeros((3, N_RAYS), bool)
    row = np.full((3, N_RAYS), -1, np.int64)
    types = ents["type"]
    why = dict(graze=0, range=0, two_types=0, z=0)   # rays marked, by rule (a ray can be marked by several)
    for p in range(3):
        t = np.where(hit & elig[p][None, :], tmin, np.inf)
        best = np.argmin(t, axis=1)                          # the first of equal distances: the lowest entity row
        tb = t[np.arange(N_RAYS), best]
        got = np.isfinite(tb)
        tb = np.where(got, tb, 0.0)
        row[p] = np.where(got, best, -1)
        out[p, :, 0] = np.where(got, tb, 0.0)
        out[p, :, 1] = np.where(got, types[best], 0)
        out[p, :, 2] = np.where(got, tb * np.cos(theta), 0.0)
        out[p, :, 3] = np.where(got, tb * np.sin(theta), 0.0)
        # a box the ray grazes decides nothing from behind a firm nearest hit: it counts where the grown box is entered
        # before that hit + DELTA
        matters = elig[p][None, :] & (tmin_g < np.where(got, tb, np.inf)[:, None] + DELTA)
        m = (soft & matters).any(axis=1)
        why["graze"] += int((graze & matters).any(axis=1).sum())
        why["range"] += int((edge_t & matters).any(axis=1).sum())
        # another entity type within DELTA behind the winner (equal distances are decided by the tie rule, not by rounding)
        close = np.isfinite(t) & (t > tb[:, None]) & (t < tb[:, None] + DELTA) & (types[None, :] != types[best][:, None])
        m |= got & close.any(axis=1)
        why["two_types"] += int((got & close.any(axis=1)).sum())
        if near_z[p].any():
            m[:] = True
            why["z"] += N_RAYS
        margin[p] = m
    return dict(out=out, margin=margin, row=row, theta=theta, why=why)


def subtended_rays(inp, w, a, half_angle, ents=None):
    """For every entity: the number of agent a's rays whose direction lies within the angle the entity's bounding circle
    subtends (exact asin / atan2; every ray when the agent is inside the circle), and its plane mask (bit p = plane p)."""
    ents = ents or lidar_entities(inp, w)
    half = lidar_half_angle(half_angle)
    st = inp["state"][w, a].astype(np.float64)
    head = float(inp["action"][w, a, 2]) if inp["controlled"][w, a, 0] else 0.0
    rx, ry = _to_frame(ents["cx"], ents["cy"], st[0], st[1], yaw_of(st[3:7]))
    rho, rb = np.hypot(rx, ry), np.hypot(ents["hx"], ents["hy"])
    phi = np.arctan2(ry, rx)
    alpha = np.where(rho <= rb, np.pi, np.arcsin(np.minimum(1.0, rb / np.maximum(rho, 1e-300))))
    diff = (ray_angles(half, head)[:, None] - phi[None, :] + np.pi) % (2 * np.pi) - np.pi
    count = (np.abs(diff) <= alpha[None, :]).sum(axis=0)
    elig, _ = plane_masks(ents, st[2])
    mask = elig[0] * 1 + elig[1] * 2 + elig[2] * 4
    count[a] = 0
    mask[a] = 0
    count = np.where(rho > LIDAR_RANGE + rb, 0, count)
    return count, mask
