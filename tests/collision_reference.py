"""Float64 statement of collision detection, written from its definition, numpy only.

It reads the tensors every simulator exports and nothing else: what tests/geom_reference.py reads (shape, the 11-float agent
state, sizes, agent types, map_observation_tensor) plus response_type_tensor, done_tensor, steps_remaining_tensor and the valid
flags of expert_trajectory_tensor.  The float32 inputs are taken as exact, so the same functions check the oracle on the CPU
and the kernel on the GPU.

The rule (reference src/sim.cpp:628-747, src/obb.hpp:12-82, src/sim.hpp:88-102):
  * every agent is a rectangle with half extents 0.7 * size / 2 around its position, turned by its heading; every road
    entity -- ALL rows of map_observation_tensor, whatever their type -- is a rectangle with its first two scales as half
    extents;
  * two rectangles overlap when no edge normal of either separates them; touching counts as overlap;
  * a pair is looked at when both are active, not both are Static (a Static body and a road never make a pair either: the
    road is Static too) and their types are not one of the 14 filtered pairs;
  * an agent is active when it is not at the padding height, and -- if nobody controls it -- its log is valid at the current
    step, or -- if it is controlled -- it is not (done and not collided) (src/sim.cpp:631-662);
  * an agent of an overlapping pair is collided, and one of info[0:3] is set after the OTHER's type: a road type (1..6)
    sets column 0, a vehicle column 1, a pedestrian or cyclist column 2 (src/sim.cpp:708-744).

`separation` is the largest gap between the two rectangles' projections over the four edge normals: <= 0 is overlap.  A
float32 implementation can give the other verdict where |separation| is small, so `collision_reference` also returns a margin
flag per agent: one of its pairs lies within `band` of touching."""
import numpy as np

from tests import geom_reference as GR

ET_NONE, ET_ROAD_EDGE, ET_ROAD_LINE, ET_ROAD_LANE, ET_CROSSWALK, ET_SPEED_BUMP, ET_STOP_SIGN, ET_VEHICLE, ET_PEDESTRIAN, \
    ET_CYCLIST = range(10)
RESP_STATIC = 2
PAD_Z = np.float32(np.finfo(np.float32).max)
EPISODE = 91
AGENT_STOP, AGENT_REMOVED, IGNORE = 0, 1, 2   # CollisionBehaviour, reference src/init.hpp

# collisionPairs, src/sim.hpp:88-102: the type pairs that never collide, in either order
FILTERED_PAIRS = (
    (ET_PEDESTRIAN, ET_ROAD_EDGE), (ET_PEDESTRIAN, ET_ROAD_LINE), (ET_PEDESTRIAN, ET_ROAD_LANE), (ET_PEDESTRIAN, ET_CROSSWALK),
    (ET_PEDESTRIAN, ET_SPEED_BUMP),
    (ET_CYCLIST, ET_ROAD_EDGE), (ET_CYCLIST, ET_ROAD_LINE), (ET_CYCLIST, ET_ROAD_LANE), (ET_CYCLIST, ET_CROSSWALK),
    (ET_CYCLIST, ET_SPEED_BUMP),
    (ET_VEHICLE, ET_CROSSWALK), (ET_VEHICLE, ET_SPEED_BUMP), (ET_VEHICLE, ET_ROAD_LINE), (ET_VEHICLE, ET_ROAD_LANE))
FILTER = np.zeros((10, 10), bool)
for _a, _b in FILTERED_PAIRS:
    FILTER[_a, _b] = FILTER[_b, _a] = True
FILTER[ET_NONE, ET_NONE] = True   # the array has 20 entries: the six value-initialised ones are (None, None)


def read_inputs(sim):
    """GR.read_inputs plus the tensors the activity rules read."""
    inp = GR.read_inputs(sim)
    inp["resp"] = GR._np(sim.response_type_tensor())[..., 0].copy()
    inp["done"] = GR._np(sim.done_tensor())[..., 0].copy()
    inp["steps"] = GR._np(sim.steps_remaining_tensor())[..., 0].astype(np.int64)
    inp["valid"] = GR._np(sim.expert_trajectory_tensor())[..., 5 * EPISODE:6 * EPISODE].copy()
    return inp


def separation(A, B):
    """A, B: (cx, cy, yaw, hx, hy), arrays that broadcast against each other.  The largest interval gap over the four edge
    normals; <= 0 means the rectangles overlap (touching included, src/obb.hpp:51-82)."""
    ax, ay, ayaw, ahx, ahy = (np.asarray(v, np.float64) for v in A)
    bx, by, byaw, bhx, bhy = (np.asarray(v, np.float64) for v in B)
    dx, dy = bx - ax, by - ay
    ca, sa, cb, sb = np.cos(ayaw), np.sin(ayaw), np.cos(byaw), np.sin(byaw)
    gaps = []
    for nx, ny in ((ca, sa), (-sa, ca), (cb, sb), (-sb, cb)):
        ra = ahx * np.abs(ca * nx + sa * ny) + ahy * np.abs(-sa * nx + ca * ny)
        rb = bhx * np.abs(cb * nx + sb * ny) + bhy * np.abs(-sb * nx + cb * ny)
        gaps.append(np.abs(dx * nx + dy * ny) - ra - rb)
    return np.maximum(np.maximum(gaps[0], gaps[1]), np.maximum(gaps[2], gaps[3]))


def seen_at_reset(inp):
    """What detection sees on a pass that moves nothing and counts no step: the flags as they stand, nobody collided yet."""
    return dict(done=inp["done"] != 0, collided=np.zeros(inp["done"].shape, bool), step=EPISODE - inp["steps"])


def seen_in_step(before, behaviour):
    """What detection sees during the step that follows the snapshot `before` (read_inputs): the movement comes first and
    marks a collided agent done under AgentStop / AgentRemoved, or forgets its collision under Ignore (src/sim.cpp:302-323);
    the step counter and the goal / end-of-episode done flag change only after detection (src/sim.cpp:589-626)."""
    was = before["state"][..., 10] != 0
    if behaviour == IGNORE:
        return dict(done=before["done"] != 0, collided=np.zeros(was.shape, bool), step=EPISODE - before["steps"])
    return dict(done=(before["done"] != 0) | was, collided=was, step=EPISODE - before["steps"])


def active(inp, w, seen=None):
    """[n] bool, src/sim.cpp:631-662 and the padding position."""
    seen = seen or seen_at_reset(inp)
    n = int(inp["shape"][w, 0])
    k = np.clip(seen["step"][w, :n], 0, EPISODE - 1)
    valid = inp["valid"][w, np.arange(n), k] != 0
    ctl = inp["controlled"][w, :n, 0] != 0
    invalid = np.where(ctl, seen["done"][w, :n] & ~seen["collided"][w, :n], ~valid)
    return (inp["state"][w, :n, 2] != PAD_Z) & ~invalid


def collision_reference(inp, w, band, seen=None):
    """World w.  Returns a dict over the n live agents: collided [n] bool, info [n, 3] int (what THIS pass finds: flags an
    agent carries from before are the caller's, see expected_after_step), margin [n] bool, sep [n, n + R] (agent against agent
    rows, then road rows), pairs [n, n + R] bool (the pairs that are looked at), active [n], ents (GR.lidar_entities)."""
    ents = GR.lidar_entities(inp, w)
    n = ents["n"]
    E = len(ents["cx"])
    act = active(inp, w, seen)
    static = inp["resp"][w, :n] == RESP_STATIC
    rect = [ents[k] for k in ("cx", "cy", "yaw", "hx", "hy")]
    with np.errstate(invalid="ignore", over="ignore"):
        sep = separation([v[:n, None] for v in rect], [v[None, :] for v in rect])
    types = np.clip(ents["type"], 0, 9)
    pairs = ~FILTER[types[:n, None], types[None, :]]
    pairs &= act[:, None]
    pairs[:, :n] &= act[None, :] & ~(static[:, None] & static[None, :]) & ~np.eye(n, dtype=bool)
    pairs[:, n:] &= ~static[:, None]
    hit = pairs & (sep <= 0)
    other = types[None, :].repeat(n, 0)
    info = np.stack([(hit & (other >= ET_ROAD_EDGE) & (other <= ET_STOP_SIGN)).any(1), (hit & (other == ET_VEHICLE)).any(1),
                     (hit & ((other == ET_PEDESTRIAN) | (other == ET_CYCLIST))).any(1)], -1).astype(np.int64)
    margin = (pairs & (np.abs(sep) < band)).any(1)
    assert E == sep.shape[1]
    return dict(collided=hit.any(1), info=info, margin=margin, sep=sep, pairs=pairs, active=act, ents=ents, static=static)


def expected_after_step(prev, fresh, behaviour):
    """The flags a step leaves.  prev: the snapshot before the step (read_inputs); fresh: collision_reference of the tensors
    after it, with seen_in_step(prev, behaviour); both for one world w = fresh["w"] or the caller's slices.

    Ignore: the movement clears what a COLLIDED agent carried (an info column that a pass without movement left on an agent
    whose collided flag was then written as 0 stays: the clearing sits inside `if hasCollided`), and the fresh flags are added.
    AgentStop / AgentRemoved: a collided agent keeps its flags (and may add to them while it is still in place), is done, and
    stands at the padding position when the behaviour is AgentRemoved or the agent is not Static -- a done agent that is not
    Static is always moved there (src/sim.cpp:302-343).  Returns dict(collided, info, done_at_least, padded) over the live
    agents; `padded` holds only the agents this rule sends to the padding position."""
    n = len(fresh["collided"])
    was = prev["state"][:n, 10] != 0
    carried = prev["info"][:n, 0:3] != 0
    if behaviour == IGNORE:
        return dict(collided=fresh["collided"], info=(fresh["info"] != 0) | (carried & ~was[:, None]), done_at_least=np.zeros(n, bool),
                    padded=np.zeros(n, bool))
    static = prev["resp"][:n] == RESP_STATIC
    return dict(collided=fresh["collided"] | was, info=(fresh["info"] != 0) | carried, done_at_least=was,
                padded=was & ((behaviour == AGENT_REMOVED) | ~static))


def world_slice(inp, w):
    """The per-world view expected_after_step takes as `prev`."""
    return dict(state=inp["state"][w], info=inp["info"][w], resp=inp["resp"][w], done=inp["done"][w])
