"""Float64 statement of the agent road rows (agent_roadmap_tensor), written from the definition, numpy
and libstdc++ only.

It reads the tensors every simulator exports -- the absolute self rows (position, rotation), map_observation_tensor (the
world's global road rows) and shape_tensor -- plus the radius, K and the mode, and states the K rows of one agent.  The float32
inputs are taken as exact, so the same function checks the oracle on the CPU and the kernels on the GPU.  No oracle, no engine
internals.

  observationOf (reference src/utils.hpp:27-65): position = R(-yaw) (road - ego), heading = wrap(road heading - yaw), scale,
    type, id and mapType copied.  Headings are compared modulo 2 pi.  (The +pi that the reference's own test pins for an
    exactly opposite road, tests/EgocentricRoadObservationTests.cpp:9-22, belongs to the quaternion it builds from 270 degrees;
    a road's exported heading lies in (-pi, pi], its quaternion is the other of the two, and the sign of that pi with it: the
    exported tensors cannot tell the two apart, so no sign is pinned here.)
  k-NN, the reference's order (src/knn.hpp:103-158): fewer than K roads -> radiusFilter over the roads in index order, then
    fillZeros; otherwise make_heap on the first K, one cmp against heap[0] per later road, pop_heap / store / push_heap, then
    radiusFilter (length() <= radius, compaction by swapping from the end), then fillZeros (all zero: id 0, mapType 0).  The
    heap is libstdc++'s (tests/heap_pin.cpp, float64 keys), which also reports the smallest gap between unequal keys over the
    comparisons it performed.
  k-NN, set order: the same set; ties at the K-th key go to the lowest road index.
  linear (src/sim.cpp:258-279): the first K roads in index order with distance <= radius, in that order, then
    MapObservation::zero() (id -1, mapType -1).

MARGINS.  Float32 rounding can turn three verdicts:
  * length() <= radius: a road with |distance - radius| < band may go either way -- unless the verdict is exact in any IEEE
    arithmetic (`exact_verdict`: the agent's rotation is the identity, road - ego is exact in float32, and either one component
    is 0 or x*x, y*y, their sum and its root are all exact, like a 3-4-5 offset);
  * which roads are the K nearest (set order, and the set of a reference-order agent): a road whose key lies within the key
    margin of the K-th key, when an unequal key across the cut does, may go either way;
  * the reference order: an agent is ORDER-DECIDED when the smallest gap over the comparisons its heap run performed exceeds
    TWICE the key margin (each of the two keys may be off by one margin).  Identical exported points give equal keys in any
    arithmetic: they are exact ties and do not count.
An agent with a marginal road is `marginal`; one that is not order-decided is held to the set.  Gaps and key errors are
measured as |a - b| / (max(a, b) + 1): relative far out, absolute (m^2) next to the agent, where a relative error means nothing.

`variant=` breaks one rule (VARIANTS); only the CPU suite uses it, to show that the constructed worlds tell the rules apart."""
import numpy as np

from tests import geom_reference as GR
from tests import heap_pin as HP

f32 = np.float32
f64 = np.float64
PI = float(np.pi)
K = 200                                   # GD_MAP_OBS_K, consts::kMaxAgentMapObservationsCount
KNN, SET, LINEAR = "knn", "set", "linear"
PAD_KNN = np.zeros(9, f64)                                            # fillZeros, src/knn.hpp:19-28
PAD_ZERO = np.asarray([0, 0, 0, 0, 0, 0, 0, -1, -1], f64)             # MapObservation::zero(), src/types.hpp:219-229
VARIANTS = ("lt_radius", "filter_before_k", "stable_compaction", "zero_padding_knn", "no_heading_wrap", "rotate_plus_yaw",
            "ties_to_highest", "linear_no_stop", "linear_k_nearest")


def snapshot(sim):
    """Copies of the tensors the reference reads, and of the rows it states."""
    g = GR._np
    return dict(shape=g(sim.shape_tensor()).copy(), abs_obs=g(sim.absolute_self_observation_tensor()).copy(),
                map_obs=g(sim.map_observation_tensor()).copy(), rows=g(sim.agent_roadmap_tensor()).copy())


def wrap(a):
    a = np.asarray(a, f64)
    return a - 2 * PI * np.round(a / (2 * PI))


def angular_distance(a, b):
    return np.abs(wrap(np.asarray(a, f64) - np.asarray(b, f64)))


def observation_of(roads, x, y, yaw, variant=None):
    """[R, 9] float64: every global road row in the frame of the agent at (x, y) turned by yaw."""
    roads = np.asarray(roads, f64)
    dx, dy = roads[:, 0] - f64(x), roads[:, 1] - f64(y)
    turn = f64(yaw) if variant == "rotate_plus_yaw" else -f64(yaw)
    c, s = np.cos(turn), np.sin(turn)
    out = roads.copy()
    out[:, 0], out[:, 1] = c * dx - s * dy, s * dx + c * dy
    out[:, 5] = roads[:, 5] - f64(yaw) if variant == "no_heading_wrap" else wrap(roads[:, 5] - f64(yaw))
    return out


def exact_verdict(roads, x, y, quat):
    """[R] bool: length() <= radius has the same answer in any IEEE arithmetic (see MARGINS)."""
    roads = np.asarray(roads, f64)
    if not np.array_equal(np.asarray(quat, f32), np.asarray([1, 0, 0, 0], f32)):
        return np.zeros(len(roads), bool)
    dx, dy = roads[:, 0] - f64(x), roads[:, 1] - f64(y)
    rep = lambda v: v.astype(f32).astype(f64) == v
    sub = rep(dx) & rep(dy)
    sx, sy = dx * dx, dy * dy
    root = np.sqrt(sx + sy)
    pythagorean = rep(sx) & rep(sy) & rep(sx + sy) & rep(root) & (root * root == sx + sy)
    return sub & ((dx == 0) | (dy == 0) | pythagorean)


def radius_filter(heap, dist, radius, variant=None):
    """src/knn.hpp:83-97 on an array of road indices: returns the compacted array."""
    heap = list(heap)
    inside = (lambda r: dist[r] < radius) if variant == "lt_radius" else (lambda r: dist[r] <= radius)
    if variant == "stable_compaction":
        return [r for r in heap if inside(r)]
    beyond, idx = len(heap), 0
    while idx < beyond:
        if inside(heap[idx]):
            idx += 1
            continue
        beyond -= 1
        heap[idx] = heap[beyond]
    return heap[:beyond]


def gap(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return np.abs(a - b) / (np.maximum(a, b) + 1.0)


def road_core(inp, w, a, radius, mode, variant=None, k=K):
    """What road_reference states before any margin: obs [R, 9], keys, dist [R], order (road indices, row by row), pad, exact
    (exact_verdict), heap / inserts / min_gap (reference order)."""
    R = int(inp["shape"][w, 1])
    roads = np.asarray(inp["map_obs"][w, :R], f64)
    ab = inp["abs_obs"][w, a]
    x, y, yaw = f64(ab[0]), f64(ab[1]), float(GR.yaw_of(ab[3:7]))
    obs = observation_of(roads, x, y, yaw, variant)
    keys = obs[:, 0] * obs[:, 0] + obs[:, 1] * obs[:, 1]
    dist = np.sqrt(keys)
    inside = dist < radius if variant == "lt_radius" else dist <= radius
    out = dict(obs=obs, keys=keys, dist=dist, inside=inside, exact=exact_verdict(roads, x, y, ab[3:7]), R=R, heap=None, inserts=0,
               min_gap=float("inf"), mode=mode, radius=radius, k=k)
    pad = PAD_KNN
    if mode == LINEAR:
        pad = PAD_ZERO
        if variant == "linear_k_nearest":
            cand = np.nonzero(inside)[0]
            order = sorted(cand[np.argsort(keys[cand], kind="stable")[:k]].tolist())
        elif variant == "linear_no_stop":
            order = np.nonzero(inside)[0][-k:].tolist()
        else:
            order = np.nonzero(inside)[0][:k].tolist()
    else:
        if variant == "zero_padding_knn":
            pad = PAD_ZERO
        if variant == "filter_before_k":
            pool = np.nonzero(inside)[0]
            sub_order, _ = HP.libstdcxx_order_f64(keys[pool], np.inf, k)
            order = [int(pool[i]) for i in sub_order if i >= 0]
            out["selected"] = list(order)
        else:
            if mode == KNN:
                heap, out["min_gap"] = HP.libstdcxx_order_f64(keys, np.inf, k)
                heap = [int(r) for r in heap if r >= 0]
                out["heap"] = list(heap)
                out["inserts"] = _count_inserts(keys, k)
            else:
                by_key = np.lexsort((-np.arange(R) if variant == "ties_to_highest" else np.arange(R), keys))[:k]
                heap = sorted(by_key.tolist())
            out["selected"] = list(heap)
            order = radius_filter(heap, dist, radius, variant)
    rows = np.tile(pad, (k, 1))
    idx = np.full(k, -1, np.int64)
    rows[:len(order)] = obs[order]
    idx[:len(order)] = order
    out.update(rows=rows, order=idx, pad=pad)
    return out


def _linear_margins(out, near_radius, key_margin, band):
    """(required, optional, decided, cut_ties) in linear mode: only the radius has a margin."""
    inside, k = out["inside"], out["k"]
    # a road in the band may be in or out, which moves the cut behind it
    sure, maybe = inside & ~near_radius, near_radius
    lo = np.cumsum(sure) - sure              # roads certainly taken before this one
    hi = np.cumsum(sure | maybe) - (sure | maybe)
    required = set(np.nonzero(sure & (hi < k))[0].tolist())
    optional = set(np.nonzero((sure | maybe) & (lo < k))[0].tolist()) - required
    return required, optional, True, set()


def _knn_margins(out, near_radius, key_margin, band):
    """(required, optional, decided, cut_ties) of a k-NN selection: the radius, the K-th cut and the heap's order."""
    keys, dist, inside, R, k, radius, mode = out["keys"], out["dist"], out["inside"], out["R"], out["k"], out["radius"], out["mode"]
    chosen = np.zeros(R, bool)
    # (reference order: what the heap holds -- among equal keys at the cut, whichever its history left; set order: the lowest indices)
    chosen[out["selected"]] = True
    at_cut = np.zeros(R, bool)      # unequal keys that float32 may order the other way across the K-th cut
    cut = np.zeros(R, bool)         # an exact tie that straddles the cut
    if R > k and chosen.any():
        kth = keys[chosen].max()
        if (keys[~chosen] == kth).any():
            cut = (keys == kth) & (dist <= radius + band)
        nxt = keys[~chosen & (keys != kth)].min() if (~chosen & (keys != kth)).any() else np.inf
        if np.isfinite(nxt) and gap(kth, nxt) <= 2 * key_margin:
            # the cut runs between two unequal keys that float32 may order the other way: every road whose key lies within
            # reach of either may be on either side (exact ties among them still go to the lowest index)
            at_cut = ((gap(keys, kth) <= 2 * key_margin) | (gap(keys, nxt) <= 2 * key_margin)) & (dist <= radius + band)
    at_radius = (chosen | at_cut) & near_radius
    decided = mode != KNN or out["min_gap"] > 2 * key_margin or not (dist <= radius + band).any()
    maybe = at_cut | at_radius | (cut & (not decided))      # (another order of inserts leaves other members of a tie)
    required = set(np.nonzero(chosen & inside & ~maybe)[0].tolist())
    optional = set(np.nonzero(maybe)[0].tolist())
    return required, optional, decided, set(np.nonzero(cut)[0].tolist())


def road_reference(inp, w, a, radius, mode, key_margin, band, variant=None, k=K, core=None):
    """The rows of agent (w, a).  key_margin: how far one key may be off, on the scale of `gap`; band: how far one distance may be
    off (metres).  Returns road_core's dict plus
      required / optional: road index sets of the selection (optional: may go either way), near_radius [R],
      marginal: some road of this agent is optional; decided: the row ORDER is held (reference order only; an agent out of
      reach of every road has no order to hold); cut_ties: the roads of a tie that straddles the K-th key."""
    out = dict(core if core is not None else road_core(inp, w, a, radius, mode, variant, k))
    near_radius = (np.abs(out["dist"] - radius) < band) & ~out["exact"]
    margins = _linear_margins if mode == LINEAR else _knn_margins
    required, optional, decided, out["cut_ties"] = margins(out, near_radius, key_margin, band)
    out.update(near_radius=near_radius, required=required, optional=optional, marginal=bool(optional), decided=decided)
    return out


def _count_inserts(keys, k):
    """How many of the roads behind the first k pass cmp(current, heap[0]) (src/knn.hpp:139-145)."""
    import heapq
    if len(keys) <= k:
        return 0
    heap = [-v for v in keys[:k]]
    heapq.heapify(heap)
    n = 0
    for v in keys[k:]:
        if v < -heap[0]:
            heapq.heapreplace(heap, -v)
            n += 1
    return n
