"""The reference's multi-policy rollout (gpudrive/utils/multi_policy_rollout.py multi_policy_rollout(), lines 36-154, and
compute_metrics, 156-169), restated for the tests of the multi-policy evaluator (gd_owned_rows, gd_policy_forward_owned,
gd_multi_policy_rollout, gpudrive_lab_amd.multi_policy_rollout).  Test infrastructure for test_multi_policy.py and
test_gpu_multi_policy.py; it never imports the evaluator.

  segment_starts(count), owned_list(mask, owner, P)   the owned row list in numpy
  list_patterns / owner_patterns / many_block_patterns the masks and owners of the list and forward cases, shared by the CPU and
                                                      the GPU tests
  owned_list_blocks, blob_of_rows, world_counts_by_wave, summary(first_256=) the same results stated per block of 1024 rows,
                                                      per position, per wave of 64 slots and per lane of 256 worlds, each with
                                                      the WRONG rules the many-block, eight-policy, two-wave and 258-world cases
                                                      are built to see (test_multi_policy.py shows that they do)
  compute_metrics(...), summary(...)                  lines 156-169 in numpy float32, and the per-policy totals
  metrics(control_mask, masks, done, info)            the bookkeeping half of the loop on scripted (done, info) sequences
  run_starts_host / run_metrics_host                  the drivers of the host program (tests/multi_policy_rule_host.cpp)
  closed_loop(sim, policies, table, ...)              the whole loop in torch over a simulator, a `DevicePolicy` per policy
                                                      called on next_obs[mask_p & live]"""
import os
import subprocess
import tempfile

import numpy as np

from tests import ppo_rollout_reference as REF

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
T_MAX = 91
ALIGN = 32
WORLD_NAMES = ("goal_achieved_count", "frac_goal_achieved", "collided_count", "frac_collided", "off_road_count", "frac_off_road",
               "n_rows")
SUMMARY_NAMES = ("goal_achieved", "collided", "off_road", "n_rows")
METRIC_KEYS = ("goal_achieved", "collided", "off_road", "off_road_count", "collided_count", "goal_achieved_count", "frac_off_road",
               "frac_collided", "frac_goal_achieved")


# ---- the owned list
def segment_starts(count):
    start = [0]
    for c in count:
        start.append(-(-(start[-1] + int(c)) // ALIGN) * ALIGN)
    return np.array(start, np.int32)


def owned_list(mask, owner, n_policies, sentinel):
    """rows [n + 32 P] (the sentinel where nothing is written), start [P + 1], count [P]."""
    mask, owner = np.asarray(mask) != 0, np.asarray(owner)
    n = len(mask)
    segs = [np.nonzero(mask & (owner == p))[0] for p in range(n_policies)]
    count = np.array([len(s) for s in segs], np.int32)
    start = segment_starts(count)
    rows = np.full(n + ALIGN * n_policies, sentinel, np.int32)
    for p, s in enumerate(segs):
        rows[start[p]:start[p] + len(s)] = s
        rows[start[p] + len(s):start[p + 1]] = -1
    return rows, start, count


BLOCK, BLOCK_LANES = 1024, 256  # GD_LIVE_ROWS_BLOCK rows to a block; the lanes that add up the blocks' counts


def owned_list_blocks(mask, owner, n_policies, sentinel, wrong=None):
    """owned_list stated by blocks of 1024 rows: per owner the blocks' counts, a block's first position = the counts of the
    blocks before it, the segment's length = the counts of all blocks, a row's position = start + before + its rank among its
    block's rows.  The right rule is owned_list's values.  wrong = 'one_trip': a lane adds the block of its own index only, so
    blocks from 256 on reach neither sum; 'before_le': in a lane's trips after the first (i >= 256) `before` takes the
    blocks i <= block.  Either is the right rule up to 256 blocks.  A position outside the array is dropped, a position
    written twice holds the later row."""
    mask, owner = np.asarray(mask) != 0, np.asarray(owner)
    n = len(mask)
    blocks = -(-n // BLOCK)
    seen = min(blocks, BLOCK_LANES) if wrong == "one_trip" else blocks
    rows = np.full(n + ALIGN * n_policies, sentinel, np.int32)
    idx, cnt, before = [], np.zeros(n_policies, np.int32), []
    for p in range(n_policies):
        i = np.nonzero(mask & (owner == p))[0]
        per_block = np.bincount(i // BLOCK, minlength=blocks)
        per_block_seen = per_block.copy()
        per_block_seen[seen:] = 0
        incl = np.cumsum(per_block_seen)
        idx.append(i)
        cnt[p] = incl[-1]
        excl = incl - per_block_seen
        if wrong == "before_le":
            excl[BLOCK_LANES:] = incl[BLOCK_LANES:]
        before.append(excl)
    start = segment_starts(cnt)
    for p, i in enumerate(idx):
        blk = i // BLOCK
        first = np.searchsorted(blk, blk, side="left")  # the list index of the first row of the row's block
        at = start[p] + before[p][blk] + (np.arange(len(i)) - first)
        ok = at < len(rows)
        rows[at[ok]] = i[ok]
    for p in range(n_policies):  # the last block's padding, after every block's rows
        rows[start[p] + cnt[p]:start[p + 1]] = -1
    return rows, start, cnt


def list_patterns(n, P, rng):
    """The owned-list cases at any n: name -> (mask uint8 [n], owner uint8 [n])."""
    ones = np.ones(n, np.uint8)
    out = {"one-owner": (ones, np.full(n, P - 1, np.uint8)),
           "alternating": (ones, (np.arange(n) % P).astype(np.uint8)),
           "zero-mask": (np.zeros(n, np.uint8), (np.arange(n) % P).astype(np.uint8)),
           "random-with-strangers": ((rng.random(n) < 0.7).astype(np.uint8) * rng.choice([1, 2, 255], n).astype(np.uint8),
                                     rng.integers(0, P + 2, n).astype(np.uint8))}
    out["random-with-strangers"][1][rng.random(n) < 0.05] = 255
    if P >= 3:  # an owner with no rows between two with rows
        gap = (np.arange(n) % 2 * (P - 1)).astype(np.uint8)
        out["gap"] = (ones, gap)
    return out


def many_block_patterns(n, P, rng):
    """The two cases of the lists of more than 256 blocks.  late: every set row of owner P - 1 lies in a block >= 256, every
    set row of another owner in a block < 256 (at 256 blocks owner P - 1 has none).  straddle: owner 0 has set rows in blocks
    255, 256 and the last block only (those of them that exist); with P > 1 the other owners share every row around them, so
    that every start behind owner 0's depends on its count."""
    blocks = -(-n // BLOCK)
    blk = np.arange(n) // BLOCK
    dense = (rng.random(n) < 0.5).astype(np.uint8)
    late_owner = np.where(blk >= BLOCK_LANES, P - 1, rng.integers(0, max(P - 1, 1), n)).astype(np.uint8)
    late_mask = dense.copy()
    if blocks > BLOCK_LANES:  # the first and the last row behind block 255 are set: at 257 blocks that is one row
        late_mask[BLOCK * BLOCK_LANES:][[0, -1]] = 1
    if P == 1:
        late_mask[blk < BLOCK_LANES] = 0
    strad_owner = (rng.integers(1, P, n) if P > 1 else np.zeros(n)).astype(np.uint8)
    strad_mask = dense.copy() if P > 1 else np.zeros(n, np.uint8)
    for b in sorted({min(255, blocks - 1), min(256, blocks - 1), blocks - 1}):
        sel = np.nonzero(blk == b)[0]
        mine = sel[rng.random(len(sel)) < 0.4]
        mine = np.union1d(mine, sel[[0, -1]])  # the block's first and last row among them
        strad_owner[mine], strad_mask[mine] = 0, 1
    return {"late": (late_mask, late_owner), "straddle": (strad_mask, strad_owner)}


OWNER_SIZES = [33, 32, 1, 0, 33, 32, 1, 0]


def owner_patterns(n, P, rng):
    """The forward's cases: name -> (mask bool [n], owner uint8 [n]): segment counts that hit 0, 1, 32 and 33 where n allows."""
    out = {}
    sizes = OWNER_SIZES[:P] if P > 1 else [33]
    for shift in range(P):  # the sizes dealt to the owners in every rotation, in consecutive blocks, the rest dead
        owner, mask, at = np.full(n, 255, np.uint8), np.zeros(n, bool), 0
        for p in range(P):
            k = min(sizes[(p + shift) % P], n - at)
            owner[at:at + k], mask[at:at + k] = p, True
            at += k
        out["blocks%d" % shift] = (mask, owner)
    out["alternating"] = (np.ones(n, bool), (np.arange(n) % P).astype(np.uint8))
    out["one-owner"] = (np.ones(n, bool), np.full(n, P - 1, np.uint8))
    out["random-with-strangers"] = (rng.random(n) < 0.6, rng.integers(0, P + 1, n).astype(np.uint8))
    out["empty"] = (np.zeros(n, bool), np.zeros(n, np.uint8))
    return out


def blob_of_rows(mask, owner, n_policies, wrong=None):
    """[n]: the index of the weights the forward on the owned list gives row i (-1: the row is not listed), read off the list as
    the kernels read it: position q is in segment segments(...)[q] and holds row rows[q].  wrong = 'blob_mod4': a segment's
    weights come from blob[p % 4]."""
    n = len(mask)
    rows, start, count = owned_list(mask, owner, n_policies, -2)
    seg = segments(start[:-1], count, n + ALIGN * n_policies)
    blob = np.full(n, -1, np.int32)
    listed = seg >= 0
    blob[rows[listed]] = seg[listed] % 4 if wrong == "blob_mod4" else seg[listed]
    return blob


def world_counts_by_wave(owner, goal, collided, off_road, n_policies, wrong=None):
    """[P, W, 4] int: per policy and world the rows with goal > 0, collided > 0, off_road > 0 and the rows, counted per wave of
    64 slots and added over the waves.  owner [W, A] (-1: no row).  wrong = 'wave0': only the first wave's counts are added."""
    owner = np.asarray(owner)
    W, A = owner.shape
    waves = 1 if wrong == "wave0" else -(-A // 64)
    out = np.zeros((n_policies, W, 4), np.int64)
    for p in range(n_policies):
        mine = owner == p
        for k, flag in enumerate((np.asarray(goal) > 0, np.asarray(collided) > 0, np.asarray(off_road) > 0, np.ones_like(mine))):
            for v in range(waves):
                out[p, :, k] += (mine & flag)[:, 64 * v:64 * v + 64].sum(1)
    return out


def segments(start, count, limit):
    """segment_of for every position below limit."""
    seg = np.full(limit, -1, np.int32)
    for p, (s, c) in enumerate(zip(start, count)):
        seg[s:s + c] = p
    return seg


# ---- compute_metrics
def compute_metrics(accumulators, denominator):
    """accumulators: per policy a dict of the three [W, A] float32 sums.  multi_policy_rollout.py:158-166 in numpy float32."""
    denominator = np.asarray(denominator, f32)
    out = []
    for acc in accumulators:
        m = dict(acc)
        m["off_road_count"] = (acc["off_road"] > 0).astype(f32).sum(1, dtype=f32)
        m["collided_count"] = (acc["collided"] > 0).astype(f32).sum(1, dtype=f32)
        m["goal_achieved_count"] = (acc["goal_achieved"] > 0).astype(f32).sum(1, dtype=f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            m["frac_off_road"] = (m["off_road_count"] / denominator).astype(f32)
            m["frac_collided"] = (m["collided_count"] / denominator).astype(f32)
            m["frac_goal_achieved"] = (m["goal_achieved_count"] / denominator).astype(f32)
        out.append(m)
    return out


def summary(per_policy, wrong=None):
    """[P, 4]: per policy the totals of goal_achieved_count, collided_count, off_road_count and n_rows in the fixed order.
    wrong = 'first_256': a lane adds the world of its own index only."""
    cut = 256 if wrong == "first_256" else None
    return np.array([[REF.ordered_sum(m["goal_achieved_count"][:cut]), REF.ordered_sum(m["collided_count"][:cut]),
                      REF.ordered_sum(m["off_road_count"][:cut]), REF.ordered_sum(m["n_rows"][:cut])] for m in per_policy], f32)


def metrics(control_mask, masks, done, info):
    """control_mask [W, A] bool, masks: per policy [W, A] bool; done [T, W, A] and info [T, W, A, 5] int32, entry t what is read
    AFTER step t.  Lines 45-57, 59-62, 115-143, 145-149 of the reference.  Returns the per-policy metrics (the nine keys and
    n_rows), live [W, A], episode_lengths, iterations, the denominator and list_count [91, P]."""
    control_mask = np.asarray(control_mask, bool)
    masks = [np.asarray(m, bool) for m in masks]
    done, info = np.asarray(done, np.int32), np.asarray(info, np.int32)
    T, (W, A) = done.shape[0], control_mask.shape
    acc = [dict(goal_achieved=np.zeros((W, A), f32), collided=np.zeros((W, A), f32), off_road=np.zeros((W, A), f32))
           for _ in masks]                                                                                     # :45-52
    episode_lengths = np.zeros(W, f32)                                                                         # :53
    active_worlds = list(range(W))                                                                             # :55
    live = control_mask.copy()                                                                                 # :57
    list_count = np.zeros((T_MAX, len(masks)), np.int32)
    iterations = 0
    for t in range(T):                                                                                         # :59
        iterations += 1
        live_masks = [m & live for m in masks]                                                                 # :62
        list_count[t] = [int(lm.sum()) for lm in live_masks]
        combined = np.zeros_like(live)
        for lm in live_masks:
            combined |= lm
        assert (live == combined).all(), "Live agent mask mismatch!"                                           # :77
        dones = done[t] != 0                                                                                   # :117
        for a, lm in zip(acc, live_masks):                                                                     # :120-123
            a["off_road"][lm] += info[t][..., 0][lm].astype(f32)
            a["collided"][lm] += (info[t][..., 1] + info[t][..., 2])[lm].astype(f32)  # (infos.collided: both kinds)
            a["goal_achieved"][lm] += info[t][..., 3][lm].astype(f32)
        live[dones] = False                                                                                    # :125
        n_done = (dones & control_mask).sum(1)                                                                 # :128-130
        for w in np.nonzero(n_done == control_mask.sum(1))[0]:
            if w in active_worlds:                                                                             # :132-135
                active_worlds.remove(w)
                episode_lengths[w] = t
        if not active_worlds:                                                                                  # :142-143
            break
    denominator = sum(m.sum(1).astype(f32) for m in masks)                                                     # :145
    per_policy = compute_metrics(acc, denominator)                                                             # :149
    for m, mask in zip(per_policy, masks):
        m["n_rows"] = (mask & control_mask).sum(1).astype(f32)
    return dict(policies=per_policy, live=live, episode_lengths=episode_lengths, iterations=iterations, denominator=denominator,
                list_count=list_count, summary=summary(per_policy))


# ---- the host program of csrc/multi_policy_rule.hpp
_HOST = {}


def rule_host(sanitize=False):
    """The compiled host program; sanitize: a second, stand-alone executable with -fsanitize=address,undefined."""
    if sanitize not in _HOST:
        out = os.path.join(tempfile.gettempdir(), "gd_multi_policy_rule_host%s_%d" % ("_san" if sanitize else "", os.getuid()))
        src = os.path.join(HERE, "multi_policy_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "multi_policy_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
            subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out, src])
        _HOST[sanitize] = out
    return _HOST[sanitize]


def _run_host(mode, payload, sanitize):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(payload)
        subprocess.check_call([rule_host(sanitize), mode, fin, fout])
        return open(fout, "rb").read()


def run_starts_host(count, sanitize=False):
    """start [P + 1] and segment_of of every position [sum(count) + 32 P]."""
    count = np.asarray(count, np.int32)
    P = len(count)
    raw = np.frombuffer(_run_host("starts", np.array([P], np.int32).tobytes() + count.tobytes(), sanitize), np.int32)
    assert len(raw) == P + 1 + int(count.sum()) + ALIGN * P
    return raw[:P + 1].copy(), raw[P + 1:].copy()


def run_metrics_host(owner, goal, collided, off_road, denominator, n_policies, sanitize=False):
    """owner [W, A] int32 (-1: no row), the three [W, A] float32 sums over ALL rows, denominator [W].  Returns per policy the
    dict of WORLD_NAMES -> [W], and the summary [P, 4]."""
    owner = np.asarray(owner, np.int32)
    W, A = owner.shape
    payload = np.array([W, A, n_policies], np.int32).tobytes() + owner.tobytes()
    for a in (goal, collided, off_road):
        payload += np.asarray(a, f32).reshape(W, A).tobytes()
    payload += np.asarray(denominator, f32).reshape(W).tobytes()
    raw = np.frombuffer(_run_host("metrics", payload, sanitize), f32)
    assert len(raw) == n_policies * 7 * W + n_policies * 4
    world = raw[:n_policies * 7 * W].reshape(n_policies, 7, W)
    return ([dict(zip(WORLD_NAMES, (world[p, j].copy() for j in range(7)))) for p in range(n_policies)],
            raw[n_policies * 7 * W:].reshape(n_policies, 4).copy())


# ---- the whole loop over a simulator
def closed_loop(sim, policies, table, n_steps=T_MAX, deterministic=False, u=None, init_steps=0, reward_weights=None):
    """multi_policy_rollout.py:36-169 on `sim`, a SimManager.  policies: a dict name -> (`DevicePolicy`, mask [W, A] bool), each
    policy called once per step on next_obs[mask_p & live] as the reference calls its networks, with the draws of those rows
    from u [n_steps, N] (N: the controlled agents in row-major order).  Returns what `ppo_rollout_reference.closed_loop`
    returns over all rows (the policies own disjoint agents, so the accumulators over all rows are the sums of theirs), and
    "policies": name -> the reference's nine keys (device tensors) and n_rows [W]; "policy_summary" [P, 4] numpy;
    "denominator" [W]; "list_count" [91, P]."""
    import torch
    W, A, dev = sim._W, sim._A, sim._device
    policies = {k: (fn, m.to(dev)) for k, (fn, m) in policies.items()}

    def get_obs():
        return sim.packed_observations(reward_weights=reward_weights).clone()

    sim.reset(list(range(W)))                                                      # :44 (env.reset ...
    if init_steps > 0:
        sim.advance_log_playback(init_steps)                                       # ... advances the log playback)
    next_obs = get_obs()
    policy_metrics = {name: {k: torch.zeros((W, A), device=dev) for k in ("goal_achieved", "collided", "off_road")}
                      for name in policies}                                        # :45-52
    episode_lengths = torch.zeros(W)                                               # :53
    active_worlds = list(range(W))                                                 # :55
    control_mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1       # :56
    live_agent_mask = control_mask.clone()                                         # :57
    N = int(control_mask.sum())
    rec = dict(actions_idx=torch.full((N, T_MAX), -1, dtype=torch.int64, device=dev),
               live_mask=torch.zeros((N, T_MAX), dtype=torch.bool, device=dev),
               agent_positions=torch.zeros((W, A, T_MAX, 2), device=dev))
    list_count = torch.zeros((T_MAX, len(policies)), dtype=torch.int32)
    any_active = torch.zeros(T_MAX + 1, dtype=torch.int32)
    any_active[0] = 1
    iterations = 0
    last_live = live_agent_mask.clone()
    for time_step in range(n_steps):                                               # :59
        iterations += 1
        rows = live_agent_mask[control_mask]
        rec["live_mask"][:, time_step] = rows
        last_live = live_agent_mask.clone()
        policy_live_masks = {name: mask & live_agent_mask for name, (fn, mask) in policies.items()}   # :62
        actions = {}
        for p, (name, (fn, mask)) in enumerate(policies.items()):                  # :66-71
            live_mask = policy_live_masks[name]
            list_count[time_step, p] = int(live_mask.sum())
            if live_mask.any():
                obs = next_obs[live_mask].contiguous()
                if deterministic:
                    actions[name] = fn(obs, deterministic=True)[0]
                else:
                    actions[name] = fn(obs, u[time_step][live_mask[control_mask]].contiguous())[0]
        combined_mask = torch.zeros_like(live_agent_mask, dtype=torch.bool)        # :74-77
        for live_mask in policy_live_masks.values():
            combined_mask |= live_mask
        assert torch.all(live_agent_mask == combined_mask), "Live agent mask mismatch!"
        action_template = torch.zeros((W, A), dtype=torch.int64, device=dev)       # :79
        for name, action in actions.items():                                       # :82-85
            live_mask = policy_live_masks[name]
            if action.numel() > 0:
                action_template[live_mask] = action.to(dtype=action_template.dtype, device=dev)
        rec["actions_idx"][:, time_step] = torch.where(rows, action_template[control_mask], -1)
        sim.action_tensor().to_torch()[:, :, :3] = table[action_template]          # :88 (step_dynamics decodes the indices)
        sim.step()
        next_obs = get_obs()                                                       # :116-118
        dones = sim.done_tensor().to_torch().reshape(W, A).bool()
        info = sim.info_tensor().to_torch().reshape(W, A, 5)
        for name, live_mask in policy_live_masks.items():                          # :120-123
            policy_metrics[name]["off_road"][live_mask] += info[..., 0][live_mask].float()
            policy_metrics[name]["collided"][live_mask] += (info[..., 1] + info[..., 2])[live_mask].float()
            policy_metrics[name]["goal_achieved"][live_mask] += info[..., 3][live_mask].float()
        live_agent_mask[dones] = False                                             # :125
        num_dones_per_world = (dones & control_mask).sum(dim=1)                    # :128-130
        total_controlled_agents = control_mask.sum(dim=1)
        done_worlds = (num_dones_per_world == total_controlled_agents).nonzero(as_tuple=True)[0]
        for world in done_worlds.tolist():                                         # :132-135
            if world in active_worlds:
                active_worlds.remove(world)
                episode_lengths[world] = time_step
        pos = sim.absolute_self_observation_tensor().to_torch()                    # :137-140
        rec["agent_positions"][:, :, time_step, 0] = pos[..., 0]
        rec["agent_positions"][:, :, time_step, 1] = pos[..., 1]
        if not active_worlds:                                                      # :142-143
            break
        any_active[time_step + 1] = 1
    controlled_per_scene = sum(mask.sum(dim=1).float() for name, (fn, mask) in policies.items())   # :145
    for name in policies:                                                          # :158-166
        m = policy_metrics[name]
        m["off_road_count"] = (m["off_road"] > 0).float().sum(axis=1)
        m["collided_count"] = (m["collided"] > 0).float().sum(axis=1)
        m["goal_achieved_count"] = (m["goal_achieved"] > 0).float().sum(axis=1)
        m["frac_off_road"] = m["off_road_count"] / controlled_per_scene
        m["frac_collided"] = m["collided_count"] / controlled_per_scene
        m["frac_goal_achieved"] = m["goal_achieved_count"] / controlled_per_scene
        m["n_rows"] = (policies[name][1] & control_mask).sum(dim=1).float()

    # over all rows, as examples/experimental/eval_utils.py:190-212 (ppo_rollout_reference.closed_loop)
    goal_achieved = sum(policy_metrics[name]["goal_achieved"] for name in policies)
    collided = sum(policy_metrics[name]["collided"] for name in policies)
    off_road = sum(policy_metrics[name]["off_road"] for name in policies)
    controlled = control_mask.sum(dim=1).float()
    goal_achieved_count = (goal_achieved > 0).float().sum(axis=1)
    collided_count = (collided > 0).float().sum(axis=1)
    off_road_count = (off_road > 0).float().sum(axis=1)
    other_count = torch.logical_and(goal_achieved == 0, torch.logical_and(collided == 0, torch.logical_and(
        off_road == 0, control_mask))).float().sum(dim=1)
    out = dict(goal_achieved_count=goal_achieved_count, frac_goal_achieved=goal_achieved_count / controlled,
               collided_count=collided_count, frac_collided=collided_count / controlled,
               off_road_count=off_road_count, frac_off_road=off_road_count / controlled,
               other_count=other_count, frac_other=other_count / controlled,
               controlled_per_scene=controlled, episode_lengths=episode_lengths.to(dev),
               goal_achieved=goal_achieved[control_mask], collided=collided[control_mask], off_road=off_road[control_mask],
               live=live_agent_mask[control_mask], last_live=last_live, control_mask=control_mask,
               any_active=any_active.to(dev), iterations=iterations, policies=policy_metrics, denominator=controlled_per_scene,
               list_count=list_count.to(dev), **rec)
    world = {k: out[k].cpu().numpy() for k in REF.WORLD_NAMES}
    out["summary"] = REF.summary(world, episode_lengths.numpy(), any_active.numpy(), n_steps)
    out["policy_summary"] = summary([{k: v.cpu().numpy() for k, v in policy_metrics[name].items()} for name in policies])
    return out
