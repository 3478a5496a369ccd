"""Float64 statement of one simulator step outside collision detection, written from its definition, numpy only.

It reads two snapshots (`snapshot`) of the tensors every simulator exports -- one taken before a pass, one after it -- and
states what the pass must leave for every live agent slot: position, yaw, velocity, the action tensor, reward, steps
remaining, done, info[3], self-observation columns 0-7 and the absolute row.  The float32 inputs are taken as exact, so the
same function checks the oracle on the CPU and the kernel on the GPU.  Collision DETECTION is tests/collision_reference.py's:
the collided flag the pass leaves is read from the `after` snapshot and only copied into the self row.

The rule, in the order the reference runs it (task graph src/sim.cpp:785-889: movement, detection, reward, step counter, done,
then the observation rows):

  movement (src/sim.cpp:294-383), skipped on a reset pass
    * an agent whose collided flag is set: AgentStop marks it done and zeroes its velocity; AgentRemoved does the same and
      puts it at the padding position (-11000, -11000, FLT_MAX; src/consts.hpp:64); Ignore forgets the flag (:302-323);
    * a Static agent is left alone after that (:327-331);
    * a done agent that is not Static goes to the padding position with zero velocity (:333-343);
    * a controlled agent is moved by the dynamics model (:345-369), anybody else is put on its log at index
      episodeLen - steps_remaining: x, y, velocity and heading from the log, z = 1, vz = 0 (:23-25, :370-382).
  dynamics (src/dynamics.hpp), dt = 0.1, speed = |(vx, vy, vz)|, yaw = the heading of the stored rotation
    * Classic (:11-50): v = speed + a dt / 2 (the mean speed of the step), beta = atan(tan(steer) / 2), the position moves by
      v dt along yaw + beta, the yaw by v cos(beta) tan(steer) / length * dt, z = 1, and the velocity is
      (speed + a dt) along the NEW yaw, vz = 0;
    * InvertibleBicycle (:52-81): a is clamped to +-6 and steer to +-3 IN THE ACTION TENSOR; the position moves by
      velocity * dt + a / 2 * dt^2 along yaw, the yaw by steer * (speed dt + a dt^2 / 2), the velocity is (speed + a dt)
      along the new yaw, vz = 0; z stays;
    * DeltaLocal (:83-115): (dx, dy) turned by +yaw is added to the position, the velocity is that over dt, vz = 0, the
      yaw moves by dyaw; z stays;
    * State (:186-194): position, yaw and velocity are the action's columns 0-2, 3, 4-6.
    Every new yaw is wrapped into [-pi, pi] (src/utils.hpp AngleAdd).
  reward (:560-587): -dist to the goal, or (dist < threshold) as 1 / 0;
  step counter (:589-592): one less, on a step pass only;
  done (:597-626): at steps == episodeLen an agent that is not done returns at once; at steps == 0 it is done; then, UNLESS
    it is done AND has reached its goal already, dist < threshold sets done and info[3];
  rows (:168-186, :769-783): speed, the three sizes, the goal offset turned into the agent's frame, collided, id; position,
    rotation, heading angle, goal, sizes, id.

MARGIN.  The one verdict float32 rounding can turn is dist < threshold.  An agent with |dist - threshold| < band is marginal:
its reward (when it is the 1 / 0 kind), done and info[3] are not compared.  Two exceptions need no margin: with a threshold
<= 0 the verdict is false for every dist >= 0 in any arithmetic; and an agent whose offset to the goal has one component
exactly 0 has dist = |the other component| exactly in any IEEE arithmetic (sqrt(fl(x * x)) = |x|), so an agent standing
exactly on the threshold along an axis is compared.

`variant=` breaks one rule (VARIANTS); only the CPU suite uses it, to show that the constructed worlds tell the rules apart."""
import numpy as np

from tests import collision_reference as CR
from tests import geom_reference as GR

f64 = np.float64
PI = float(np.pi)
DT = 0.1
EPISODE = CR.EPISODE
PAD_XY = -11000.0
PAD_Z = float(CR.PAD_Z)
CLASSIC, BICYCLE, DELTA, STATE = range(4)             # DynamicsModel, src/init.hpp:97-103
DISTANCE_BASED, ON_GOAL = 0, 1                        # RewardType, src/init.hpp:76-81
TRAJ_POS, TRAJ_VEL, TRAJ_HEAD, TRAJ_VALID = 0, 2 * EPISODE, 4 * EPISODE, 5 * EPISODE   # Trajectory, src/types.hpp:348-354

VARIANTS = ("mean_is_end_speed", "beta_without_half", "no_wrap", "width_for_length", "no_clamp", "delta_minus_yaw",
            "log_off_by_one", "le_threshold", "reward_sign", "decrement_after_done", "no_reach_when_done", "static_padded")


def snapshot(sim):
    """Copies of every tensor the reference reads or states, from the oracle or the HIP simulator."""
    state = sim.get_state() if hasattr(sim, "get_state") else sim.debug_get_state()
    g = GR._np
    return dict(shape=g(sim.shape_tensor()).copy(), state=np.array(state, np.float32),
                abs_obs=g(sim.absolute_self_observation_tensor()).copy(), self_obs=g(sim.self_observation_tensor()).copy(),
                info=g(sim.info_tensor()).copy(), controlled=g(sim.controlled_state_tensor())[..., 0].copy(),
                resp=g(sim.response_type_tensor())[..., 0].copy(), done=g(sim.done_tensor())[..., 0].copy(),
                steps=g(sim.steps_remaining_tensor())[..., 0].astype(np.int64), action=g(sim.action_tensor()).copy(),
                reward=g(sim.reward_tensor())[..., 0].copy(), traj=g(sim.expert_trajectory_tensor()).copy())


def wrap(a):
    """src/utils.hpp NormalizeAngle: the remainder of a / 2 pi, brought into [-pi, pi]."""
    r = np.fmod(np.asarray(a, f64), 2 * PI)
    return np.where(r > PI, r - 2 * PI, np.where(r < -PI, r + 2 * PI, r))


def angular_distance(a, b):
    """|a - b| modulo 2 pi: a rotation q and -q, or a sum that lands on either side of the seam, are the same heading."""
    d = np.fmod(np.abs(np.asarray(a, f64) - np.asarray(b, f64)), 2 * PI)
    return np.minimum(d, 2 * PI - d)


def step_reference(before, after, w, model, behaviour, reward_type, threshold, band, reset_pass=False, variant=None):
    """World w.  before / after: snapshots around the pass.  Returns a dict over the n live agents: x, y, z, yaw, vel [n, 3],
    action [n, 10], reward, steps, done, reached, self_obs [n, 8], abs_pos / abs_goal / abs_size / abs_id, margin [n], padded
    [n], and the intermediate values the cases' premises read: speed0, v_mean, v_end, yaw0, yaw_sum (the new yaw before the
    wrap), along (the velocity's component along the old heading), dist, log_index, driven, replayed."""
    assert variant is None or variant in VARIANTS, variant
    n = int(before["shape"][w, 0])
    st = before["state"][w, :n].astype(f64)
    x, y, z = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy()
    yaw0 = GR.yaw_of(st[:, 3:7])
    vel = st[:, 7:10].copy()
    hit0 = st[:, 10] != 0
    done = before["done"][w, :n] == 1
    reached = before["info"][w, :n, 3] == 1
    steps0 = before["steps"][w, :n]
    ctl = before["controlled"][w, :n] != 0
    static = before["resp"][w, :n] == CR.RESP_STATIC
    ab = before["abs_obs"][w, :n].astype(f64)
    gx, gy, length, width = ab[:, 8], ab[:, 9], ab[:, 10], ab[:, 11]
    act = before["action"][w, :n].astype(f64)
    act_out = act.copy()
    yaw, yaw_sum = yaw0.copy(), yaw0.copy()
    speed0 = np.sqrt((vel ** 2).sum(-1))
    along = vel[:, 0] * np.cos(yaw0) + vel[:, 1] * np.sin(yaw0)
    v_mean, v_end = speed0.copy(), speed0.copy()
    driven, replayed = np.zeros(n, bool), np.zeros(n, bool)
    log_index = np.clip(EPISODE - steps0, 0, EPISODE - 1)

    if not reset_pass:
        if behaviour != CR.IGNORE:                                     # src/sim.cpp:302-313
            done = done | hit0
            vel[hit0] = 0
            if behaviour == CR.AGENT_REMOVED:
                x[hit0], y[hit0], z[hit0] = PAD_XY, PAD_XY, PAD_Z
        gone = done & ~static if variant != "static_padded" else done  # :327-343
        x[gone], y[gone], z[gone] = PAD_XY, PAD_XY, PAD_Z
        vel[gone] = 0
        driven = ctl & ~static & ~gone
        replayed = ~ctl & ~static & ~gone
        d = driven
        a, steer = act[:, 0].copy(), act[:, 1].copy()
        if model == CLASSIC:                                           # src/dynamics.hpp:11-50
            v_end = speed0 + a * DT
            v_mean = speed0 + 0.5 * a * DT if variant != "mean_is_end_speed" else v_end
            tan_d = np.tan(steer)
            beta = np.arctan(0.5 * tan_d) if variant != "beta_without_half" else np.arctan(tan_d)
            rate = v_mean * np.cos(beta) * tan_d / (length if variant != "width_for_length" else width)
            yaw_sum = np.where(d, yaw0 + rate * DT, yaw0)
            new_yaw = wrap(yaw_sum) if variant != "no_wrap" else yaw_sum
            x = np.where(d, x + v_mean * np.cos(yaw0 + beta) * DT, x)
            y = np.where(d, y + v_mean * np.sin(yaw0 + beta) * DT, y)
            z = np.where(d, 1.0, z)
            vel[d] = np.stack([v_end * np.cos(new_yaw), v_end * np.sin(new_yaw), 0 * v_end], -1)[d]
            yaw = np.where(d, new_yaw, yaw)
        elif model == BICYCLE:                                         # :52-81
            if variant != "no_clamp":
                a, steer = np.clip(a, -6.0, 6.0), np.clip(steer, -3.0, 3.0)
            act_out[d, 0], act_out[d, 1] = a[d], steer[d]
            v_end = speed0 + a * DT
            v_mean = speed0 + 0.5 * a * DT
            yaw_sum = np.where(d, yaw0 + steer * (speed0 * DT + 0.5 * a * DT * DT), yaw0)
            new_yaw = wrap(yaw_sum) if variant != "no_wrap" else yaw_sum
            x = np.where(d, x + vel[:, 0] * DT + 0.5 * a * np.cos(yaw0) * DT * DT, x)
            y = np.where(d, y + vel[:, 1] * DT + 0.5 * a * np.sin(yaw0) * DT * DT, y)
            vel[d] = np.stack([v_end * np.cos(new_yaw), v_end * np.sin(new_yaw), 0 * v_end], -1)[d]
            yaw = np.where(d, new_yaw, yaw)
        elif model == DELTA:                                           # :83-115
            turn = yaw0 if variant != "delta_minus_yaw" else -yaw0
            dx = act[:, 0] * np.cos(turn) - act[:, 1] * np.sin(turn)
            dy = act[:, 0] * np.sin(turn) + act[:, 1] * np.cos(turn)
            yaw_sum = np.where(d, yaw0 + act[:, 2], yaw0)
            new_yaw = wrap(yaw_sum) if variant != "no_wrap" else yaw_sum
            x, y = np.where(d, x + dx, x), np.where(d, y + dy, y)
            vel[d] = np.stack([dx / DT, dy / DT, 0 * dx], -1)[d]
            yaw = np.where(d, new_yaw, yaw)
        else:                                                          # :186-194
            x, y, z = np.where(d, act[:, 0], x), np.where(d, act[:, 1], y), np.where(d, act[:, 2], z)
            yaw_sum = np.where(d, act[:, 3], yaw0)
            yaw = yaw_sum.copy()
            vel[d] = act[d, 4:7]
        r = replayed                                                   # src/sim.cpp:23-25, 370-382
        k = log_index if variant != "log_off_by_one" else np.clip(log_index + 1, 0, EPISODE - 1)
        tr = before["traj"][w, :n].astype(f64)
        rows = np.arange(n)
        x, y = np.where(r, tr[rows, TRAJ_POS + 2 * k], x), np.where(r, tr[rows, TRAJ_POS + 2 * k + 1], y)
        z = np.where(r, 1.0, z)
        vel[r] = np.stack([tr[rows, TRAJ_VEL + 2 * k], tr[rows, TRAJ_VEL + 2 * k + 1], 0 * x], -1)[r]
        yaw = np.where(r, tr[rows, TRAJ_HEAD + k], yaw)
        yaw_sum = np.where(r, yaw, yaw_sum)

    dist = np.hypot(x - gx, y - gy)                                    # src/sim.cpp:560-587
    inside = dist < threshold if variant != "le_threshold" else dist <= threshold
    reward = -dist if reward_type == DISTANCE_BASED else inside.astype(f64)
    if variant == "reward_sign":
        reward = -reward
    steps = steps0 - (0 if reset_pass else 1)                          # :589-592
    seen = steps if variant != "decrement_after_done" else steps0      # :597-626
    early = (seen == EPISODE) & ~done
    done_out = done | (~early & (seen == 0))
    looked = ~early & (~done_out | ~reached if variant != "no_reach_when_done" else ~done_out)
    arrive = looked & inside
    done_out, reached_out = done_out | arrive, reached | arrive
    on_axis = ((x == gx) | (y == gy)) & (dist == threshold)
    margin = (np.abs(dist - threshold) < band) & ~on_axis if threshold > 0 else np.zeros(n, bool)

    c, s = np.cos(yaw), np.sin(yaw)                                    # :168-186
    collided = after["state"][w, :n, 10] != 0
    self_obs = np.stack([np.sqrt((vel ** 2).sum(-1)), ab[:, 10], ab[:, 11], ab[:, 12], c * (gx - x) + s * (gy - y),
                         -s * (gx - x) + c * (gy - y), collided.astype(f64), ab[:, 13]], -1)
    return dict(x=x, y=y, z=z, yaw=yaw, vel=vel, action=act_out, reward=reward, steps=steps, done=done_out, reached=reached_out,
                self_obs=self_obs, abs_goal=ab[:, 8:10], abs_size=ab[:, 10:13], abs_id=ab[:, 13], margin=margin, padded=z == PAD_Z,
                speed0=speed0, v_mean=v_mean, v_end=v_end, yaw0=yaw0, yaw_sum=yaw_sum, along=along, dist=dist, log_index=log_index,
                driven=driven, replayed=replayed, static=static, controlled=ctl, inside=inside, early=early)
