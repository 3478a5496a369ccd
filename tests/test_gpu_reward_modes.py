"""GPU suite: the reward types "reward_conditioned" and "distance_to_logs" of the device episode loop (csrc/episode.hip) and
the conditioned packed observation (csrc/pack_obs.hip), through EpisodeTracker / SimManager -> ctypes -> the C ABI.
References: gpudrive/env/env_torch.py:247-401, 469-603, 756-810; gpudrive/env/env_puffer.py:250-403."""
import numpy as np
import pytest
import torch

from tests import parity as P
from tests.conftest import SCENE_4, SCENE_407, TEST_JSON
from tests.test_reward_modes import draw_weights_np

pytestmark = pytest.mark.gpu

KW = dict(polylineReductionThreshold=0.1, observationRadius=50.0, collisionBehaviour=0, rewardType=1,
          distanceToGoalThreshold=2.0, dynamicsModel=0, maxNumControlledAgents=3, isStaticAgentControlled=0,
          initOnlyValidAgentsAtFirstStep=0, IgnoreNonVehicles=0)
SCENES = [SCENE_4, SCENE_407, TEST_JSON, SCENE_4]
WEIGHTS = (-0.75, 1.0, -0.5)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _actions(rng, W, A):
    act = P.random_actions(rng, W, A, 0)
    act[..., 0] = np.abs(act[..., 0])  # accelerate: collisions, goals and off-road events all happen
    return act


def _lockstep_tracker(oracle_mod, steps, reward_type, gt_kw, check_reward, expert=False, seed=5):
    """Drive an EpisodeTracker and the oracle's weighted tracker on the same actions; `check_reward(g_rew, o_rew, t0, orc, gt,
    ot)` compares the rewards and returns what the tracker adds to the oracle's weighted reward (None: nothing); everything
    else is compared bit for bit here, the returns within 1e-5 where a term was added."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    from oracle.episode import OracleEpisodeTracker
    gpu = P.make_gpu_sim(SCENES, max_agents=64, **KW)
    orc = P.make_oracle_sim(oracle_mod, SCENES, max_agents=64, **KW)
    gt = EpisodeTracker(gpu, *WEIGHTS, reward_type=reward_type, **gt_kw)
    ot = OracleEpisodeTracker(orc, *WEIGHTS)
    rewards_of = ot.get_rewards

    def rewards_and_positions():  # the positions the rewards see: after the step, before the oracle resets finished worlds
        ot.pos_before_reset = np.array(orc.absolute_self_observation_tensor())[..., :2].copy()
        return rewards_of()
    ot.get_rewards = rewards_and_positions
    rng = np.random.default_rng(seed)
    exp_act = orc.expert_actions()[0] if expert else None
    finished = np.zeros(orc.W, np.int64)
    exact = ["collided_in_episode", "offroad_in_episode", "episode_lengths"]
    extra_ret = np.zeros((orc.W, orc.A))  # float64 sums of the added terms over each episode
    for k in range(steps):
        t0 = np.clip(ot.episode_lengths[:, 0].astype(np.int64), 0, 90)  # before the step (env_puffer.py:251-256)
        if expert:
            act = np.zeros((orc.W, orc.A, 10), np.float32)
            act[..., :3] = exp_act[np.arange(orc.W), :, t0]
        else:
            act = _actions(rng, orc.W, orc.A)
        P.write_actions(gpu, act)
        np.copyto(orc.action_tensor(), act)
        o_rew, o_term, o_trunc, o_mask, o_done = ot.step()
        g_rew, g_term, g_trunc, g_mask = [t.cpu().numpy() for t in gt.step()]
        try:
            extra = check_reward(g_rew, o_rew, t0, orc, gt, ot)
            assert np.array_equal(g_term, o_term) and np.array_equal(g_trunc, o_trunc) and np.array_equal(g_mask, o_mask)
            assert np.array_equal(gt.done_worlds.cpu().numpy(), o_done), "done worlds"
            for n in exact:
                assert np.array_equal(bits(getattr(gt, n).cpu().numpy()), bits(getattr(ot, n))), n
            assert np.array_equal(gt.live_agent_mask.cpu().numpy(), ot.live_agent_mask)
            done = np.flatnonzero(o_done)
            finished[done] += 1
            if extra is not None:
                extra_ret[o_mask] += extra[o_mask]
                ws, ows = gt.world_stats.cpu().numpy()[done], ot.world_stats[done]
                cols = [c for c in range(ws.shape[1]) if c != 2]  # 2: the return sum
                assert np.array_equal(bits(ws[:, cols]), bits(ows[:, cols])), "episode statistics"
                want_sum = ows[:, 2] + np.where(ot.controlled_agent_mask[done], extra_ret[done], 0.0).sum(axis=1)
                np.testing.assert_allclose(ws[:, 2], want_sum, rtol=0, atol=1e-4, err_msg="return sums")
                extra_ret[done] = 0.0
                np.testing.assert_allclose(gt.agent_episode_returns.cpu().numpy(), ot.agent_episode_returns + extra_ret,
                                           rtol=0, atol=1e-5, err_msg="returns")
            else:
                assert np.array_equal(bits(gt.agent_episode_returns.cpu().numpy()), bits(ot.agent_episode_returns))
                assert np.array_equal(bits(gt.world_stats.cpu().numpy()[done]), bits(ot.world_stats[done])), "statistics"
            P.compare_ints(gpu, orc, ["done_tensor", "info_tensor", "steps_remaining_tensor"])
            P.compare_state(gpu, orc)
            P.inject_and_compare(gpu, orc)
        except AssertionError as e:
            raise AssertionError("step %d: %s" % (k + 1, e))
    assert (finished >= 2).all(), finished
    gpu.close()
    return gt


def test_conditioned_fixed_equals_the_weighted_combination(oracle_mod):
    """reward_conditioned with fixed weights (cw, gw, ow) is bit for bit the weighted combination with those weights, over
    200 steps with device-driven resets (every reset world redraws the same fixed weights)."""
    def check(g_rew, o_rew, t0, orc, gt, ot):
        assert np.array_equal(bits(g_rew), bits(o_rew)), "rewards"
    gt = _lockstep_tracker(oracle_mod, 200, "reward_conditioned",
                           dict(condition_mode="fixed", agent_type=torch.tensor(WEIGHTS)), check)
    wt = gt.reward_weights_tensor.cpu().numpy()
    assert np.array_equal(bits(wt), bits(np.broadcast_to(np.asarray(WEIGHTS, np.float32), wt.shape)))
    assert (gt.weight_draws.cpu().numpy() >= 3).all()  # draw 0 + one per episode end


@pytest.mark.parametrize("expert", [True, False], ids=["expert_actions", "random_actions"])
def test_distance_to_logs_against_the_oracle(oracle_mod, expert):
    """distance_to_logs = the weighted combination + 0.01 exp(-|log_pos[t] - pos|), t = episode_lengths[:, 0] before the
    step; the distance term restated in float64 from the oracle's tensors."""
    dists = []

    def check(g_rew, o_rew, t0, orc, gt, ot):
        W, A = g_rew.shape
        pos = ot.pos_before_reset.astype(np.float64)
        log = np.array(orc.expert_trajectory_tensor())[..., :2 * 91].reshape(W, A, 91, 2)[np.arange(W), :, t0]
        d = np.linalg.norm(log.astype(np.float64) - pos, axis=-1)
        dists.append(np.median(d[ot.controlled_agent_mask]))
        want = o_rew.astype(np.float64) + 0.01 * np.exp(-d)
        np.testing.assert_allclose(g_rew, want, rtol=0, atol=1e-6, err_msg="rewards")
        return 0.01 * np.exp(-d)
    _lockstep_tracker(oracle_mod, 200, "distance_to_logs", {}, check, expert=expert)
    if expert:  # the logs' own actions start the agents on the logged path (one step ahead of log_pos[t]: t lags by one)
        assert dists[0] < 1.0, dists[0]


def test_conditioned_random_draws(oracle_mod):
    """random: draw 0 of every world at construction, draw k + 1 of exactly the worlds that finished, each step's reward the
    conditioned sum of info and the weights it was computed with; then an explicit preset for two worlds."""
    from gpudrive_lab_amd.episode import EpisodeTracker, resolve_condition
    seed = 1234
    gpu = P.make_gpu_sim(SCENES, max_agents=64, **KW)
    W, A = len(SCENES), 64
    gt = EpisodeTracker(gpu, reward_type="reward_conditioned", condition_mode="random", seed=seed)
    draws = np.zeros(W, np.int64)
    want = np.stack([draw_weights_np(seed, w, 0, A) for w in range(W)])
    assert np.array_equal(bits(gt.reward_weights_tensor.cpu().numpy()), bits(want))
    assert np.array_equal(gt.weight_draws.cpu().numpy(), draws + 1)
    draws += 1
    rng = np.random.default_rng(8)
    ends = 0
    for k in range(200):
        before = gt.reward_weights_tensor.cpu().numpy().copy()
        P.write_actions(gpu, _actions(rng, W, A))
        gpu.step()
        info = gpu.info_tensor().to_torch().cpu().numpy()  # what the rewards see, before the reset pass
        g_rew = gt.step(step_sim=False)[0].cpu().numpy()
        off, col, goal = info[..., 0].astype(np.float32), info[..., 1:3].astype(np.float32).sum(-1), info[..., 3].astype(np.float32)
        rew = (before[..., 0] * col + before[..., 1] * goal) + before[..., 2] * off
        assert np.array_equal(bits(g_rew), bits(rew)), "step %d: rewards" % (k + 1)
        done = gt.done_worlds.cpu().numpy() != 0
        after = gt.reward_weights_tensor.cpu().numpy()
        for w in range(W):
            if done[w]:
                assert np.array_equal(bits(after[w]), bits(draw_weights_np(seed, w, int(draws[w]), A))), (k + 1, w)
                draws[w] += 1
                ends += 1
            else:
                assert np.array_equal(bits(after[w]), bits(before[w])), (k + 1, w)
        assert np.array_equal(gt.weight_draws.cpu().numpy(), draws)
    assert ends >= 2 * W
    before = gt.reward_weights_tensor.cpu().numpy().copy()
    gt.set_reward_weights(worlds=[0, 2], condition_mode="preset", agent_type="risk_taker")
    after = gt.reward_weights_tensor.cpu().numpy()
    rt = resolve_condition("preset", "risk_taker")[1]
    for w in range(W):
        exp = np.broadcast_to(rt, (A, 3)) if w in (0, 2) else before[w]
        assert np.array_equal(bits(after[w]), bits(exp)), w
    with pytest.raises(ValueError):
        gt.set_reward_weights(condition_mode="preset", agent_type="timid")
    with pytest.raises(ValueError):
        gt.set_reward_weights(worlds=[W])
    assert np.array_equal(bits(gt.reward_weights_tensor.cpu().numpy()), bits(after))  # nothing reached the device
    gpu.close()


@pytest.mark.parametrize("direct", [False, True], ids=["second_pass", "direct_only"])
@pytest.mark.parametrize("A", [64, 128])
def test_conditioned_pack(A, direct):
    """packed_observations(reward_weights=W) == cat(P[..., :6], W, P[..., 6:]) bit for bit, P the unconditioned pack of the
    same state, from the raw tensors and from the attached direct-pack buffer; at the step that auto-resets a world its
    new weights are in its rows; nothing is written past out_bytes."""
    from gpudrive_lab_amd.episode import EpisodeTracker
    gpu = P.make_gpu_sim(SCENES, max_agents=A, **dict(KW, maxNumControlledAgents=A))
    W = len(SCENES)
    D = 6 + (A - 1) * 6 + 200 * 13
    if direct:
        assert gpu.direct_pack(only=True)
    gt = EpisodeTracker(gpu, reward_type="reward_conditioned", seed=A)
    wt = gt.reward_weights_tensor
    n = W * A * (D + 3)
    guard = torch.empty(n + 67, dtype=torch.float32, device=wt.device)
    guard.view(torch.int32).fill_(0x7FC0BEEF)
    rng = np.random.default_rng(A)

    def check(what):
        base = gpu.packed_observations().clone()
        got = gpu.packed_observations(reward_weights=wt).clone()
        want = torch.cat([base[..., :6], wt, base[..., 6:]], -1)
        assert got.shape == (W, A, D + 3)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what
        g = gpu.packed_observations(out=guard, reward_weights=wt)
        assert torch.equal(g.view(torch.int32), want.view(torch.int32)), what + " (caller's buffer)"
        tail = guard[n:].view(torch.int32).cpu()
        assert (tail == 0x7FC0BEEF).all(), what + ": written past out_bytes"

    check("fresh")
    reset_seen = False
    for k in range(100):
        before = wt.clone()
        P.write_actions(gpu, _actions(rng, W, A))
        gt.step()
        done = gt.done_worlds.cpu().numpy() != 0
        if k < 2 or done.any():
            check("step %d" % (k + 1))
        if done.any():
            changed = (wt != before).flatten(1).any(1).cpu().numpy()
            assert np.array_equal(changed, done)
            reset_seen = True
            break
    assert reset_seen
    gpu.close()
