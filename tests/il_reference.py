"""The reference's imitation-learning recorder, restated on the call-sequence harness: `save_trajectory` of
gpudrive/integrations/il/storage.py:17-98 statement for statement, its per-index Python loop included (slow on purpose: it
is the yardstick, not the product).  It uses nothing but `TorchCallSequence`, which the reference's goldens pin, and never
imports the recorder.

Differences from the reference, all outside the arithmetic:
  - `mask` stands where `env.cont_agent_mask` does (default: the harness's own),
  - the partner mask has max_agent_count - 1 columns where the reference writes its fork's 127 as a literal,
  - one hook, `get_obs`, for where the observation comes from.  `h.get_obs()` is also what refreshes the harness's partner
    mask; with another source the loop calls `h.make_partner_mask` on that observation's partner columns itself,
  - nothing is printed or written: the arrays are returned (before the `~collision` filter, with `collision` beside them),
    together with the number of iterations run.  The reference leaves `collision` undefined when its loop never breaks (a
    NameError there); here it is then computed after the loop by the same expression."""
import torch


def save_trajectory(h, mask=None, get_obs=None):
    A = h.max_agent_count
    own = get_obs is None

    def observe():
        if own:
            o = h.get_obs()
            return o, h.get_partner_mask()
        o = get_obs()
        return o, h.make_partner_mask(o[..., 6:6 + (A - 1) * 6]).clone()

    obs = h.reset()
    expert_actions, _, _, _, _ = h.get_expert_actions()  # (num_worlds, num_agents, episode_len, action_dim)
    road_mask = h.get_road_mask()
    partner_mask = h.get_partner_mask()
    if not own:
        obs, partner_mask = observe()
    device = h.device

    env_cont_agent_mask = h.cont_agent_mask if mask is None else mask
    cont_agent_mask = env_cont_agent_mask.to(device)  # (num_worlds, num_agents)
    alive_agent_indices = cont_agent_mask.nonzero(as_tuple=False)
    alive_agent_num = env_cont_agent_mask.sum().item()

    expert_trajectory_lst = torch.zeros((alive_agent_num, h.episode_len, obs.shape[-1]), device=device)
    expert_actions_lst = torch.zeros((alive_agent_num, h.episode_len, 3), device=device)
    expert_dead_mask_lst = torch.ones((alive_agent_num, h.episode_len), device=device, dtype=torch.bool)
    expert_partner_mask_lst = torch.full((alive_agent_num, h.episode_len, A - 1), 2, device=device, dtype=torch.long)
    expert_road_mask_lst = torch.ones((alive_agent_num, h.episode_len, 200), device=device, dtype=torch.bool)
    expert_global_pos_lst = torch.zeros((alive_agent_num, h.episode_len, 2), device=device)  # global pos (2)
    expert_global_rot_lst = torch.zeros((alive_agent_num, h.episode_len, 1), device=device)  # global actions (1)
    # Initialize dead agent mask
    agent_info = h.sim.absolute_self_observation_tensor().to_torch().to(device)
    dead_agent_mask = ~env_cont_agent_mask.clone().to(device)  # (num_worlds, num_agents)
    road_mask = h.get_road_mask()
    goal_achieved = 0
    off_road = 0
    veh_collision = 0
    collision = None
    iterations = 0
    for time_step in range(h.episode_len):
        iterations += 1
        for idx, (world_idx, agent_idx) in enumerate(alive_agent_indices):
            if not dead_agent_mask[world_idx, agent_idx]:
                expert_trajectory_lst[idx][time_step] = obs[world_idx, agent_idx]
                expert_actions_lst[idx][time_step] = expert_actions[world_idx, agent_idx, time_step]
                expert_partner_mask_lst[idx][time_step] = partner_mask[world_idx, agent_idx]
                expert_road_mask_lst[idx][time_step] = road_mask[world_idx, agent_idx]
                expert_global_pos_lst[idx, time_step] = agent_info[world_idx, agent_idx, 0:2]
                expert_global_rot_lst[idx, time_step] = agent_info[world_idx, agent_idx, 7:8]
            expert_dead_mask_lst[idx][time_step] = dead_agent_mask[world_idx, agent_idx]

        # env.step() -> gather next obs
        h.step_dynamics(expert_actions[:, :, time_step, :])
        dones = h.get_dones().to(device)

        dead_agent_mask = torch.logical_or(dead_agent_mask, dones)
        obs, partner_mask = observe()
        road_mask = h.get_road_mask()
        agent_info = h.sim.absolute_self_observation_tensor().to_torch().to(device)
        infos = h.get_infos()

        goal_achieved += infos.goal_achieved[cont_agent_mask]
        off_road += infos.off_road[cont_agent_mask]
        veh_collision += infos.collided[cont_agent_mask]
        goal_achieved = torch.clamp(goal_achieved, max=1.0)
        off_road = torch.clamp(off_road, max=1.0)
        veh_collision = torch.clamp(veh_collision, max=1.0)

        if (dead_agent_mask == True).all():  # noqa: E712 (the reference's spelling)
            collision = (veh_collision + off_road > 0)
            break

    if collision is None:
        collision = (veh_collision + off_road > 0)
    return dict(obs=expert_trajectory_lst, actions=expert_actions_lst, dead_mask=expert_dead_mask_lst,
                partner_mask=expert_partner_mask_lst, road_mask=expert_road_mask_lst,
                ego_global_pos=expert_global_pos_lst, ego_global_rot=expert_global_rot_lst,
                goal_achieved=goal_achieved, off_road=off_road, veh_collision=veh_collision, collision=collision,
                iterations=iterations)
