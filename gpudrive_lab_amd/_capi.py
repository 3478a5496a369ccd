"""ctypes binding of include/gpudrive_amd.h.  There is no CPU fallback: if the HIP library is
missing or no gfx950 device is visible, calls fail loudly."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libgpudrive_amd.so")
# Developer experiments only (tools/build_expt.sh writes them to build/expt/, outside this package): another build of the
# library is loaded only when GPUDRIVE_DEV=1 says so as well -- a stray GPUDRIVE_AMD_LIB alone must never make a bench or
# a test run a diagnostic build.
if os.environ.get("GPUDRIVE_AMD_LIB"):
    if os.environ.get("GPUDRIVE_DEV") != "1":
        raise ImportError("GPUDRIVE_AMD_LIB is set but GPUDRIVE_DEV=1 is not: refusing to load a developer build of the "
                          "library (unset GPUDRIVE_AMD_LIB, or set GPUDRIVE_DEV=1 for an experiment)")
    _SO = os.environ["GPUDRIVE_AMD_LIB"]
_LIB = None

GD_OK = 0
GD_ERR_INVALID, GD_ERR_IO, GD_ERR_PARSE, GD_ERR_DEVICE, GD_ERR_UNSUPPORTED = -1, -2, -3, -4, -5

(T_ACTION, T_REWARD, T_DONE, T_INFO, T_SELF_OBS, T_ABS_OBS, T_PARTNER_OBS, T_AGENT_MAP_OBS, T_MAP_OBS,
 T_LIDAR, T_BEV, T_STEPS_REMAINING, T_SHAPE, T_CONTROLLED_STATE, T_RESPONSE_TYPE, T_EXPERT_TRAJECTORY,
 T_WORLD_MEANS, T_METADATA, T_DELETED_AGENTS, T_MAP_NAME, T_SCENARIO_ID, T_COUNT) = range(22)

DTYPE_F32, DTYPE_I32 = 0, 1


class GdParams(C.Structure):
    _fields_ = [
        ("polylineReductionThreshold", C.c_float),
        ("observationRadius", C.c_float),
        ("rewardType", C.c_int32),
        ("distanceToGoalThreshold", C.c_float),
        ("distanceToExpertThreshold", C.c_float),
        ("collisionBehaviour", C.c_int32),
        ("maxNumControlledAgents", C.c_uint32),
        ("IgnoreNonVehicles", C.c_int32),
        ("roadObservationAlgorithm", C.c_int32),
        ("initOnlyValidAgentsAtFirstStep", C.c_int32),
        ("isStaticAgentControlled", C.c_int32),
        ("enableLidar", C.c_int32),
        ("disableClassicalObs", C.c_int32),
        ("dynamicsModel", C.c_int32),
        ("readFromTracksToPredict", C.c_int32),
    ]


class GdTensorDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("ndim", C.c_int32),
                ("dims", C.c_int64 * 5), ("nbytes", C.c_int64)]


class GdConfig(C.Structure):
    _fields_ = [("num_worlds", C.c_int32), ("max_agents", C.c_int32), ("device_id", C.c_int32),
                ("stream", C.c_void_p), ("knn_order", C.c_int32), ("alloc_bev", C.c_int32),
                ("lidar_half_angle", C.c_float), ("external", C.c_void_p * T_COUNT)]


class GdHostWorld(C.Structure):
    _fields_ = [("num_agents", C.c_int32), ("num_roads", C.c_int32), ("num_collidable_roads", C.c_int32),
                ("max_agents", C.c_int32), ("mean", C.c_float * 3), ("map_name", C.c_int32 * 32),
                ("scenario_id", C.c_int32 * 32), ("map_obs", C.POINTER(C.c_float)),
                ("trajectory", C.POINTER(C.c_float)), ("controlled", C.POINTER(C.c_int32)),
                ("response_type", C.POINTER(C.c_int32)), ("agent_id", C.POINTER(C.c_int32)),
                ("entity_type", C.POINTER(C.c_int32)), ("metadata", C.POINTER(C.c_int32)),
                ("vehicle_size", C.POINTER(C.c_float)), ("goal", C.POINTER(C.c_float))]


EPISODE_STATS = 12
EPISODE_STAT_NAMES = ("episodes", "finished_agents", "return_sum", "off_road_agents", "collided_agents", "goal_achieved",
                      "truncated_agents", "length_sum", "total_collisions", "total_off_road")


EPISODE_REWARD_WEIGHTED, EPISODE_REWARD_SPARSE, EPISODE_REWARD_CONDITIONED, EPISODE_REWARD_LOG_DISTANCE = range(4)
CONDITION_RANDOM, CONDITION_PRESET, CONDITION_FIXED = range(3)
WARMUP_RESET_WORLDS, WARMUP_ALL_WORLDS = range(2)
INIT_STEPS_MAX = 90  # the expert trajectory has 91 steps
STAT_WARMED_WORLDS = 46  # gd_stat: worlds the warm-up of the device auto-reset advanced


class GdEpisodeConfig(C.Structure):
    _fields_ = [("collision_weight", C.c_float), ("goal_achieved_weight", C.c_float), ("off_road_weight", C.c_float),
                ("reward_type", C.c_int32), ("auto_reset", C.c_int32),
                ("log_distance_weight", C.c_float), ("condition_mode", C.c_int32), ("weights", C.c_float * 3),
                ("lb", C.c_float * 3), ("ub", C.c_float * 3), ("seed", C.c_uint64)]


class GdEpisodeBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "controlled_mask", "agent_episode_returns", "episode_lengths", "collided_in_episode", "offroad_in_episode",
        "live_agent_mask", "reward_out", "terminal_out", "truncated_out", "mask_out", "done_worlds", "stats", "world_stats",
        "reward_weights", "weight_draws")]


class GdEpisodeBuffersRows(GdEpisodeBuffers):
    """The whole gd_episode_buffers: GdEpisodeBuffers (the layout before the learner rows) + the four flat outputs appended
    with them.  The entry points take this one only, so that the engine never reads past a caller's struct."""
    _fields_ = [(n, C.c_void_p) for n in ("reward_rows", "terminal_rows", "truncated_rows", "mask_rows")]


class GdRecordBuffers(C.Structure):
    """gd_record_buffers: the expert trajectory recorder's outputs and running state (device pointers; kernel_ms: host)."""
    _fields_ = ([("row_slot", C.c_void_p), ("n_rows", C.c_int32)] +
                [(n, C.c_void_p) for n in ("obs", "actions", "dead_mask", "partner_mask", "road_mask", "ego_global_pos",
                                           "ego_global_rot", "dead", "goal_achieved", "off_road", "veh_collision",
                                           "any_alive")] +
                [("kernel_ms", C.POINTER(C.c_float))])


IL_MAX_SHARDS = 8


class GdIlShard(C.Structure):
    """gd_il_shard: one recorded episode batch of the device expert dataset (device pointers)."""
    _fields_ = [(n, C.c_void_p) for n in ("obs", "actions", "dead_mask", "partner_mask", "road_mask", "keep")] + [("n_rows", C.c_int32)]


class GdIlDataset(C.Structure):
    _fields_ = [("shard", GdIlShard * IL_MAX_SHARDS), ("n_shards", C.c_int32), ("max_agents", C.c_int32),
                ("rollout_len", C.c_int32), ("pred_len", C.c_int32)]


class GdIlBatchBuffers(C.Structure):
    """gd_il_batch_buffers: the index, the selection and the five outputs of one batch (device pointers)."""
    _fields_ = [("entries", C.c_void_p), ("n_entries", C.c_int64), ("sel", C.c_void_p), ("batch", C.c_int32),
                ("bad_indices", C.c_void_p), ("obs", C.c_void_p), ("actions", C.c_void_p), ("partner_mask", C.c_void_p),
                ("road_mask", C.c_void_p), ("data_idx", C.c_void_p)]


IL_FUTURE_OTHER, IL_FUTURE_EGO = range(2)


class GdIlFuture(C.Structure):
    """gd_il_future: the per-shard ego poses (device pointers), the future step, the experiment and the 2 x 9 bin edges."""
    _fields_ = [("ego_global_pos", C.c_void_p * IL_MAX_SHARDS), ("ego_global_rot", C.c_void_p * IL_MAX_SHARDS),
                ("future_step", C.c_int32), ("exp", C.c_int32), ("xbins", C.c_double * 9), ("ybins", C.c_double * 9)]


class GdIlFutureBuffers(C.Structure):
    """gd_il_future_buffers: the index, the selection and the eight outputs of one linear-probing batch (device pointers)."""
    _fields_ = [("entries", C.c_void_p), ("n_entries", C.c_int64), ("sel", C.c_void_p), ("batch", C.c_int32),
                ("bad_indices", C.c_void_p), ("obs", C.c_void_p), ("actions", C.c_void_p), ("valid_mask", C.c_void_p),
                ("ego_mask", C.c_void_p), ("partner_mask", C.c_void_p), ("road_mask", C.c_void_p), ("future_mask", C.c_void_p),
                ("future_pos", C.c_void_p)]


class GdRollout(C.Structure):
    """gd_rollout: the sizes, the storage and the counters of the device rollout buffer (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("batch_size", "num_rows", "obs_width", "action_width")] +
                [(n, C.c_void_p) for n in ("obs", "actions", "logprobs", "rewards", "dones", "values", "row", "ord", "count",
                                           "dst", "state")])


ROLLOUT_STATE = ("ptr", "step", "dropped", "bad_positions")  # gd_rollout.state


class GdRolloutBatch(C.Structure):
    """gd_rollout_batch: the permutation, the advantages, the minibatch geometry and the seven outputs (device pointers)."""
    _fields_ = ([("idxs", C.c_void_p), ("advantages", C.c_void_p)] +
                [(n, C.c_int32) for n in ("num_minibatches", "minibatch_rows", "bptt_horizon", "first", "n", "split")] +
                [(n, C.c_void_p) for n in ("obs", "actions", "logprobs", "dones", "values", "advantages_out", "returns")])


class GdPolicy(C.Structure):
    """gd_policy: the sizes, the packed weights and the two scratch arrays of the device policy forward (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("num_rows", "max_agents", "ego_width", "n_actions")] +
                [("blob", C.c_void_p), ("blob_floats", C.c_int64), ("features", C.c_void_p), ("logits", C.c_void_p)])


class GdPolicyGrad(C.Structure):
    """gd_policy_grad: what gd_policy_evaluate saves for gd_policy_backward, and the backward's weights and scratch (device
    pointers)."""
    _fields_ = ([(n, C.c_void_p) for n in ("features", "logits", "winners", "params", "rowstat", "partials")] +
                [("grad_floats", C.c_int64), ("num_partials", C.c_int32), ("reserved", C.c_int32)])


PPO_STATS = ("policy_loss", "value_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")  # gd_ppo.stats


class GdPPO(C.Structure):
    """gd_ppo: the hyper-parameters, the device scalars, the optimiser state and the scratch of the device PPO update (device
    pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("num_rows", "ego_width", "n_actions", "norm_adv", "clip_vloss")] +
                [(n, C.c_float) for n in ("clip_coef", "vf_clip_coef", "ent_coef", "vf_coef", "max_grad_norm", "eps",
                                          "stats_scale")] +
                [("beta1", C.c_double), ("beta2", C.c_double), ("grad_floats", C.c_int64), ("blob_floats", C.c_int64)] +
                [(n, C.c_void_p) for n in ("lr", "step", "beta_pow", "params", "exp_avg", "exp_avg_sq", "blob", "blob_of",
                                           "stats", "stats_sum", "scal", "newlogprob", "entropy", "newvalue", "d_logprob",
                                           "d_entropy", "d_value", "grad")])


class GdDropout(C.Structure):
    """gd_dropout: the seed, the device call counter, the word evaluate leaves for backward, the threshold and the scale of
    the training-mode masks (csrc/dropout_rule.hpp)."""
    _fields_ = [("seed", C.c_uint64), ("call", C.c_void_p), ("used", C.c_void_p), ("threshold", C.c_uint32), ("scale", C.c_float)]


class GdBCPolicy(C.Structure):
    """gd_bc_policy: the sizes, the packed weights and the chunk scratch of the device BC policy forward (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("max_agents", "num_stack", "fusion_layers", "branch_layers", "head_layers",
                                          "n_components")] +
                [("clip_value", C.c_float), ("chunk_rows", C.c_int32), ("blob", C.c_void_p), ("blob_floats", C.c_int64),
                 ("scratch", C.c_void_p), ("scratch_floats", C.c_int64)])


class GdBCPolicyDim(C.Structure):
    """gd_bc_policy_dim: gd_bc_policy with the encoder's width (64 or 128) beside it, for the gd_bc_*_dim entry points."""
    _fields_ = [("base", GdBCPolicy), ("network_dim", C.c_int32), ("reserved", C.c_int32)]


class GdBCOutputs(C.Structure):
    """gd_bc_outputs: the outputs of one gd_bc_forward (device pointers; NULL: not written)."""
    _fields_ = [(n, C.c_void_p) for n in ("context", "means", "log_covariances", "covariances", "weights", "actions", "nll",
                                          "ego_attn_score", "component")]


class GdBCRolloutBuffers(C.Structure):
    """gd_bc_rollout_buffers: the rows, the draws, the window and masks the forward reads, the running state, the results and
    the optional per-step records of one closed-loop episode (device pointers)."""
    _fields_ = ([("row_slot", C.c_void_p), ("row_of_slot", C.c_void_p), ("n_rows", C.c_int32), ("deterministic", C.c_int32)] +
                [(n, C.c_void_p) for n in ("u", "z", "window", "partner_mask", "road_mask", "partner_value", "row_actions",
                                           "dead", "goal_achieved", "off_road", "veh_collision", "goal_step", "off_road_step",
                                           "init_goal_dist", "goal_dist", "any_alive", "summary", "actions", "dead_mask",
                                           "ego_global_pos", "ego_global_rot")])


BC_ROLLOUT_SUMMARY = ("off_road_rate", "veh_coll_rate", "goal_rate", "collision_rate", "goal_progress", "goal_count", "n_rows",
                      "iterations")  # gd_bc_rollout_buffers.summary


class GdPolicyRolloutBuffers(C.Structure):
    """gd_policy_rollout_buffers: the draws, the action table, the forward's outputs, the running state, the per-world results
    and the optional per-step records of one closed-loop episode of the late-fusion policy (device pointers)."""
    _fields_ = ([("n_rows", C.c_int32), ("deterministic", C.c_int32), ("u", C.c_void_p), ("table", C.c_void_p),
                 ("n_actions", C.c_int32), ("reserved", C.c_int32)] +
                [(n, C.c_void_p) for n in ("actions", "logprob", "entropy", "value", "live", "goal_achieved", "collided",
                                           "off_road", "world_active", "episode_lengths", "bad_indices", "any_active",
                                           "goal_achieved_count", "frac_goal_achieved", "collided_count", "frac_collided",
                                           "off_road_count", "frac_off_road", "other_count", "frac_other",
                                           "controlled_per_scene", "summary", "actions_idx", "live_mask", "agent_positions")])


POLICY_ROLLOUT_SUMMARY = ("goal_achieved", "collided", "off_road", "other", "n_rows", "worlds_with_rows", "iterations",
                          "mean_episode_length")  # gd_policy_rollout_buffers.summary


LIVE_ROWS_BLOCK = 1024  # GD_LIVE_ROWS_BLOCK: gd_live_rows' scratch has one int32 per block of this many rows


class GdPolicyRolloutRows(C.Structure):
    """gd_policy_rollout_rows: the row list of the current step, its length, gd_live_rows' scratch and the optional record of
    the lengths of one closed-loop episode with the list in the loop (device pointers)."""
    _fields_ = [(n, C.c_void_p) for n in ("rows", "count", "scratch", "live_count")] + [("reserved", C.c_int32)]


POLICY_SET_MAX = 8    # GD_POLICY_SET_MAX: the policies of one gd_policy_set
OWNED_ROWS_ALIGN = 32  # every segment of an owned list starts at a multiple of this (csrc/multi_policy_rule.hpp)


class GdPolicySet(C.Structure):
    """gd_policy_set: the policies of one forward on an owned list and the call's own position-indexed scratch (device
    pointers)."""
    _fields_ = [("n_policies", C.c_int32), ("reserved", C.c_int32), ("policy", GdPolicy * POLICY_SET_MAX),
                ("features", C.c_void_p), ("logits", C.c_void_p)]


MULTI_POLICY_WORLD = ("goal_achieved_count", "frac_goal_achieved", "collided_count", "frac_collided", "off_road_count",
                      "frac_off_road", "n_rows")  # gd_multi_policy_buffers: [P][W] each
MULTI_POLICY_SUMMARY = ("goal_achieved", "collided", "off_road", "n_rows")  # gd_multi_policy_buffers.summary, per policy


class GdMultiPolicyBuffers(C.Structure):
    """gd_multi_policy_buffers: the owners, the owned list and its scratch, the denominator, the per-policy results and the
    optional record of the segment lengths of one multi-policy episode (device pointers)."""
    _fields_ = ([(n, C.c_void_p) for n in ("owner", "rows", "start", "count", "scratch", "denominator") + MULTI_POLICY_WORLD
                 + ("summary", "list_count")] + [("reserved", C.c_int32)])


class GdBCRolloutRows(C.Structure):
    """gd_bc_rollout_rows: gd_policy_rollout_rows for the closed-loop BC driver (device pointers)."""
    _fields_ = [(n, C.c_void_p) for n in ("rows", "count", "scratch", "live_count")] + [("reserved", C.c_int32)]


class GdBCGrad(C.Structure):
    """gd_bc_grad: the scratch and the partial sums of one gd_bc_backward (device pointers)."""
    _fields_ = [("scratch", C.c_void_p), ("scratch_floats", C.c_int64), ("partials", C.c_void_p), ("grad_floats", C.c_int64),
                ("num_partials", C.c_int32), ("reserved", C.c_int32)]


BC_STATS = ("loss", "dx_loss", "dy_loss", "dyaw_loss", "grad_norm", "max_grad_norm")  # gd_bc_opt.stats


class GdBCOpt(C.Structure):
    """gd_bc_opt: the hyper-parameters, the configuration, the device scalars, the optimiser state and the scratch of the device
    BC update (device pointers)."""
    _fields_ = ([(n, C.c_float) for n in ("max_grad_norm", "eps", "weight_decay", "stats_scale")] +
                [("beta1", C.c_double), ("beta2", C.c_double), ("grad_floats", C.c_int64), ("blob_floats", C.c_int64)] +
                [(n, C.c_int32) for n in ("num_stack", "fusion_layers", "branch_layers", "head_layers", "n_components",
                                          "num_tensors", "max_rows", "reserved")] +
                [(n, C.c_void_p) for n in ("tensor_end", "lr", "step", "beta_pow", "params", "exp_avg", "exp_avg_sq", "blob",
                                           "blob_of", "stats", "stats_sum", "max_grad_tensor", "tensor_norms", "scal",
                                           "actions", "nll", "grad_nll", "grad")])


LP_TAP_FUSION, LP_TAP_RO = range(2)
LP_EARLY, LP_LATE, LP_BASELINE = range(3)
LP_EVAL_WORDS = 208  # gd_lp_eval_accumulate's acc, int32 words
LP_PART_INTS = 392   # gd_lp_probe.part_i, words per partial
LP_STATS = ("loss", "accuracy", "f1_macro", "ood_loss_sum", "ood_correct", "ood_rows", "rows", "bad_labels")  # gd_lp_probe.stats


class GdLPProbe(C.Structure):
    """gd_lp_probe: the configuration, the weights in both layouts, the optimiser state and the scratch of the device linear
    probe (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("model", "exp", "in_features", "num_partials", "max_agents", "num_stack")] +
                [("reserved", C.c_int32 * 2), ("eps", C.c_float), ("weight_decay", C.c_float), ("beta1", C.c_double),
                 ("beta2", C.c_double)] +
                [(n, C.c_void_p) for n in ("weight", "packed", "exp_avg", "exp_avg_sq", "lr", "step", "beta_pow", "grad", "part_f",
                                           "part_d", "part_i", "stats", "sums", "counts", "scal")])


class GdLPRows(C.Structure):
    """gd_lp_rows: the optional per-row outputs of the gd_lp_* calls (device pointers; NULL: not written)."""
    _fields_ = [(n, C.c_void_p) for n in ("logits", "loss_row", "pred")]


BC_READOUT_MAX = 8      # GD_BC_READOUT_MAX: the probes of one list of a gd_bc_readout
BC_READOUT_NO_CLASS = 255  # the fill value of the class outputs of a closed-loop episode


class GdBCReadoutProbe(C.Structure):
    """gd_bc_readout_probe: a probe's packed and flat weights (device pointers)."""
    _fields_ = [("packed", C.c_void_p), ("weight", C.c_void_p)]


class GdBCReadout(C.Structure):
    """gd_bc_readout: the tap, the probes, the labels, the three outputs with their row strides and the bad-label counter of the
    probe read-outs inside the BC forward (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("tap", "layer", "n_other", "n_ego", "intervene", "reserved")] +
                [("other", GdBCReadoutProbe * BC_READOUT_MAX), ("ego", GdBCReadoutProbe * BC_READOUT_MAX),
                 ("labels", C.c_void_p), ("label", C.c_int64)] +
                [(n, C.c_void_p) for n in ("other_pred", "ego_pred", "ego_pred_prime")] +
                [(n, C.c_int64) for n in ("other_stride", "ego_stride", "prime_stride")] + [("bad_labels", C.c_void_p)])


class GdBCRolloutReads(C.Structure):
    """gd_bc_rollout_reads: the per-step attention scores and the read-out of a closed-loop episode (device pointers)."""
    _fields_ = [("ego_attn_score", C.c_void_p), ("readout", C.POINTER(GdBCReadout))]


# every symbol include/gpudrive_amd.h declares
SYMBOLS = [
    "gd_version", "gd_last_error", "gd_default_params", "gd_tensor_shape", "gd_create", "gd_destroy",
    "gd_step", "gd_reset", "gd_set_maps", "gd_delete_agents", "gd_tensor", "gd_pack_observations", "gd_attach_packed",
    "gd_expert_actions", "gd_advance_log_playback", "gd_record_expert", "gd_il_index", "gd_il_batch", "gd_il_future_batch",
    "gd_rollout_store", "gd_rollout_sort", "gd_rollout_gae", "gd_rollout_gather", "gd_policy_forward",
    "gd_policy_evaluate", "gd_policy_backward", "gd_ppo_loss", "gd_ppo_adam", "gd_ppo_update",
    "gd_policy_forward_dropout", "gd_policy_evaluate_dropout", "gd_policy_backward_dropout", "gd_ppo_update_dropout",
    "gd_bc_forward", "gd_bc_backward", "gd_bc_eval_accumulate", "gd_bc_train_rows", "gd_bc_adamw", "gd_bc_update",
    "gd_bc_rollout", "gd_policy_rollout", "gd_live_rows", "gd_policy_forward_rows", "gd_policy_rollout_compact", "gd_owned_rows", "gd_policy_forward_owned",
    "gd_multi_policy_rollout", "gd_bc_forward_rows", "gd_bc_rollout_compact", "gd_bc_hidden", "gd_bc_hidden_layer", "gd_bc_forward_readout", "gd_bc_forward_rows_readout", "gd_bc_rollout_readout", "gd_bc_forward_dim", "gd_bc_forward_rows_dim", "gd_bc_rollout_dim", "gd_bc_backward_dim", "gd_bc_adamw_dim", "gd_bc_update_dim", "gd_lp_forward", "gd_lp_update", "gd_lp_eval_accumulate", "gd_episode_step",
    "gd_sync",
    "gd_pack_observations_conditioned", "gd_episode_draw_weights", "gd_episode_set_warmup",
    "gd_set_learner_rows", "gd_attach_packed_rows", "gd_attach_packed_rows_conditioned", "gd_set_discrete_actions",
    "gd_set_stream", "gd_attach_bev", "gd_stat",
    "gd_kernel_timing_enable", "gd_kernel_timing_read", "gd_debug_get_state", "gd_debug_set_state", "gd_debug_road_path",
    "gd_host_world_build", "gd_host_world_free", "gd_scene_cache_write",
]


def lib_path():
    return _SO


def build(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcdir = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", srcdir]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return _SO


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise ImportError(
            "gpudrive_lab_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the step path." % _SO)
    # torch-ROCm bundles its own libamdhip64.so.7; load it first so that this library binds to the
    # SAME HIP runtime instance (two runtimes in one process cannot both own the device, and the
    # engine is handed torch-allocated device pointers).
    import torch  # noqa: F401
    L = C.CDLL(_SO)
    L.gd_version.restype = C.c_char_p
    L.gd_last_error.restype = C.c_char_p
    L.gd_default_params.argtypes = [C.POINTER(GdParams)]
    L.gd_default_params.restype = None
    L.gd_tensor_shape.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(GdTensorDesc)]
    L.gd_create.argtypes = [C.POINTER(GdConfig), C.POINTER(GdParams), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
    L.gd_destroy.argtypes = [C.c_void_p]
    L.gd_destroy.restype = None
    L.gd_step.argtypes = [C.c_void_p]
    L.gd_reset.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.gd_set_maps.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32]
    L.gd_delete_agents.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
    L.gd_tensor.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GdTensorDesc)]
    L.gd_sync.argtypes = [C.c_void_p]
    L.gd_pack_observations.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.gd_attach_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    L.gd_attach_packed.restype = C.c_int
    L.gd_episode_step.argtypes = [C.c_void_p, C.POINTER(GdEpisodeConfig), C.POINTER(GdEpisodeBuffersRows)]
    L.gd_episode_draw_weights.argtypes = [C.c_void_p, C.POINTER(GdEpisodeConfig), C.POINTER(GdEpisodeBuffersRows),
                                          C.POINTER(C.c_int32), C.c_int32]
    L.gd_episode_set_warmup.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.gd_set_learner_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.gd_attach_packed_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    L.gd_attach_packed_rows_conditioned.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    L.gd_set_discrete_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.gd_pack_observations_conditioned.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.gd_scene_cache_write.argtypes = [C.c_char_p, C.c_float, C.c_char_p]
    L.gd_expert_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gd_advance_log_playback.argtypes = [C.c_void_p, C.c_int32]
    L.gd_record_expert.argtypes = [C.c_void_p, C.POINTER(GdRecordBuffers), C.c_int32]
    L.gd_il_index.argtypes = [C.POINTER(GdIlDataset), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gd_il_batch.argtypes = [C.POINTER(GdIlDataset), C.POINTER(GdIlBatchBuffers), C.c_void_p]
    L.gd_il_future_batch.argtypes = [C.POINTER(GdIlDataset), C.POINTER(GdIlFuture), C.POINTER(GdIlFutureBuffers), C.c_void_p]
    L.gd_rollout_store.argtypes = [C.POINTER(GdRollout)] + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p]
    L.gd_rollout_sort.argtypes = [C.POINTER(GdRollout), C.c_void_p, C.c_void_p, C.c_void_p]
    L.gd_rollout_gae.argtypes = [C.POINTER(GdRollout), C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]
    L.gd_rollout_gather.argtypes = [C.POINTER(GdRollout), C.POINTER(GdRolloutBatch), C.c_void_p]
    L.gd_policy_forward.argtypes = [C.POINTER(GdPolicy), C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    L.gd_policy_evaluate.argtypes = [C.POINTER(GdPolicy), C.POINTER(GdPolicyGrad)] + [C.c_void_p] * 6
    L.gd_policy_backward.argtypes = [C.POINTER(GdPolicy), C.POINTER(GdPolicyGrad)] + [C.c_void_p] * 7
    L.gd_ppo_loss.argtypes = [C.POINTER(GdPPO)] + [C.c_void_p] * 11
    L.gd_ppo_adam.argtypes = [C.POINTER(GdPPO), C.c_void_p, C.c_void_p]
    L.gd_ppo_update.argtypes = [C.POINTER(GdPolicy), C.POINTER(GdPolicyGrad), C.POINTER(GdPPO)] + [C.c_void_p] * 7
    D = C.POINTER(GdDropout)
    L.gd_policy_forward_dropout.argtypes = [C.POINTER(GdPolicy), D, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    L.gd_policy_evaluate_dropout.argtypes = [C.POINTER(GdPolicy), C.POINTER(GdPolicyGrad), D] + [C.c_void_p] * 6
    L.gd_policy_backward_dropout.argtypes = [C.POINTER(GdPolicy), C.POINTER(GdPolicyGrad), D] + [C.c_void_p] * 7
    L.gd_ppo_update_dropout.argtypes = [C.POINTER(GdPolicy), C.POINTER(GdPolicyGrad), C.POINTER(GdPPO), D] + [C.c_void_p] * 7
    L.gd_bc_forward.argtypes = ([C.POINTER(GdBCPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] +
                                [C.c_void_p] * 3 + [C.POINTER(GdBCOutputs), C.c_void_p])
    L.gd_bc_backward.argtypes = ([C.POINTER(GdBCPolicy), C.POINTER(GdBCGrad), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] +
                                 [C.c_void_p] * 5)
    L.gd_bc_eval_accumulate.argtypes = [C.c_int32] + [C.c_void_p] * 5
    L.gd_bc_train_rows.argtypes = [C.POINTER(GdBCOpt), C.c_int32] + [C.c_void_p] * 5
    L.gd_bc_adamw.argtypes = [C.POINTER(GdBCOpt), C.c_void_p, C.c_void_p]
    L.gd_bc_update.argtypes = ([C.POINTER(GdBCPolicy), C.POINTER(GdBCGrad), C.POINTER(GdBCOpt)] + [C.c_void_p] * 3 +
                               [C.c_int32, C.c_void_p, C.c_void_p])
    L.gd_bc_rollout.argtypes = [C.c_void_p, C.POINTER(GdBCPolicy), C.POINTER(GdBCRolloutBuffers), C.c_int32]
    L.gd_policy_rollout.argtypes = [C.c_void_p, C.POINTER(GdPolicy), C.POINTER(GdPolicyRolloutBuffers), C.c_int32]
    L.gd_live_rows.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    L.gd_policy_forward_rows.argtypes = [C.POINTER(GdPolicy), D, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    L.gd_policy_rollout_compact.argtypes = [C.c_void_p, C.POINTER(GdPolicy), C.POINTER(GdPolicyRolloutBuffers),
                                            C.POINTER(GdPolicyRolloutRows), C.c_int32]
    L.gd_owned_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    L.gd_policy_forward_owned.argtypes = [C.POINTER(GdPolicySet), C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 9
    L.gd_multi_policy_rollout.argtypes = [C.c_void_p, C.POINTER(GdPolicySet), C.POINTER(GdPolicyRolloutBuffers),
                                          C.POINTER(GdMultiPolicyBuffers), C.c_int32]
    L.gd_bc_forward_rows.argtypes = ([C.POINTER(GdBCPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] +
                                     [C.c_void_p] * 3 + [C.POINTER(GdBCOutputs)] + [C.c_void_p] * 3)
    L.gd_bc_rollout_compact.argtypes = [C.c_void_p, C.POINTER(GdBCPolicy), C.POINTER(GdBCRolloutBuffers),
                                        C.POINTER(GdBCRolloutRows), C.c_int32]
    L.gd_bc_hidden.argtypes = [C.POINTER(GdBCPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.gd_bc_hidden_layer.argtypes = ([C.POINTER(GdBCPolicy), C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 3 +
                                     [C.c_void_p, C.c_void_p])
    L.gd_bc_forward_readout.argtypes = ([C.POINTER(GdBCPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] +
                                        [C.c_void_p] * 3 + [C.POINTER(GdBCOutputs), C.POINTER(GdBCReadout), C.c_void_p])
    L.gd_bc_forward_rows_readout.argtypes = ([C.POINTER(GdBCPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] +
                                             [C.c_void_p] * 3 + [C.POINTER(GdBCOutputs), C.POINTER(GdBCReadout)] + [C.c_void_p] * 3)
    L.gd_bc_rollout_readout.argtypes = [C.c_void_p, C.POINTER(GdBCPolicy), C.POINTER(GdBCRolloutBuffers),
                                        C.POINTER(GdBCRolloutRows), C.POINTER(GdBCRolloutReads), C.c_int32]
    L.gd_bc_forward_dim.argtypes = ([C.POINTER(GdBCPolicyDim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] +
                                    [C.c_void_p] * 3 + [C.POINTER(GdBCOutputs), C.c_void_p])
    L.gd_bc_forward_rows_dim.argtypes = ([C.POINTER(GdBCPolicyDim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] +
                                         [C.c_void_p] * 3 + [C.POINTER(GdBCOutputs)] + [C.c_void_p] * 3)
    L.gd_bc_rollout_dim.argtypes = [C.c_void_p, C.POINTER(GdBCPolicyDim), C.POINTER(GdBCRolloutBuffers),
                                    C.POINTER(GdBCRolloutRows), C.POINTER(GdBCRolloutReads), C.c_int32]
    L.gd_bc_backward_dim.argtypes = ([C.POINTER(GdBCPolicyDim), C.POINTER(GdBCGrad), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] +
                                     [C.c_void_p] * 5)
    L.gd_bc_adamw_dim.argtypes = [C.POINTER(GdBCOpt), C.c_int32, C.c_void_p, C.c_void_p]
    L.gd_bc_update_dim.argtypes = ([C.POINTER(GdBCPolicyDim), C.POINTER(GdBCGrad), C.POINTER(GdBCOpt)] + [C.c_void_p] * 3 +
                                   [C.c_int32, C.c_void_p, C.c_void_p])
    lp = [C.POINTER(GdBCPolicy), C.POINTER(GdLPProbe), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    L.gd_lp_forward.argtypes = lp + [C.POINTER(GdLPRows), C.c_void_p]
    L.gd_lp_update.argtypes = lp + [C.c_void_p, C.c_void_p, C.POINTER(GdLPRows), C.c_void_p]
    L.gd_lp_eval_accumulate.argtypes = lp + [C.c_void_p, C.c_void_p, C.POINTER(GdLPRows), C.c_void_p, C.c_void_p]
    L.gd_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.gd_attach_bev.argtypes = [C.c_void_p, C.c_void_p]
    L.gd_stat.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    L.gd_kernel_timing_enable.argtypes = [C.c_void_p, C.c_int32]
    L.gd_kernel_timing_read.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.gd_debug_get_state.argtypes = [C.c_void_p, C.c_void_p]
    L.gd_debug_set_state.argtypes = [C.c_void_p, C.c_void_p]
    L.gd_debug_road_path.argtypes = [C.c_void_p, C.c_void_p]
    L.gd_host_world_build.argtypes = [C.c_char_p, C.POINTER(GdParams), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                      C.POINTER(GdHostWorld)]
    L.gd_host_world_free.argtypes = [C.POINTER(GdHostWorld)]
    L.gd_host_world_free.restype = None
    _LIB = L
    return L


def check(rc, what="call"):
    if rc == GD_OK:
        return
    msg = lib().gd_last_error().decode("utf-8", "replace")
    if rc == GD_ERR_IO:
        raise FileNotFoundError(msg)
    if rc == GD_ERR_INVALID:
        raise ValueError(msg)
    if rc == GD_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError("%s failed (%d): %s" % (what, rc, msg))
