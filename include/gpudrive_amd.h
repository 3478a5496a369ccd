/*
 * gpudrive_amd.h -- C ABI of the MI355X-native GPUDrive step engine (libgpudrive_amd.so).
 *
 * This is the drop-in boundary for ONE path of CILAB-MA/gpudrive_lab: the batched per-world
 * simulation step behind `madrona_gpudrive.SimManager`.  Every entry point names the reference
 * interface it replaces (paths relative to the reference checkout).  Plain pointers and sizes
 * only; no torch / Python types.  All functions return GD_OK (0) or a negative error code and
 * never abort the process; gd_last_error() returns the message of the calling thread's last
 * failure.
 *
 * Buffers: every exported tensor lives in device (HBM) memory for the lifetime of the sim.
 * Either the caller hands in device pointers (gd_config.external[...], e.g. torch-allocated
 * storage so that `.to_torch()` is a zero-copy alias) or the engine allocates them itself.
 * The exported buffers ARE the live simulation storage, exactly like Madrona's exported ECS
 * columns: actions are written in place by the caller (gpudrive/env/env_torch.py:645-664) and
 * `controlled_state`, `done`, `expert_trajectory` ... are read back by the next step.
 */
#ifndef GPUDRIVE_AMD_H
#define GPUDRIVE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_OK 0
#define GD_ERR_INVALID (-1)   /* bad argument */
#define GD_ERR_IO (-2)        /* scene file missing / unreadable (reference: assert, src/MapReader.cpp:40) */
#define GD_ERR_PARSE (-3)     /* malformed scene JSON (reference: nlohmann exception -> abort) */
/* After gd_create, gd_set_maps or gd_delete_agents returns GD_ERR_DEVICE (e.g. the device is out of memory in the middle
 * of a rebuild) the worlds are not in a usable state: the only supported calls on that simulator are gd_destroy and
 * gd_last_error.  gd_destroy is always safe: the engine never keeps a device address it has returned. */
#define GD_ERR_DEVICE (-4)    /* HIP runtime failure, no gfx950 device */
#define GD_ERR_UNSUPPORTED (-5)

/* src/consts.hpp:11-13,34,37 */
#define GD_MAX_AGENTS_LIMIT 128
#define GD_MAX_ROAD_ENTITIES 10000
#define GD_MAP_OBS_K 200
#define GD_EPISODE_LEN 91
#define GD_NUM_LIDAR_SAMPLES 50
#define GD_TRAJECTORY_FLOATS 1456   /* src/types.hpp:373 */
#define GD_BEV_RES 200
#define GD_VEHICLE_SCALE 0.7f       /* src/consts.hpp:25 */

/* src/init.hpp:76-109 enums (values as seen through src/bindings.cpp:31-88) */
enum { GD_REWARD_DISTANCE_BASED = 0, GD_REWARD_ON_GOAL_ACHIEVED = 1, GD_REWARD_DENSE = 2 };
enum { GD_COLLISION_AGENT_STOP = 0, GD_COLLISION_AGENT_REMOVED = 1, GD_COLLISION_IGNORE = 2 };
enum { GD_DYNAMICS_CLASSIC = 0, GD_DYNAMICS_INVERTIBLE_BICYCLE = 1, GD_DYNAMICS_DELTA_LOCAL = 2,
       GD_DYNAMICS_STATE = 3 };
enum { GD_ROADS_K_NEAREST = 0, GD_ROADS_ALL_WITHIN_RADIUS = 1 };

/* src/init.hpp:111-127 `Parameters` (+ RewardParams :83-88), field for field. */
typedef struct gd_params {
    float polylineReductionThreshold;
    float observationRadius;
    int32_t rewardType;
    float distanceToGoalThreshold;
    float distanceToExpertThreshold;
    int32_t collisionBehaviour;          /* default AgentStop */
    uint32_t maxNumControlledAgents;     /* default 10000 */
    int32_t IgnoreNonVehicles;           /* default 0 */
    int32_t roadObservationAlgorithm;    /* default K nearest */
    int32_t initOnlyValidAgentsAtFirstStep; /* default 1 */
    int32_t isStaticAgentControlled;     /* default 0 */
    int32_t enableLidar;                 /* default 0 */
    int32_t disableClassicalObs;         /* default 0 */
    int32_t dynamicsModel;               /* default Classic */
    int32_t readFromTracksToPredict;     /* default 0 */
} gd_params;

/* Export slots: src/sim.hpp:17-45 `ExportID`, in the order of the getters of src/bindings.cpp:109-149. */
enum {
    GD_T_ACTION = 0,          /* action_tensor                   f32 [W,A,10]        mgr.cpp:718 */
    GD_T_REWARD,              /* reward_tensor                   f32 [W,A,1]         mgr.cpp:729 */
    GD_T_DONE,                /* done_tensor                     i32 [W,A,1]         mgr.cpp:749 */
    GD_T_INFO,                /* info_tensor                     i32 [W,A,5]         mgr.cpp:759 */
    GD_T_SELF_OBS,            /* self_observation_tensor         f32 [W,A,8]         mgr.cpp:769 */
    GD_T_ABS_OBS,             /* absolute_self_observation_tensor f32 [W,A,14]       mgr.cpp:865 */
    GD_T_PARTNER_OBS,         /* partner_observations_tensor     f32 [W,A,A-1,9]     mgr.cpp:792 */
    GD_T_AGENT_MAP_OBS,       /* agent_roadmap_tensor            f32 [W,A,200,9]     mgr.cpp:804 */
    GD_T_MAP_OBS,             /* map_observation_tensor          f32 [W,10000,9]     mgr.cpp:780 */
    GD_T_LIDAR,               /* lidar_tensor                    f32 [W,A,3,50,4]    mgr.cpp:817 */
    GD_T_BEV,                 /* bev_observation_tensor          f32 [W,A,200,200,1] mgr.cpp:829 (lazy) */
    GD_T_STEPS_REMAINING,     /* steps_remaining_tensor          i32 [W,A,1]         mgr.cpp:841 */
    GD_T_SHAPE,               /* shape_tensor                    i32 [W,2]           mgr.cpp:852 */
    GD_T_CONTROLLED_STATE,    /* controlled_state_tensor         i32 [W,A,1]         mgr.cpp:857 */
    GD_T_RESPONSE_TYPE,       /* response_type_tensor            i32 [W,A,1]         mgr.cpp:861 */
    GD_T_EXPERT_TRAJECTORY,   /* expert_trajectory_tensor        f32 [W,A,1456]      mgr.cpp:877 */
    GD_T_WORLD_MEANS,         /* world_means_tensor              f32 [W,3]           mgr.cpp:739 */
    GD_T_METADATA,            /* metadata_tensor                 i32 [W,A,4]         mgr.cpp:897 */
    GD_T_DELETED_AGENTS,      /* deleted_agents_tensor           i32 [W,A]           mgr.cpp:656 */
    GD_T_MAP_NAME,            /* map_name_tensor                 i32 [W,32]          mgr.cpp:883 */
    GD_T_SCENARIO_ID,         /* scenario_id_tensor              i32 [W,32]          mgr.cpp:890 */
    GD_T_COUNT
};

enum { GD_DTYPE_F32 = 0, GD_DTYPE_I32 = 1 };

typedef struct gd_tensor_desc {
    void *data;        /* device pointer (NULL from gd_tensor_shape) */
    int32_t dtype;     /* GD_DTYPE_* */
    int32_t ndim;
    int64_t dims[5];
    int64_t nbytes;
} gd_tensor_desc;

/* How the k-NN road observation orders its rows. */
enum {
    GD_KNN_REFERENCE_ORDER = 0, /* rows in the reference's SGI-heap array order (src/knn.hpp:103-158) */
    GD_KNN_SET_ORDER = 1        /* same row SET, in a fixed order of the engine's own (grid cell by grid cell); NOT elementwise identical */
};

/* Manager::Config (src/mgr.hpp:30-44) minus the render fields, plus engine knobs. */
typedef struct gd_config {
    int32_t num_worlds;         /* = len(scenes) */
    int32_t max_agents;         /* consts::kMaxAgentCount: 64 (benchmark configs) or 128 (this fork) */
    int32_t device_id;          /* Config::gpuID */
    void *stream;               /* hipStream_t to launch on; NULL = the null stream */
    int32_t knn_order;          /* GD_KNN_* */
    int32_t alloc_bev;          /* 1: allocate + compute the BEV tensor (160 KB/agent) */
    float lidar_half_angle;     /* consts::lidarAngle; 0 -> pi/3 (reference), pi -> 360 degrees */
    void *external[GD_T_COUNT]; /* caller-owned device buffers per export slot, or NULL */
} gd_config;

typedef struct gd_sim gd_sim;

/* Library identity / capability probes (no device access). */
const char *gd_version(void);
const char *gd_last_error(void);
void gd_default_params(gd_params *out);                   /* src/init.hpp:111-127 defaults */

/* Shape/dtype of export slot `id` for (num_worlds, max_agents); data = NULL.  Lets the caller
 * allocate storage before gd_create.  Replaces the dims lists of src/mgr.cpp:656-902. */
int gd_tensor_shape(int32_t id, int32_t num_worlds, int32_t max_agents, gd_tensor_desc *out);

/* Manager::Manager (src/mgr.cpp:565; bindings.cpp:93-108): parse `scenes`, build every world,
 * upload, and run the Reset task graph once so that all tensors hold t = 0 state. */
int gd_create(const gd_config *cfg, const gd_params *params, const char *const *scenes, gd_sim **out);
/* Manager::~Manager */
void gd_destroy(gd_sim *sim);

/* Manager::step (src/mgr.cpp:569-580): movement -> collision -> reward -> --t -> done -> obs.
 * Launches on cfg.stream and returns without synchronising (stream order = data order). */
int gd_step(gd_sim *sim);
/* Manager::reset (src/mgr.cpp:582-588): flag the listed worlds, run the Reset graph for ALL worlds. */
int gd_reset(gd_sim *sim, const int32_t *world_indices, int32_t n);
/* Manager::setMaps (src/mgr.cpp:590-654): n must equal num_worlds. */
int gd_set_maps(gd_sim *sim, const char *const *scenes, int32_t n);
/* Manager::deleteAgents (src/mgr.cpp:665-715): CSR lists; ids[offsets[i]..offsets[i+1]) for worlds[i]. */
int gd_delete_agents(gd_sim *sim, const int32_t *worlds, const int32_t *offsets, const int32_t *ids,
                     int32_t n_worlds);
/* Manager::*Tensor() (src/mgr.cpp:656-902). */
int gd_tensor(gd_sim *sim, int32_t id, gd_tensor_desc *out);
/* Fused observation pack: writes what GPUDriveTorchEnv.get_obs() concatenates with
 * norm_obs=True (gpudrive/env/env_torch.py:756-896,1172-1216) for every agent slot:
 * out[W][A][6 + (A-1)*6 + 200*13] f32 = ego | partners | road points (type one-hot over 7).
 * `out` is a device pointer of at least out_bytes bytes. */
int gd_pack_observations(gd_sim *sim, float *out, int64_t out_bytes);
/* The same tensor written WHERE THE ROWS ARE PRODUCED instead of by a second pass over the exported tensors: from this call on
 * every step / reset pass writes the live agents' packed rows straight into `out` (k_world_step: ego + partner columns; the
 * road kernel: the 200 x 13 road columns), bit-identical to gd_pack_observations on the same state; `out` must stay valid
 * until it is detached (out = NULL) or the simulator is destroyed.  only != 0: the raw partner_observations and
 * agent_roadmap rows of live agents are no longer written (for a learner that reads nothing but the packed tensor --
 * gpudrive/env/env_torch.py:756-896 is the only consumer of those rows in the reference's PPO loop); only = 0 keeps them.
 * Every road path writes them (the linear scan, the fused set-order kernel, k_map_rows behind the reference-order
 * selections); GD_ERR_UNSUPPORTED only with disableClassicalObs or the developer switch GPUDRIVE_LINEAR_LEGACY=1.  With a
 * buffer attached gd_pack_observations is a no-op for that buffer and a device copy for any other. */
int gd_attach_packed(gd_sim *sim, float *out, int64_t out_bytes, int32_t only);
/* The packed observation of the reward-conditioned policy (env_torch.py:756-810; gpudrive/networks/late_fusion.py:104-110):
 * out[W][A][D + 3] f32 = ego(6) | weights[w][a][0..3) | partners (A-1) x 6 | road points 200 x 13, D as above; every column
 * but the three inserted ones bit-identical to gd_pack_observations on the same state.  `weights` is a device pointer to
 * [W][A][3] f32 (EpisodeTracker.reward_weights_tensor).  Written from the raw tensors, or -- while a buffer is attached with
 * gd_attach_packed -- by a copy of that buffer that inserts the three columns (with only != 0 the raw rows are stale). */
int gd_pack_observations_conditioned(gd_sim *sim, const float *weights, float *out, int64_t out_bytes);
/* Learner rows: the flat, controlled-agent-only view of the reference's PPO loop (gpudrive/env/env_puffer.py:235-403), which
 * hands the policy obs[controlled_agent_mask] as [N, D] and takes one discrete action index per row.  `mask` is a device
 * [W][A] bool (uint8); the learner rows are its true slots in row-major (world, agent) order -- the order of torch's boolean
 * indexing.  The engine builds the maps slot -> row and row -> slot on the device, reads the row count back once (a setup call:
 * it synchronises) and returns GD_ERR_INVALID, with no rows set, when it differs from n_rows.  mask = NULL clears the rows;
 * n_rows = 0 is legal.  The map stays as it is until the next call: set_maps, gd_delete_agents and resets do not change it
 * (the reference captures controlled_agent_mask once and re-derives it in resample_scenario_batch, env_puffer.py:438-453;
 * after gd_set_maps the caller sets the rows again).  Setting or clearing the rows detaches a gd_attach_packed_rows buffer. */
int gd_set_learner_rows(gd_sim *sim, const uint8_t *mask, int32_t n_rows);
/* gd_attach_packed for the learner rows only: out is [n_rows][D], D as above, and from this call on every step / reset pass
 * writes learner row r at out + r * D -- bit-identical to row slot_of_row[r] of gd_pack_observations on the same state -- and
 * no packed row for any other slot (with only != 0 the other slots' road rows are not even selected by the linear scan).
 * One packed buffer exists at a time: this call and gd_attach_packed replace each other, gd_attach_packed(sim, NULL, 0, 0)
 * detaches either kind, and gd_set_learner_rows detaches this kind.  While attached, gd_pack_observations and
 * gd_pack_observations_conditioned work from the raw tensors with only = 0 and return GD_ERR_UNSUPPORTED with only != 0 (the
 * raw rows are stale, and there is no [W][A][D] buffer to copy from).  GD_ERR_INVALID without learner rows;
 * GD_ERR_UNSUPPORTED where gd_attach_packed is. */
int gd_attach_packed_rows(gd_sim *sim, float *out, int64_t out_bytes, int32_t only);
/* gd_attach_packed_rows for the reward-conditioned policy: out is [n_rows][D + 3] f32, contiguous, and learner row r is row
 * slot_of_row[r] of gd_pack_observations_conditioned(weights) bit for bit -- ego 6 | the slot's 3 weights | partners | road
 * points -- after every step and every reset pass.  weights: the [W][A][3] device tensor the episode tracker keeps
 * (gd_episode_buffers.reward_weights); gd_episode_step's redraw of reset worlds and gd_episode_draw_weights given that same
 * pointer also rewrite the weight columns of the learner rows of the worlds they draw.  Weights changed any other way reach
 * a row when its head is next written.  Every other rule of gd_attach_packed_rows applies; weights = NULL is GD_ERR_INVALID. */
int gd_attach_packed_rows_conditioned(gd_sim *sim, float *out, int64_t out_bytes, int32_t only, const float *weights);
/* Discrete actions decoded on the device: action[slot_of_row[r]][0..3) = table[indices[r]] for every learner row r, what
 * _apply_actions + _copy_actions_to_simulator do with a [N] index tensor for classic, bicycle and delta_local
 * (gpudrive/env/env_torch.py:615-664).  indices: device int64 [n_rows]; table: device f32 [n_actions][3].  Other slots are
 * left untouched (the simulator ignores the actions of uncontrolled agents).  An index outside [0, n_actions) leaves its row's
 * action as it was and is counted (gd_stat 45).  Launched on the simulator's stream, outside the captured step graph.
 * GD_ERR_UNSUPPORTED for the State dynamics model (no discrete space in the reference); GD_ERR_INVALID without learner rows. */
int gd_set_discrete_actions(gd_sim *sim, const int64_t *indices, const float *table, int32_t n_actions);
/* Expert-action export: GPUDriveTorchEnv.get_expert_actions()
 * (gpudrive/env/env_torch.py:1445-1509 over gpudrive/datatypes/trajectory.py:24-41) in one pass over the
 * expert trajectory rows.  Device pointers, any of them may be NULL:
 *   actions f32 [W][A][91][cols]  cols = 10 for DynamicsModel::State, else 3 (clamped per model)
 *   pos_xy  f32 [W][A][91][2], vel_xy f32 [W][A][91][2], yaw f32 [W][A][91][1], valids i32 [W][A][91][1]
 * `action_cols` must match the simulator's dynamics model (GD_ERR_INVALID otherwise). */
int gd_expert_actions(gd_sim *sim, float *actions, int32_t action_cols, float *pos_xy, float *vel_xy, float *yaw,
                      int32_t *valids);
/* GPUDriveTorchEnv.advance_sim_with_log_playback(init_steps) (gpudrive/env/env_torch.py:1274-1293): for
 * t = 0 .. init_steps-1 write the expert action of step t into action[:, :, :cols] of every agent slot
 * (env_torch.py:645-664) and step.  init_steps >= 91 is GD_ERR_INVALID (the reference raises ValueError). */
int gd_advance_log_playback(gd_sim *sim, int32_t init_steps);
/* Expert trajectory recorder: the imitation-learning dataset of save_trajectory (gpudrive/integrations/il/storage.py:10-109;
 * read by baselines/il/il.py:71-84) written on the device.  Replaces its Python loop over every controlled agent inside the
 * loop over 91 steps (storage.py:47-56: seven indexed tensor copies per agent and step) and the per-step get_dones / get_obs /
 * get_road_mask / get_partner_mask / get_infos round trips (storage.py:60-80) by one kernel launch per time index between the
 * steps of a log playback, with no host synchronisation inside the episode.  All pointers are device pointers owned by the
 * caller; N = n_rows, A = max_agents, D = 6 + (A-1)*6 + 200*13; the time pitch is always 91.  The caller fills the defaults of
 * storage.py:29-35 first (obs / actions / global 0, dead_mask 1, partner_mask 2, road_mask 1) and zeroes the running state:
 * only live rows are written. */
typedef struct gd_record_buffers {
    const int32_t *row_slot;  /* [N] world * A + agent of every recorded row (cont_agent_mask.nonzero() order, storage.py:25);
                               * a value outside [0, W * A) leaves its row untouched */
    int32_t n_rows;
    float *obs;               /* [N][91][D] the packed observation, bit for bit row row_slot[n] of gd_pack_observations */
    float *actions;           /* [N][91][3] the logged action fed at that step (gd_expert_actions' columns) */
    uint8_t *dead_mask;       /* [N][91] bool: the row was done BEFORE step t (storage.py:56) */
    uint8_t *partner_mask;    /* [N][91][A-1] 0 a partner that acts, 1 a Static one with a non-zero packed row, 2 nobody
                               * (env_torch.py:1224-1253) */
    uint8_t *road_mask;       /* [N][91][200] bool: road row is padding (id -1, env_torch.py:1255-1272) */
    float *ego_global_pos;    /* [N][91][2] absolute_self_observation columns 0, 1 */
    float *ego_global_rot;    /* [N][91][1] absolute_self_observation column 7 */
    /* running state, read and written: zero before the call */
    uint8_t *dead;            /* [N] */
    float *goal_achieved, *off_road, *veh_collision;  /* [N] sums of info columns 3 / 0 / 1 + 2, clamped to 1 (storage.py:75-80) */
    int32_t *any_alive;       /* [92] 1 where some recorded row was alive before step t: iteration t of the reference's loop
                               * exists (its `break`, storage.py:82-89); their sum is the number of iterations it runs */
    /* optional diagnostic, HOST pointer: the summed duration of the recorder's launches in ms from events around each of
     * them.  Non-NULL makes the call synchronise at its end. */
    float *kernel_ms;
} gd_record_buffers;
/* For t in [0, n_steps): record time index t, write the logged action of step t into every agent slot (what
 * gd_advance_log_playback does) and step; then the bookkeeping of the last step.  With n_steps < 91 the result is the prefix
 * [0, n_steps) of the full recording (dead flags and accumulators as they stand after n_steps steps).  It does not reset: the
 * caller does.  GD_ERR_INVALID: a null pointer, n_rows < 0, n_steps outside [1, 91], the State dynamics model (its actions
 * have 10 columns; the dataset's have 3).  GD_ERR_UNSUPPORTED while a packed buffer is attached with only != 0 (the raw rows
 * the observation is computed from are stale). */
int gd_record_expert(gd_sim *sim, const gd_record_buffers *buffers, int32_t n_steps);
/* Device expert dataset: the consumer of the recorder's arrays.  Replaces the reference's ExpertDataset
 * (gpudrive/integrations/il/dataloader.py:5-71, 183-211; built and iterated by baselines/il/il.py:70-97, unpacked by
 * il.py:248-263): its padded second copy of every array (dataloader.py:10, 46-54), its Python list of valid (row, time)
 * pairs (dataloader.py:66-71) and the per-sample slicing in DataLoader workers (dataloader.py:183-205), by an index built on
 * the device and one kernel that gathers a batch.  Needs no simulator: every pointer is a device pointer owned by the caller,
 * `stream` is a hipStream_t (NULL: the default stream).  T = 91, A = max_agents (64 or 128), D = 6 + (A-1)*6 + 200*13,
 * R = rollout_len, P = pred_len with R >= 1, P >= 1, R + P <= 91 (outside it the reference switches to an unrelated flat mode).
 * A shard is one recorded episode batch; shards are never concatenated. */
#define GD_IL_MAX_SHARDS 8
typedef struct gd_il_shard {
    const float *obs;             /* [n_rows][91][D], 16-byte aligned */
    const float *actions;         /* [n_rows][91][3] */
    const uint8_t *dead_mask;     /* [n_rows][91] bool */
    const uint8_t *partner_mask;  /* [n_rows][91][A-1] 0 / 1 / 2 */
    const uint8_t *road_mask;     /* [n_rows][91][200] bool, 8-byte aligned */
    const uint8_t *keep;          /* [n_rows] bool: the rows ExpertEpisode.save() writes (storage.py:86-98) */
    int32_t n_rows;
} gd_il_shard;
typedef struct gd_il_dataset {
    gd_il_shard shard[GD_IL_MAX_SHARDS];
    int32_t n_shards;             /* 0..8 */
    int32_t max_agents;           /* 64 or 128 */
    int32_t rollout_len, pred_len;
} gd_il_dataset;
/* The valid-sample index (dataloader.py:16-23, 66-71), in two launches with the caller's prefix sums between them.  A source
 * row is a (shard, local row) pair; g counts them through the shards in order.  valid[g][t] = !dead_mask && !(|a1| > 0.5f ||
 * |a0| > 5.f || |a2| > 0.2f) (strict, fp32; a NaN does not invalidate).  The samples of row g are the idx2 in [0, 91 - P] with
 * keep[g] && valid[g][idx2 + P - 1], ascending.
 *   entries == NULL: counts[g] = the number of samples of row g, kept[g] = keep[g] (both int32 [rows]).
 *   entries != NULL: entry_offset[g] (int64: the exclusive prefix sum of counts) and kept_ordinal[g] (int64: the exclusive
 *       prefix sum of kept, idx1 of the reference after save() dropped the other rows) are read, and row g's entries written
 *       at entries[entry_offset[g] ...] as int32 x 4 {shard, local row, idx2, idx1}.
 * GD_ERR_INVALID: a null pointer, R / P out of range, A not 64 or 128, a negative row count, more than 8 shards, a
 * misaligned obs or road_mask. */
int gd_il_index(const gd_il_dataset *ds, int32_t *counts, int32_t *kept, const int64_t *entry_offset,
                const int64_t *kept_ordinal, int32_t *entries, void *stream);
typedef struct gd_il_batch_buffers {
    const int32_t *entries;   /* [n_entries][4] gd_il_index's */
    int64_t n_entries;
    const int64_t *sel;       /* [batch] positions into entries, any order, repeats allowed */
    int32_t batch;
    int32_t *bad_indices;     /* [1] incremented once for every sel outside [0, n_entries) */
    /* outputs; every byte of each is written by every call */
    float *obs;               /* [batch][R][D] rows at times idx2 - R + 1 .. idx2, zeros where the time is < 0; 16-byte aligned */
    float *actions;           /* [batch][P][3] actions at times idx2 .. idx2 + P - 1 */
    uint8_t *partner_mask;    /* [batch][R][A-1] bool: stored value == 2; true where the time is < 0.  Any alignment */
    uint8_t *road_mask;       /* [batch][R][200] bool; true where the time is < 0; 8-byte aligned */
    int64_t *data_idx;        /* [batch][2] (idx1, idx2) */
} gd_il_batch_buffers;
/* One training batch (dataloader.py:183-205 for every sample, then the DataLoader's collate and the copy to the device):
 * one launch, no host synchronisation.  A sel outside [0, n_entries) gives an all-padding sample (obs 0, actions 0, masks
 * true, data_idx (-1, -1)) and counts in bad_indices.  GD_ERR_INVALID as above, and for batch < 0, batch > 2^25 - 1 or
 * n_entries < 0. */
int gd_il_batch(const gd_il_dataset *ds, const gd_il_batch_buffers *buffers, void *stream);
/* Linear-probing batches from the same recording and the same index: the reference's FutureDataset
 * (gpudrive/integrations/il/linear_probing/dataloader.py:6-230; unpacked by baselines/il/linear_probing.py:173) without its
 * padded copy of obs, its [N][91][A-1] arrays of transformed positions and its per-sample slicing.  A label is computed per
 * sample inside the gather, in fp32 in the reference's operation order (no fused multiply-add, correctly rounded division,
 * cos / sin evaluated in double and rounded once).  F = future_step, (n, idx2) the sample's source row and current time,
 * valid[n][t] gd_il_index's flag, pos / rot the ego's recorded pose (gd_record_buffers' ego_global_pos / ego_global_rot).
 *   cls(v, b)  = clamp(#{i : b[i] <= (double)v} - 1, 0, 7); a NaN v gives 7 (numpy.digitize)
 *   label(x, y) = cls(x, xbins) * 8 + cls(y, ybins);  norm(v) = 2 * ((v - (-1000)) / 2000) - 1
 *   GD_IL_FUTURE_EGO: future_mask [batch] = valid[n][idx2] && idx2 + F < 91 && valid[n][idx2 + F]; future_pos [batch] =
 *     label(0, 0) where idx2 + F >= 91, else with d = pos[idx2 + F] - pos[idx2], c = cos(rot[idx2]), s = sin(rot[idx2]):
 *     label(norm(d.x * c + d.y * s), norm((-d.x) * s + d.y * c)).
 *   GD_IL_FUTURE_OTHER, per partner column j: future_mask [batch][A-1] = partner_mask[n][idx2][j] != 0 || idx2 + F >= 91 ||
 *     partner_mask[n][idx2 + F][j] != 0; future_pos [batch][A-1] = label(0, 0) where the mask is true, else with
 *     p = obs[n][idx2 + F][6 + 6j + 1 .. + 3) * 1000, e = pos[idx2 + F], c / s = cos / sin(rot[idx2 + F]):
 *     g = ((e.x + p.x * c) - p.y * s, (e.y + p.x * s) + p.y * c), d = g - pos[idx2], c2 / s2 = cos / sin(-rot[idx2]):
 *     label(norm(d.x * c2 + d.y * s2), norm((-d.x) * s2 + d.y * c2)) -- the reference's rotation by +rot[idx2]
 *     (dataloader.py:105-109), reproduced. */
enum { GD_IL_FUTURE_OTHER = 0,  /* exp='other': the partners' positions F steps ahead, in the ego's current frame */
       GD_IL_FUTURE_EGO = 1 };  /* exp='ego': the ego's own displacement over F steps */
typedef struct gd_il_future {
    const float *ego_global_pos[GD_IL_MAX_SHARDS];  /* per shard of the dataset: [n_rows][91][2] */
    const float *ego_global_rot[GD_IL_MAX_SHARDS];  /* per shard of the dataset: [n_rows][91][1] */
    int32_t future_step;          /* F, 1..90 */
    int32_t exp;                  /* GD_IL_FUTURE_* */
    double xbins[9], ybins[9];    /* the bin edges, strictly increasing (numpy.linspace(lo, hi, 9); the reference's default
                                   * is (-0.05, 0.05) for both) */
} gd_il_future;
typedef struct gd_il_future_buffers {
    const int32_t *entries;   /* as gd_il_batch_buffers */
    int64_t n_entries;
    const int64_t *sel;
    int32_t batch;
    int32_t *bad_indices;
    /* outputs, in the order linear_probing.py:173 unpacks them; every byte of each is written by every call */
    float *obs;               /* [batch][R][D] as gd_il_batch's, bit for bit; 16-byte aligned */
    float *actions;           /* [batch][P][3] as gd_il_batch's */
    uint8_t *valid_mask;      /* [batch] bool: valid[n][idx2 + P - 1] (true for every sample of the index) */
    uint8_t *ego_mask;        /* [batch][R] bool: valid[n][idx2 - R + 1 + r], false where the time is < 0 */
    uint8_t *partner_mask;    /* [batch][R][A-1] bool as gd_il_batch's.  Any alignment */
    uint8_t *road_mask;       /* [batch][R][200] bool as gd_il_batch's; 8-byte aligned */
    uint8_t *future_mask;     /* OTHER: [batch][A-1] bool (aux_mask), any alignment; EGO: [batch] bool (future_valid_mask) */
    int64_t *future_pos;      /* OTHER: [batch][A-1] (other_pos); EGO: [batch] (ego_pos); classes 0..63 */
} gd_il_future_buffers;
/* One linear-probing batch: one launch, no host synchronisation.  A sel outside [0, n_entries) gives gd_il_batch's padding
 * in obs, actions, partner_mask and road_mask, false in valid_mask, ego_mask and the EGO future_mask, true in the OTHER
 * future_mask, label(0, 0) in future_pos, and counts in bad_indices.  GD_ERR_INVALID as gd_il_batch, and for a null pose
 * pointer of a shard, F outside [1, 90], an unknown exp, and bin edges that are not finite and strictly increasing. */
int gd_il_future_batch(const gd_il_dataset *ds, const gd_il_future *future, const gd_il_future_buffers *buffers, void *stream);
/* Device rollout buffer: the consumer of the learner rows on the PPO side.  Replaces the reference's Experience and
 * compute_gae (gpudrive/integrations/puffer/ppo.py:530-666, used by ppo.py:108-260): store's host copy of the live indices
 * and of five arrays per step (ppo.py:606-620), the Python sorted() over (env_id, step) tuples (ppo.py:622-644), the serial
 * host loop of the advantages (ppo.py:239-245) and flatten_batch's copies back to the device (ppo.py:646-666).  Needs no
 * simulator: every pointer is a device pointer owned by the caller, `stream` is a hipStream_t (NULL: the default stream).
 * B = batch_size, N = num_rows, D = obs_width (any positive width), AW = action_width (the product of the action shape, 1 for
 * a scalar action).  env_id[i] = i: row i of a step's inputs is environment i. */
typedef struct gd_rollout {
    int32_t batch_size, num_rows, obs_width, action_width;
    /* the storage, in the order the entries were stored */
    float *obs;        /* [B][D]; 16-byte pieces are used where D % 4 == 0 and the pointer is 16-byte aligned */
    int64_t *actions;  /* [B][AW] */
    float *logprobs;   /* [B] */
    float *rewards;    /* [B] */
    float *dones;      /* [B] 0.0f or 1.0f */
    float *values;     /* [B] */
    int32_t *row;      /* [B] the entry's row (env_id) */
    int32_t *ord;      /* [B] how many entries of that row were stored before it in this rollout */
    int32_t *count;    /* [N] entries of each row in this rollout */
    int32_t *dst;      /* [N] scratch of one store: the storage position of each row, -1 where nothing is stored */
    int32_t *state;    /* [4] ptr, step, dropped (live rows that did not fit, never reset), bad_positions (positions outside
                        * [0, B) met by sort, gae or gather, never reset; 0 unless a caller hands in a foreign idxs) */
} gd_rollout;
/* One step (ppo.py:606-620): the live rows are the i with mask[i] != 0, ascending, cut to the first B - ptr of them; they
 * land at [ptr, ptr + k) in that order.  ptr += k, step += 1 (also when nothing is live), dropped += the live rows that did
 * not fit.  Two launches, no host synchronisation, no atomics: one workgroup scans the mask and writes dst, the scalars, row,
 * ord and count, then a workgroup per row copies its D floats.  The inputs are read when the launches run: enqueue the call
 * before whatever overwrites them on the same stream.  obs [N][D], value / logprob / reward [N], action [N][AW] int64,
 * done / mask [N] bool.  streaming != 0: the observation rows are stored non-temporally.  GD_ERR_INVALID: a null pointer, a
 * size < 1, num_rows > 2^20, B > 2^22 (every kernel covers the batch with one launch), B * max(D, AW) > 2^40. */
int gd_rollout_store(const gd_rollout *ro, const float *obs, const float *value, const int64_t *action, const float *logprob,
                     const float *reward, const uint8_t *done, const uint8_t *mask, int32_t streaming, void *stream);
/* The permutation of ppo.py:622-625, sorted by (row, step), without a sort: idxs[offset[row[p]] + ord[p]] = p for every
 * p in [0, B), with offset [N] int64 the exclusive prefix sum of count (the caller's, as gd_il_index's offsets are).  Then
 * ptr = 0, step = 0 and count[] = 0 (ppo.py:641-643).  The storage must be full (ptr == B): the caller checks.  One launch. */
int gd_rollout_sort(const gd_rollout *ro, const int64_t *offset, int64_t *idxs, void *stream);
/* The advantages in sorted order (ppo.py:239-245), [B] float32: the rule of csrc/gae_chain.hpp, which states the operation
 * order and the two float corner cases in which cutting the chain at a done differs from the serial loop.  gamma and
 * gae_lambda are float32 already.  delta, coef: [B] float32 scratch, written whole.  Two launches: the terms through idxs,
 * then one chain per run between dones; no workgroup waits on another.  A batch without a done is one chain of B, walked by
 * one lane.  GD_ERR_INVALID: a null pointer, gamma or gae_lambda not finite. */
int gd_rollout_gae(const gd_rollout *ro, const int64_t *idxs, float gamma, float gae_lambda, float *delta, float *coef,
                   float *advantages, void *stream);
typedef struct gd_rollout_batch {
    const int64_t *idxs;        /* [B] gd_rollout_sort's */
    const float *advantages;    /* [B] gd_rollout_gae's, in sorted order */
    int32_t num_minibatches, minibatch_rows, bptt_horizon;  /* B = num_minibatches * minibatch_rows * bptt_horizon */
    int32_t first, n;           /* the minibatches [first, first + n) are gathered */
    int32_t split;              /* workgroups per sample, 1..64; 0: the default */
    /* outputs, [n][minibatch_rows][bptt_horizon] each; every byte of each is written by every call */
    float *obs;                 /* [..][D]; 16-byte pieces where D % 4 == 0 and both obs pointers are 16-byte aligned */
    int64_t *actions;           /* [..][AW] */
    float *logprobs, *dones, *values, *advantages_out, *returns;
} gd_rollout_batch;
/* Minibatches as flatten_batch lays them out (ppo.py:646-666): sample (m, r, h) has the sorted position
 * s = (r * num_minibatches + first + m) * bptt_horizon + h and the storage position p = idxs[s]; it takes obs, actions,
 * logprobs, dones and values at p, advantages at s, and returns = advantages[s] + values[p] (one fp32 add).  One launch, no
 * host synchronisation.  A p outside [0, B) gives zeros and counts in state[3].  GD_ERR_INVALID: a null pointer, sizes that
 * do not multiply to B, [first, first + n) outside the minibatches, split outside 0..64, samples * split >= 2^24. */
int gd_rollout_gather(const gd_rollout *ro, const gd_rollout_batch *batch, void *stream);
/* Device policy forward: the producer of actions, logprobs and values between the learner step and the rollout buffer.
 * Replaces the reference's NeuralNet.forward under no_grad (gpudrive/networks/late_fusion.py:170-210, called by
 * gpudrive/integrations/puffer/ppo.py:150-160) and its chain of torch operators over [N][200][64] and [N][A-1][64]
 * intermediates.  Needs no simulator: every pointer is a device pointer owned by the caller, `stream` is a hipStream_t.
 * N = num_rows, A = max_agents, EW = ego_width, NA = n_actions, D = EW + 6 (A - 1) + 200 * 13.
 *
 * The network rule (float32 throughout; the module in EVAL mode, dropout is the identity):
 *   ego      = L2e(tanh(LN(L1e(obs[0 .. EW)))))                                        [64]
 *   partner  = max over ALL A - 1 rows j of L2p(tanh(LN(L1p(obs[EW + 6 j .. + 6)))))   [64]  (padding rows included)
 *   road     = max over ALL 200 rows j of L2r(tanh(LN(L1r(obs[EW + 6 (A-1) + 13 j .. + 13)))))   [64]
 *   hidden   = Ws [ego, partner, road] + bs                                            [128] (no activation)
 *   logits   = Wa hidden + ba   [NA];   value = Wc hidden + bc
 *   LN(x)    = (x - mean) * (1 / sqrt(var + 1e-5)) * g + b, var the biased variance, sqrt and division correctly rounded.
 * The matrix products are v_mfma_f32_32x32x2_f32 chains (one fmaf per term, float32 in and out); the summation order
 * differs from a BLAS's, the precision does not.  Observations must be finite.
 *
 * The action rule is csrc/policy_rule.hpp, stated there in full: with m = max l, p[k] = expf(l[k] - m) and S the sum of p in
 * ascending k, the sampled action is the first k whose running sum exceeds u[row] * S (the last k if none does), the
 * deterministic action is the first index of the maximum; logprob = (l[a] - m) - logf(S); entropy = -sum q exp(q) with
 * q = l - m - logf(S).
 *
 * blob: the weights packed once in the order the kernels read them (gpudrive_lab_amd/policy.py `pack_index` is the
 * statement of the layout; acc(r, h) = (r & 3) + 8 (r >> 2) + 4 h is the accumulator row of register r in lane half h,
 * lane = 0..63, h = lane >> 5, c = lane & 31), in floats, in this order:
 *   ego:      W1 [64][EW], b1 [64], g [64], b [64], W2 transposed [in 64][out 64], b2 [64]
 *   partner:  W1 as [t 2][s 3][lane] = W1[32 t + c][3 h + s];  b1, g, b [64];  W2 as [t2 2][t 2][r 16][lane] =
 *             W2[32 t2 + c][32 t + acc(r, h)];  b2 [64]
 *   road:     the same with [t 2][s 7][lane] = W1[32 t + c][7 h + s], zero where 7 h + s == 13
 *   shared:   Ws as [t 4][s 96][lane] = Ws[32 t + c][96 h + s];  bs [128]
 *   heads:    [actor; critic] (NA + 1 rows, zero rows up to T = ceil((NA + 1) / 32) tiles) as [i T][t 4][r 16][lane] =
 *             W[32 i + c][32 t + acc(r, h)];  the biases [32 T] */
typedef struct gd_policy {
    int32_t num_rows;     /* N, 1 .. 2^20 */
    int32_t max_agents;   /* A: 64 or 128 */
    int32_t ego_width;    /* 6, or 9 for reward-conditioned rows */
    int32_t n_actions;    /* 1 .. 1024 */
    const float *blob;    /* blob_floats floats, 16-byte aligned */
    int64_t blob_floats;  /* checked against the layout's size for (ego_width, n_actions) */
    float *features;      /* [N][192] scratch, 16-byte aligned: ego, partner, road */
    float *logits;        /* [N][NA] scratch: the logits the action rule reads */
} gd_policy;
/* One forward: three launches on `stream`, no host synchronisation, no allocation, no atomics.  obs [N][D] float32 at any
 * 4-byte alignment (rows of odd width start at every dword phase; entity rows are read with 4-byte loads).  u [N] float32 in
 * [0, 1), required unless deterministic != 0.  Outputs, every byte written by every call: actions [N] int64, logprob,
 * entropy, value [N] float32; logits_out [N][NA] float32, or NULL for not written.
 * GD_ERR_INVALID: a null pointer, max_agents not 64 or 128, ego_width not 6 or 9, n_actions outside [1, 1024], num_rows
 * outside [1, 2^20], blob_floats not the layout's size, a misaligned pointer. */
int gd_policy_forward(const gd_policy *p, const float *obs, const float *u, int32_t deterministic, int64_t *actions,
                      float *logprob, float *entropy, float *value, float *logits_out, void *stream);
/* Device policy backward: the training side of gd_policy -- the network's forward for GIVEN actions and its backward to
 * parameter gradients (the reference's `data.policy(obs, action=atn)` under autograd and `loss.backward()`,
 * gpudrive/integrations/puffer/ppo.py:261-332).  The loss arithmetic, advantage normalisation, gradient clipping and the
 * optimiser stay with the caller.  Every pointer is a device pointer owned by the caller; G = grad_floats is the number of
 * parameters; the flat layout of `params` and of `grad` is the state dict's: for ego, partner, road in turn W1 [64][K]
 * (K = EW, 6, 13), b1 [64], LayerNorm weight [64] and bias [64], W2 [64][64], b2 [64]; then Ws [128][192], bs [128],
 * Wa [NA][128], ba [NA], Wc [128], bc [1]; each row-major (gpudrive_lab_amd/policy.py `expected_shapes`). */
typedef struct gd_policy_grad {
    float *features;       /* [N][192], 16-byte aligned: written by evaluate, read by backward */
    float *logits;         /* [N][NA]: written by evaluate, read by backward */
    uint8_t *winners;      /* [N][128]: per pooled feature the entity that attained the max, 64 partner indices then 64 road
                            * indices.  Written by evaluate, read by backward */
    const float *params;   /* backward only: G floats, the weights in the flat layout above (the same values as p->blob) */
    float *rowstat;        /* backward only: [N][8] scratch */
    float *partials;       /* backward only: [num_partials][G] scratch */
    int64_t grad_floats;   /* backward only: G, checked against the parameter count for (ego_width, n_actions) */
    int32_t num_partials;  /* backward only: P, 1 .. 1024 */
    int32_t reserved;
} gd_policy_grad;
/* The training-side forward: the network, the blob and the arithmetic of gd_policy_forward (the same two kernels, so the
 * logits are bit-identical to its logits), then logprob and entropy of the GIVEN actions [N] int64 by the action rule's
 * formulas (csrc/policy_rule.hpp `evaluate`; nothing is drawn): evaluating the actions a forward sampled returns that
 * forward's logprob, entropy and value bit for bit.  An action outside [0, NA) is clamped into it, for memory safety only.
 * p->features and p->logits are not used: features, logits and winners go to g's buffers, every byte written by every call.
 * The winner of a pooled feature is the LOWEST entity index among the entities that attain the float32 maximum; padding rows
 * take part, as in the forward.  For finite observations every winner is below the set's size (A - 1, 200).  A pooled feature
 * that is NaN (non-finite observations are outside the contract) has no entity equal to its maximum: its winner is the
 * sentinel 255, which gd_policy_backward clamps to the set's last entity, for memory safety only.  Three launches on `stream`, no host synchronisation, no allocation, no atomics.
 * GD_ERR_INVALID: as gd_policy_forward, for p's ranges, null pointers and alignment. */
int gd_policy_evaluate(const gd_policy *p, const gd_policy_grad *g, const float *obs, const int64_t *actions, float *logprob,
                       float *entropy, float *value, void *stream);
/* The backward of one gd_policy_evaluate call with the same p, g, obs and actions: grad [G] float32 = the gradient, with
 * respect to every parameter, of sum_r (d_logprob[r] logprob[r] + d_entropy[r] entropy[r] + d_value[r] value[r]), the three
 * upstream gradients being float32 [N].  dlogits follow csrc/policy_grad_rule.hpp.  The max-pools pass a feature's gradient to
 * its recorded winner alone; obs gets no gradient.  Every element of grad, rowstat and partials is stored by every call;
 * nothing relies on a zeroed buffer.  The sums over rows are deterministic and use no atomics: workgroup p of P sums the rows
 * p, p + P, .. in ascending order into partials[p], and grad[e] = partials[0][e] + partials[1][e] + .. in that order, so the
 * bits depend on P but not on the run.  p->blob, p->features and p->logits are not used.  Three launches on `stream`, no host
 * synchronisation, no allocation.
 * GD_ERR_INVALID: a null pointer, p's ranges as in gd_policy_forward, num_partials outside [1, 1024], grad_floats not the
 * parameter count, a misaligned pointer. */
int gd_policy_backward(const gd_policy *p, const gd_policy_grad *g, const float *obs, const int64_t *actions,
                       const float *d_logprob, const float *d_entropy, const float *d_value, float *grad, void *stream);
/* Device PPO update: the rest of one minibatch update around gd_policy_evaluate and gd_policy_backward -- the reference's loss
 * with its three upstream gradients, clip_grad_norm_ and Adam (gpudrive/integrations/puffer/ppo.py:282-332).  The rule, with
 * every rounding and the order of every sum, is csrc/ppo_rule.hpp.  Every pointer is a device pointer owned by the caller, and
 * every value that changes between calls (the learning rate, the step count, the running products of the betas) lives on the
 * device, so a sequence of calls never depends on a host value that changes.  G = grad_floats, M = num_rows. */
typedef struct gd_ppo {
    int32_t num_rows;       /* M, 1 .. 2^20 (at least 2 with norm_adv) */
    int32_t ego_width;      /* 6 or 9: with n_actions it fixes G and the blob's size */
    int32_t n_actions;      /* 1 .. 1024 */
    int32_t norm_adv;       /* != 0: advantages normalised per minibatch */
    int32_t clip_vloss;     /* != 0: the clipped value loss */
    float clip_coef, vf_clip_coef, ent_coef, vf_coef;
    float max_grad_norm;    /* > 0 */
    float eps;              /* Adam's, > 0 */
    float stats_scale;      /* every call adds stats_scale * its statistics into stats_sum */
    double beta1, beta2;    /* in [0, 1) */
    int64_t grad_floats;    /* G, checked against the parameter count for (ego_width, n_actions) */
    int64_t blob_floats;    /* checked against the layout's size */
    const float *lr;        /* [1] the learning rate */
    int32_t *step;          /* [1] optimiser steps taken */
    double *beta_pow;       /* [2] beta1^step, beta2^step (1, 1 before the first step), 8-byte aligned */
    float *params;          /* [G + 1] the weights in gd_policy_grad's flat layout; element G is a zero nobody writes */
    float *exp_avg;         /* [G] Adam's first moment */
    float *exp_avg_sq;      /* [G] Adam's second moment */
    float *blob;            /* gd_policy.blob: every updated weight is stored here too; padding entries are never written */
    const int32_t *blob_of; /* [G] blob_of[e]: the one place of parameter e in blob (the inverse of the layout) */
    float *stats;           /* [7] the last call's policy_loss, value_loss, entropy, old_approx_kl, approx_kl, clipfrac
                             * (gd_ppo_loss) and grad_norm (gd_ppo_adam) */
    float *stats_sum;       /* [7] running sums of stats_scale * stats; the caller zeroes them when it reads them */
    float *scal;            /* [4] scratch of gd_ppo_adam: total, coef, bc1, rbc2 from its first launch to its second */
    /* scratch of gd_ppo_update only: */
    float *newlogprob, *entropy, *newvalue;   /* [M] each: what gd_policy_evaluate returns */
    float *d_logprob, *d_entropy, *d_value;   /* [M] each: the upstream gradients */
    float *grad;                              /* [G] the gradient */
} gd_ppo;
/* The loss: from newlogprob, entropy, newvalue (gd_policy_evaluate's outputs), the stored old_logprob and old_value, the
 * advantages and the returns, all [M] float32, the upstream gradients d_logprob, d_entropy, d_value [M] float32 of
 * mean(pg) - ent_coef mean(entropy) + vf_coef v_loss (every element stored), stats[0..6), and stats_scale * stats added into
 * stats_sum[0..6).  One launch on `stream` (a single workgroup: the sums have one fixed order), no host synchronisation, no
 * allocation, no atomics.  Uses of ppo: the hyper-parameters, num_rows, stats, stats_sum.
 * GD_ERR_INVALID: a null pointer, num_rows outside [1, 2^20], num_rows < 2 with norm_adv, a misaligned pointer. */
int gd_ppo_loss(const gd_ppo *ppo, const float *newlogprob, const float *entropy, const float *newvalue, const float *old_logprob,
                const float *old_value, const float *adv, const float *ret, float *d_logprob, float *d_entropy, float *d_value,
                void *stream);
/* Gradient clipping and one Adam step on grad [G] float32: the norm, the coefficient, the moments and the weights by the rule;
 * each updated weight is stored to params[e] and to blob[blob_of[e]] by the same lane, so the forward's packed weights follow
 * without a re-pack; stats[6] = the norm before clipping (and stats_sum[6]); step and beta_pow advance by one.  Two launches on
 * `stream`: the first (one workgroup) leaves the step's scalars in scal, the second (a lane per parameter) reads them.  No
 * host synchronisation, no allocation, no atomics.
 * GD_ERR_INVALID: a null pointer, ego_width not 6 or 9, n_actions outside [1, 1024], grad_floats or blob_floats not the
 * layout's, betas outside [0, 1), eps or max_grad_norm not positive, a misaligned pointer. */
int gd_ppo_adam(const gd_ppo *ppo, const float *grad, void *stream);
/* One whole minibatch update as one call: gd_policy_evaluate(p, g, obs, actions) into ppo's row scratch, gd_ppo_loss,
 * gd_policy_backward into ppo->grad, gd_ppo_adam -- nine launches on `stream`, no host synchronisation, no allocation, no
 * atomics; the results are bit for bit those of the four calls.  p->blob must be ppo->blob, g->params ppo->params, and the sizes
 * of p, g and ppo must agree.
 * GD_ERR_INVALID: whatever the four calls refuse, or a disagreement between p, g and ppo; before any launch. */
int gd_ppo_update(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, const float *obs, const int64_t *actions,
                  const float *old_logprob, const float *old_value, const float *adv, const float *ret, void *stream);
/* Training-mode dropout of the device policy: the reference trains (and rolls out) with its four nn.Dropout layers live --
 * after the tanh of each of the three embedders and after shared_embed's linear.  torch's random stream cannot be reproduced,
 * so the mask is this project's rule, csrc/dropout_rule.hpp, stated there in full: whether an element is kept is a pure
 * function of (seed, call, row, site, entity, feature) through Philox4x32-10 cut into 16-bit fields; an element is dropped
 * iff its field < threshold; a kept element is x * scale, a dropped one +0.  `call` indexes the masked forward / evaluate
 * calls; it lives on the device (as gd_ppo's step does), so a sequence of calls never depends on a host value that changes:
 * every kernel of a call reads *call, and one lane of the call's last launch stores *call + 1 (the library writes the word;
 * callers only read it, or set it between calls).  gd_policy_evaluate_dropout also stores the index it consumed to *used,
 * which is what gd_policy_backward_dropout reads: the backward recomputes the masks of ITS evaluate call. */
typedef struct gd_dropout {
    uint64_t seed;
    const uint64_t *call;   /* device: the index the next forward / evaluate consumes */
    uint64_t *used;         /* device: evaluate stores the index it consumed; backward reads it */
    uint32_t threshold;     /* T */
    float scale;            /* 1 / (1 - p) */
} gd_dropout;
/* The four calls with the masks applied: the arguments, outputs, launch counts (3 / 3 / 3 / 9) and refusals of
 * gd_policy_forward, gd_policy_evaluate, gd_policy_backward and gd_ppo_update, plus d.  d == NULL is exactly the existing
 * function: the same kernels, the same bits.  Otherwise the forward and evaluate mask the four sites at index *d->call and
 * advance it by one (evaluate stores the consumed index to *d->used; the forward does not touch used); the backward masks at
 * index *d->used and writes neither word; gd_ppo_update_dropout is evaluate, loss, backward, Adam with the backward reading
 * the index its own evaluate stored.  Winners are recorded on the masked outputs.  No host synchronisation, no allocation, no
 * atomics; no workgroup reads a word another workgroup of the same launch writes.
 * GD_ERR_INVALID, before any launch: whatever the existing call refuses; with d != NULL a null or not 8-byte aligned call or
 * used, threshold outside [1, 65535], a scale that is not finite. */
int gd_policy_forward_dropout(const gd_policy *p, const gd_dropout *d, const float *obs, const float *u, int32_t deterministic,
                              int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out, void *stream);
int gd_policy_evaluate_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_dropout *d, const float *obs,
                               const int64_t *actions, float *logprob, float *entropy, float *value, void *stream);
int gd_policy_backward_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_dropout *d, const float *obs,
                               const int64_t *actions, const float *d_logprob, const float *d_entropy, const float *d_value,
                               float *grad, void *stream);
int gd_ppo_update_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, const gd_dropout *d, const float *obs,
                          const int64_t *actions, const float *old_logprob, const float *old_value, const float *adv,
                          const float *ret, void *stream);
/* Device BC policy forward: the reference's imitation-learning model, EarlyFusionAttnBCNet in eval mode
 * (gpudrive/integrations/il/model/model.py, networks.py), on the tensors gd_il_batch writes.  Float32 throughout; the matrix
 * products over token tiles are v_mfma_f32_32x32x2_f32 chains.  network_dim 64, head_dim 64, 4 heads of 16 channels, 4 embedder
 * layers, tanh, no dropout, action_dim 3, time_dim 1, no aux head.
 *   tokens: ego (input: its R six-float blocks in time order), partner e (its R six-float rows), road r (its R thirteen-float
 *           rows), each through 4 x (Linear, LayerNorm, tanh); L = A + 200 tokens, masked entities embedded like any other
 *   layer:  h = LN(x); q, k, v = Linear(h), q / 4; scores of masked keys replaced by -FLT_MAX (an all-masked row attends
 *           uniformly); softmax; o_proj; + x; then + MLP (LN, Linear, erf GELU, Linear)
 *   fusion_layers over all L tokens, mask [0 | partner_mask[:, R-1] | road_mask[:, R-1]]; branch_layers over the first A
 *   tokens and, separately, over the 200 road tokens; two cross-attention layers with the ego token (token 0) as the one
 *   query over the partner tokens and over the road tokens; context = [ego | ego_ro | ego_rg]; the GMM head (192 -> 64 ReLU,
 *   head_layers x (x + ReLU(Linear x)), 64 -> 7 C) and csrc/bc_rule.hpp.
 * blob: the weights packed once in the order the kernels read them; gpudrive_lab_amd/bc_policy.py `pack_index` states it.
 * scratch: chunk_rows * 3 * (A + 200) * 64 floats (token, key and value buffers of one chunk of rows); a larger n runs chunk
 * after chunk on the stream. */
typedef struct gd_bc_policy {
    int32_t max_agents;     /* A: 64 or 128 */
    int32_t num_stack;      /* R: 1 .. 8 */
    int32_t fusion_layers;  /* num_layer[0]: 1 .. 4 */
    int32_t branch_layers;  /* num_layer[1]: 1 .. 4 (ro_attn and rg_attn each) */
    int32_t head_layers;    /* head_num_layers: 0 .. 4 */
    int32_t n_components;   /* C: 1 .. 16 */
    float clip_value;       /* the lower clamp of the raw covariances */
    int32_t chunk_rows;     /* 1 .. 4096: the rows the scratch holds */
    const float *blob;      /* blob_floats floats, 16-byte aligned */
    int64_t blob_floats;    /* checked against the layout's size */
    float *scratch;         /* scratch_floats floats, 256-byte aligned */
    int64_t scratch_floats; /* at least chunk_rows * 3 * (A + 200) * 64 */
} gd_bc_policy;
/* The outputs of one forward (device pointers); NULL: not written.  Every byte of every one given is stored by every call. */
typedef struct gd_bc_outputs {
    float *context;          /* [n][192] ([n][384] at network_dim 128, gd_bc_forward_dim) */
    float *means;            /* [n][C][3] */
    float *log_covariances;  /* [n][C][3] the clamped raw values */
    float *covariances;      /* [n][C][3] their exp */
    float *weights;          /* [n][C] */
    float *actions;          /* [n][3] the deterministic action, or the rule's draw from u and z */
    float *nll;              /* [n] gmm_loss's per-row value for expert_actions (which is then required) */
    float *ego_attn_score;   /* [n][4][A - 1] ego_ro_attn's attention row divided by its sum */
    int32_t *component;      /* [n] the component the action came from */
} gd_bc_outputs;
/* obs [n][R][D] float32 (D = 6 + 6 (A - 1) + 2600), 4-byte aligned; partner_mask [n][R][A - 1] and road_mask [n][R][200], one
 * byte per entry (bool or uint8, non-zero: padding), any alignment; only time index R - 1 is read.  u [n] in [0, 1) and z
 * [n][3] standard normals, required unless deterministic != 0.  expert_actions [n][3], required with out->nll.
 * 2 fusion_layers + 2 branch_layers + 3 launches per chunk on `stream`, no host synchronisation, no allocation, no atomics.
 * GD_ERR_INVALID: a null pointer, a value outside the ranges above, n outside [1, 2^20], blob_floats or scratch_floats not
 * the layout's, a misaligned pointer. */
int gd_bc_forward(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                  int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                  void *stream);
/* One batch of the reference's evaluate() (baselines/il/il.py:99-180) added to acc [11] float32 on the device, one launch, fixed
 * summation order: acc[0] += mean nll; acc[1..3] += mean |actions - expert| per dimension; acc[4..6] += the sums of
 * |actions - expert| over the rows with |expert_0| > 2, |expert_1| > 0.035, |expert_2| > 0.023; acc[7..9] += those rows' counts;
 * acc[10] += 1.  n in [1, 2^20]. */
int gd_bc_eval_accumulate(int32_t n, const float *nll, const float *actions, const float *expert_actions, float *acc, void *stream);
/* Device BC policy backward: the gradient of sum_b grad_nll[b] * nll[b] (nll: gd_bc_forward's out->nll, gmm_loss's per-row
 * value) with respect to every parameter, float32, flat in the state dict's order (gpudrive_lab_amd/bc_policy.py
 * `expected_shapes`) and each tensor's natural row-major layout.  No gradient with respect to obs.  It follows torch's autograd
 * of the reference: a masked score receives no gradient (a row whose keys are all masked passes its uniform share to the
 * values and nothing to queries and keys), the covariance clamp passes the gradient on [clip_value, 3.58352] bounds
 * included and an exact 0 outside (csrc/bc_grad_rule.hpp), the head's ReLU passes nothing at a pre-activation <= 0.
 * Memory does not depend on n: per chunk of p->chunk_rows rows the forward is run again by gd_bc_forward's own kernels (the
 * nll is therefore gd_bc_forward's bit for bit), the inputs of the self-attention layers are kept in `scratch`, and layer by
 * layer, last to first, the layer's keys, values, attention output and softmax row statistics are recomputed and its
 * backward runs: scores are rebuilt per 32 x 32 tile from q, k and the statistics, once with a query tile owning dQ and
 * walking the keys, once with a key tile owning dK and dV and walking the queries.  No tensor with an L x L extent exists.
 * No atomics: weight gradients are summed by num_partials workgroups, workgroup w over the (row, tile) pairs w, w +
 * num_partials, .. of a launch in ascending order into partials[w], across chunks; the last launch adds the partials in
 * index order.  Equal inputs, chunk_rows and num_partials give equal bits.  Every element of scratch that is read, of
 * partials and of grad is stored by every call. */
typedef struct gd_bc_grad {
    float *scratch;         /* scratch_floats floats, 256-byte aligned */
    int64_t scratch_floats; /* at least blob_floats rounded up to 64 + chunk_rows * (A + 200) * (64 * (fusion_layers +
                             * branch_layers + 5) + 16) */
    float *partials;        /* [num_partials][grad_floats], 16-byte aligned */
    int64_t grad_floats;    /* the parameters' count: checked against the layout's */
    int32_t num_partials;   /* 1 .. 4096 */
    int32_t reserved;       /* 0 */
} gd_bc_grad;
/* obs, the masks and expert_actions as gd_bc_forward takes them; grad_nll [n] the upstream gradient; nll [n] or NULL receives
 * the recomputed forward's value; grad [grad_floats], 16-byte aligned.  p->scratch is used as by gd_bc_forward.  No host
 * synchronisation, no allocation.  GD_ERR_INVALID, before any launch: whatever gd_bc_forward refuses, a null or misaligned
 * buffer, scratch_floats or grad_floats not the layout's, num_partials outside [1, 4096]. */
int gd_bc_backward(const gd_bc_policy *p, const gd_bc_grad *g, const float *obs, const uint8_t *partner_mask,
                   const uint8_t *road_mask, int32_t n, const float *expert_actions, const float *grad_nll, float *nll, float *grad,
                   void *stream);
/* Device BC update: the rest of one gradient step of the reference's imitation learning (baselines/il/il.py:267-303) around
 * gd_bc_forward and gd_bc_backward -- the step's statistics and the upstream gradient of loss.mean(), clip_grad_norm_, the
 * reference's get_grad_norm and torch.optim.AdamW (no amsgrad, no maximize).  The rule, with every rounding and the order of
 * every sum, is csrc/bc_opt_rule.hpp.  Every pointer is a device pointer owned by the caller, and every value that changes
 * between calls (the learning rate, the step count, the running products of the betas) lives on the device.  G = grad_floats,
 * T = num_tensors: the flat gradient cut into the state dict's tensors (gpudrive_lab_amd/bc_policy.py `expected_shapes`). */
typedef struct gd_bc_opt {
    float max_grad_norm;    /* > 0 */
    float eps;              /* AdamW's, > 0 */
    float weight_decay;     /* >= 0, finite */
    float stats_scale;      /* every call adds stats_scale * its statistics into stats_sum */
    double beta1, beta2;    /* in [0, 1) */
    int64_t grad_floats;    /* G, checked against the parameter count of the configuration below */
    int64_t blob_floats;    /* checked against the layout's size */
    int32_t num_stack, fusion_layers, branch_layers, head_layers, n_components; /* gd_bc_policy's: they fix G, T and the blob */
    int32_t num_tensors;    /* T, checked against the layout's (at most 288) */
    int32_t max_rows;       /* the rows the row scratch below holds, 1 .. 2^20 */
    int32_t reserved;       /* 0 */
    const int32_t *tensor_end; /* [T] cumulative element counts: tensor t is [tensor_end[t - 1], tensor_end[t]) */
    const float *lr;        /* [1] the learning rate */
    int32_t *step;          /* [1] optimiser steps taken */
    double *beta_pow;       /* [2] beta1^step, beta2^step (1, 1 before the first step), 8-byte aligned */
    float *params;          /* [G + 1] the weights in the flat layout; element G is a zero nobody writes */
    float *exp_avg;         /* [G] AdamW's first moment */
    float *exp_avg_sq;      /* [G] AdamW's second moment */
    float *blob;            /* gd_bc_policy.blob: every updated weight is stored here too; padding entries are never written */
    const int32_t *blob_of; /* [G] blob_of[e]: the one place of parameter e in blob (the inverse of the layout) */
    float *stats;           /* [6] the last call's loss, dx_loss, dy_loss, dyaw_loss (gd_bc_train_rows), grad_norm (before
                             * clipping) and max_grad_norm (the largest tensor norm after clipping) (gd_bc_adamw) */
    float *stats_sum;       /* [6] running sums of stats_scale * stats; the caller zeroes them when it reads them */
    int32_t *max_grad_tensor; /* [1] the first tensor that attains the largest norm */
    float *tensor_norms;    /* [T] every tensor's gradient norm before clipping */
    float *scal;            /* [4 + 2 T] scratch of gd_bc_adamw, 8-byte aligned: total, coef, bc1, rbc2, then the tensors'
                             * sums of squares as float64 */
    /* scratch of gd_bc_update only: */
    float *actions;         /* [max_rows][3] the deterministic actions of the weights before the step */
    float *nll;             /* [max_rows] */
    float *grad_nll;        /* [max_rows] */
    float *grad;            /* [G] the gradient, 16-byte aligned */
} gd_bc_opt;
/* The rows of one step: from nll [n] and actions [n][3] (gd_bc_forward's, deterministic) and expert_actions [n][3], stats[0..4)
 * = the means of nll and of |actions - expert_actions| per dimension, stats_scale * them added into stats_sum[0..4), and
 * grad_nll[b] = 1 / n for every b < n.  One launch on `stream` (a single workgroup of 256 lanes: the sums have one fixed
 * order), no host synchronisation, no allocation, no atomics.  Uses of opt: stats_scale, stats, stats_sum.
 * GD_ERR_INVALID: a null pointer, n outside [1, 2^20], a misaligned pointer. */
int gd_bc_train_rows(const gd_bc_opt *opt, int32_t n, const float *nll, const float *actions, const float *expert_actions,
                     float *grad_nll, void *stream);
/* Gradient clipping and one AdamW step on grad [G] float32: the tensors' norms (tensor_norms, every element stored), the total
 * norm, the coefficient, the moments and the weights by the rule; each updated weight is stored to params[e] and to
 * blob[blob_of[e]] by the same lane, so the forward's packed weights follow without a re-pack; stats[4] = the norm before
 * clipping, stats[5] = the largest tensor norm after it (both also into stats_sum), max_grad_tensor its tensor; step and
 * beta_pow advance by one.  Three launches on `stream`: a workgroup per tensor, one workgroup that leaves the step's scalars in
 * scal, a lane per parameter that reads them.  No host synchronisation, no allocation, no atomics; no workgroup reads a word
 * another workgroup of the same launch writes.
 * GD_ERR_INVALID, before any launch: a null pointer, a configuration outside gd_bc_policy's ranges, grad_floats, blob_floats or
 * num_tensors not the layout's, betas outside [0, 1), eps or max_grad_norm not positive, a negative or non-finite
 * weight_decay, a non-zero reserved, a misaligned pointer. */
int gd_bc_adamw(const gd_bc_opt *opt, const float *grad, void *stream);
/* One whole gradient step as one call: gd_bc_forward(p, deterministic) with actions and nll into opt's row scratch,
 * gd_bc_train_rows, gd_bc_backward(grad_nll of the scratch, nll NULL) into opt->grad, gd_bc_adamw -- on `stream`, no host
 * synchronisation, no allocation, no atomics; the results are bit for bit those of the four calls.  p->blob must be opt->blob,
 * the configurations and sizes of p, g and opt must agree, n is in [1, opt->max_rows] and may differ from call to call.
 * GD_ERR_INVALID: whatever the four calls refuse, or a disagreement between p, g and opt; before any launch. */
int gd_bc_update(const gd_bc_policy *p, const gd_bc_grad *g, const gd_bc_opt *opt, const float *obs, const uint8_t *partner_mask,
                 const uint8_t *road_mask, int32_t n, const float *expert_actions, void *stream);
/* Closed-loop BC driver: one episode with the BC policy in the loop and its metrics, on the device.  The reference's
 * closed-loop script (baselines/il/test/simulation.py run(), lines 22-135): a window of R = num_stack packed observations per
 * controlled agent, an action from the policy for every agent still alive, zeros for everyone else, the step, the off-road /
 * collision / goal flags, the steps at which goal and off-road first happened, the distance to the goal at the start and at
 * the end, the rates.  All pointers are device pointers owned by the caller; N = n_rows, A = max_agents,
 * D = 6 + (A-1)*6 + 200*13, R = the policy's num_stack; the time pitch of the optional records is always 91.  The caller zeroes
 * dead, the accumulators, the distances and any_alive, fills both step indices with -1, zeroes both masks (only time index
 * R - 1 is ever written) and fills the optional records with its defaults.  csrc/bc_rollout_rule.hpp states the per-row
 * arithmetic and the summary's summation order. */
typedef struct gd_bc_rollout_buffers {
    const int32_t *row_slot;     /* [N] world * A + agent of every row (mask.nonzero() order), each in [0, W * A) */
    const int32_t *row_of_slot;  /* [W * A] the inverse: a slot's row, -1 where the slot is no row */
    int32_t n_rows;              /* 1 .. 2^20 */
    int32_t deterministic;       /* != 0: the mean of the first component of maximal weight; 0: the rule's draw from u and z */
    const float *u;              /* [n_steps][N] in [0, 1), required unless deterministic */
    const float *z;              /* [n_steps][N][3] standard normals, required unless deterministic */
    float *window;               /* [N][R][D] the last R packed observations, oldest first; zeros before the first step.
                                  * Need not be initialised. */
    uint8_t *partner_mask;       /* [N][R][A-1] what gd_bc_forward reads: at time index R - 1, 1 where the partner value is 2 */
    uint8_t *road_mask;          /* [N][R][200] at time index R - 1, 1 where the road row is padding (id -1) */
    uint8_t *partner_value;      /* [N][A-1] the recorder's value of the newest frame: 0 acts, 1 Static and non-zero, 2 nobody */
    float *row_actions;          /* [N][3] the policy's action of every row in the current step (dead rows included) */
    /* running state and results */
    uint8_t *dead;               /* [N] */
    float *goal_achieved, *off_road, *veh_collision;  /* [N] sums of info columns 3 / 0 / 1 + 2, clamped to 1 */
    int32_t *goal_step, *off_road_step;               /* [N] the first t whose info row, read before step t, is > 0; else -1 */
    float *init_goal_dist, *goal_dist;                /* [N] sqrtf(x x + y y) of ego columns 3, 4: at t = 0, at the last step */
    int32_t *any_alive;          /* [92] 1 where some row was alive before step t: iteration t of the reference's loop exists
                                  * (its `break`); their sum is the number of iterations it runs */
    float *summary;              /* [8] off_road_rate, veh_coll_rate, goal_rate, collision_rate, goal_progress, goal_count,
                                  * n_rows, iterations */
    /* optional per-step records (NULL: not written); only iterations that exist are written */
    float *actions;              /* [N][91][3] what was written into the simulator for the row: zeros once it is dead */
    uint8_t *dead_mask;          /* [N][91] the row was dead BEFORE step t */
    float *ego_global_pos;       /* [N][91][2] absolute_self_observation columns 0, 1, live rows only */
    float *ego_global_rot;       /* [N][91] absolute_self_observation column 7, live rows only */
} gd_bc_rollout_buffers;
/* For t in [0, n_steps), on the simulator's stream: the row kernel for time index t (window, masks, distances, step indices,
 * records), gd_bc_forward on all N rows into row_actions, the action kernel (action[:, :, :3] of every slot: a live row's
 * action, zeros for every other slot), the step, the bookkeeping of that step (dead |= done, the accumulators, any_alive[t + 1]);
 * then the summary.  Iterations after every row is dead change no output (the simulator still steps, with zero actions).  With
 * n_steps < 91 the result is the prefix of the full episode.  It does not reset: the caller does.  3 launches per step beside the
 * forward's and the step's, no host synchronisation, no allocation, no atomics.
 * GD_ERR_INVALID: a null pointer, n_rows outside [1, 2^20], n_steps outside [1, 91], the State dynamics model, a policy whose
 * max_agents differs from the simulator's, whatever gd_bc_forward refuses.  GD_ERR_UNSUPPORTED while a packed buffer is
 * attached with only != 0 (the raw rows the observation is computed from are stale). */
int gd_bc_rollout(gd_sim *sim, const gd_bc_policy *policy, const gd_bc_rollout_buffers *buffers, int32_t n_steps);
/* Closed-loop PPO evaluator: one episode with the late-fusion policy (gd_policy) in the loop and the per-world metrics, on the
 * device.  The reference's evaluation rollout (examples/experimental/eval_utils.py rollout(), lines 94-227): an action index
 * from the policy for every controlled agent still live, decoded through the action table, index 0 for everyone else, the
 * step, the off-road / collision / goal sums of live rows, live &= !done, the step at which every world finished, and per
 * world the counts and fractions of rows that achieved the goal, collided, went off road, or did none of the three.  All
 * pointers are device pointers owned by the caller; N = n_rows, the simulator's learner rows (gd_set_learner_rows), whose
 * [N][D] buffer (gd_attach_packed_rows, or gd_attach_packed_rows_conditioned for ego_width 9) is the observation the forward
 * reads; W worlds, A = max_agents; the time pitch of the optional records is always 91.  The caller fills live and
 * world_active with 1, zeroes the accumulators, episode_lengths and bad_indices, sets any_active[0] = 1 and zeroes the rest
 * of it, and fills the optional records with its defaults (actions_idx -1, live_mask 0, agent_positions 0).
 * csrc/policy_rollout_rule.hpp states the per-row and per-world arithmetic and the summary's order. */
typedef struct gd_policy_rollout_buffers {
    int32_t n_rows;              /* N, 1 .. 2^20: the number of learner rows */
    int32_t deterministic;       /* != 0: the first index of the largest logit; 0: the action rule's draw from u */
    const float *u;              /* [n_steps][N] in [0, 1), required unless deterministic */
    const float *table;          /* [n_actions][3] the action table: row k is what action index k writes */
    int32_t n_actions;           /* the table's rows; must be the policy's n_actions */
    int32_t reserved;            /* 0 */
    /* what every forward writes (all N rows, dead rows too: there is no compaction) */
    int64_t *actions;            /* [N] */
    float *logprob, *entropy, *value;  /* [N] each */
    /* running state and results, per row */
    uint8_t *live;               /* [N] */
    float *goal_achieved, *collided, *off_road;  /* [N] raw sums of info columns 3 / 1 + 2 / 0 over the steps the row was live */
    /* running state and results, per world */
    uint8_t *world_active;       /* [W] */
    float *episode_lengths;      /* [W] the first t at which every mask slot of the world is done; 0 if that never happened */
    int32_t *bad_indices;        /* [W] live rows whose action index was outside the table (added to gd_stat 45 at the end) */
    int32_t *any_active;         /* [92] 1 where some world was active before step t: iteration t of the reference's loop exists */
    float *goal_achieved_count, *frac_goal_achieved, *collided_count, *frac_collided, *off_road_count, *frac_off_road,
        *other_count, *frac_other, *controlled_per_scene;  /* [W] each; a fraction is NaN for a world without rows */
    float *summary;              /* [8] the totals of the four counts (goal_achieved, collided, off_road, other), n_rows,
                                  * worlds_with_rows, iterations, mean_episode_length */
    /* optional per-step records (NULL: not written); only iterations that exist are written */
    int64_t *actions_idx;        /* [N][91] what the policy chose for the row, -1 once the row is dead */
    uint8_t *live_mask;          /* [N][91] the row was live BEFORE step t */
    float *agent_positions;      /* [W][A][91][2] absolute_self_observation columns 0, 1 of every slot AFTER step t */
} gd_policy_rollout_buffers;
/* For t in [0, n_steps), on the simulator's stream: gd_policy_forward on all N rows of the attached buffer with u + t * N (or
 * the deterministic argmax; always the unmasked forward, a dropout rule is neither consulted nor advanced), the action kernel
 * (action[:, :, :3] of every slot: table[index] for a live row, table[0] for every other slot; a live row's index outside
 * the table leaves its action as it was and is counted), the step, the bookkeeping kernel (one workgroup per world: the
 * sums, live &= !done, the world test, episode_lengths, any_active[t + 1], the records); then a per-world kernel (counts and
 * fractions) and a one-workgroup summary.  Iterations after every world is inactive change no output (the simulator still
 * steps).  With n_steps < 91 the result is the prefix of the full episode.  It does not reset and does not advance the log
 * playback: the caller does.  2 launches per step beside the forward's three and the step's, no host synchronisation, no
 * allocation, no atomics.
 * GD_ERR_INVALID: a null pointer, n_rows outside [1, 2^20] or not the number of learner rows, n_steps outside [1, 91], no
 * learner rows or no row buffer attached, a policy whose max_agents, ego_width or num_rows differs from the simulator's and
 * its buffer's, n_actions different from the policy's, reserved != 0, a misaligned pointer, whatever gd_policy_forward
 * refuses.  GD_ERR_UNSUPPORTED for the State dynamics model (no discrete action space). */
int gd_policy_rollout(gd_sim *sim, const gd_policy *policy, const gd_policy_rollout_buffers *buffers, int32_t n_steps);
/* Live rows: the forward on a device-resident list of rows whose length only the device knows, so that a rollout stops paying
 * for rows that are done.  Nothing here synchronises with the host, allocates, or uses an atomic.
 *
 * gd_live_rows: mask [n] bytes -> rows[0 .. *count) = the indices i with mask[i] != 0, ascending; rows[*count .. n) is not
 * written; count is ONE int32 on the device.  scratch: one int32 per block of GD_LIVE_ROWS_BLOCK rows, that is
 * (n + GD_LIVE_ROWS_BLOCK - 1) / GD_LIVE_ROWS_BLOCK of them (1024 cover every n).  Two launches on `stream`; equal input gives
 * equal bytes.  GD_ERR_INVALID, before any launch: a null pointer, rows, count or scratch not 4-byte aligned, n outside
 * [1, 2^20]. */
#define GD_LIVE_ROWS_BLOCK 1024
int gd_live_rows(const uint8_t *mask, int32_t n, int32_t *rows, int32_t *count, int32_t *scratch, void *stream);
/* gd_policy_forward (d == NULL) or gd_policy_forward_dropout on the rows of a list: rows [N] int32 of which the first *count
 * are read, count one int32 on the device (gd_live_rows writes both).  For a listed row r the call reads obs[r] and u[r] and
 * writes actions[r], logprob[r], entropy[r], value[r] and logits_out[r], every bit what the full forward (the masked one at the
 * same call index) writes for that row: no result of a row depends on which rows share its wave, and the dropout rule is keyed
 * on r, not on the position in the list.  Rows that are not listed are NOT written, in any output.  The grids are sized for
 * p->num_rows and every wave whose positions are past *count returns at once; p->features and p->logits are indexed by position
 * and hold nothing specified afterwards.  With d the call index advances by exactly one per call, also when *count == 0.  An
 * entry outside [0, N) is skipped and a count above N is read as N, for memory safety only; entries must be distinct (a row
 * listed twice is written by two waves).  Three launches, no LDS.
 * GD_ERR_INVALID, before any launch: whatever gd_policy_forward / gd_policy_forward_dropout refuse, a null or not 4-byte aligned
 * rows or count. */
int gd_policy_forward_rows(const gd_policy *p, const gd_dropout *d, const float *obs, const float *u, int32_t deterministic,
                           int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out, const int32_t *rows,
                           const int32_t *count, void *stream);
/* gd_policy_rollout with the list in the loop.  Device pointers owned by the caller; N = buffers->n_rows. */
typedef struct gd_policy_rollout_rows {
    int32_t *rows;               /* [N] the list of the current step */
    int32_t *count;              /* [1] its length */
    int32_t *scratch;            /* gd_live_rows' scratch for n = N */
    int32_t *live_count;         /* [91] the length of step t's list (the rows live before step t), or NULL; entries
                                  * t >= n_steps are not written */
    int32_t reserved;            /* 0 */
} gd_policy_rollout_rows;
/* For t in [0, n_steps): gd_live_rows on buffers->live (its second launch also stores live_count[t]), gd_policy_forward_rows
 * on that list with u + t * N, then the action kernel, the step and the bookkeeping kernel of gd_policy_rollout, and its two
 * kernels at the end: 2 launches per step more than gd_policy_rollout.  Every result gd_policy_rollout defines is the same,
 * bit for bit; actions, logprob, entropy and value of a row hold the forward of the last step the row was live at (the action
 * kernel reads the index of live rows only).  GD_ERR_INVALID / GD_ERR_UNSUPPORTED: whatever gd_policy_rollout refuses; a null
 * rows argument, a null or not 4-byte aligned rows, count or scratch, a live_count that is not 4-byte aligned,
 * reserved != 0. */
int gd_policy_rollout_compact(gd_sim *sim, const gd_policy *policy, const gd_policy_rollout_buffers *buffers,
                              const gd_policy_rollout_rows *rows, int32_t n_steps);
/* Several policies in the same worlds (the reference's gpudrive/utils/multi_policy_rollout.py): every row has an owner, one of
 * P <= GD_POLICY_SET_MAX policies, and ONE forward of three launches serves them all.  Nothing here synchronises with the
 * host, allocates, or uses an atomic.  csrc/multi_policy_rule.hpp states the segment arithmetic, the per-policy counts and the
 * summary's order.
 *
 * gd_owned_rows: mask [n] bytes and owner [n] bytes -> one list with a segment per policy.  count[p] = the rows i with
 * mask[i] != 0 && owner[i] == p; start[0] = 0, start[p + 1] = start[p] + count[p] rounded up to a multiple of 32;
 * rows[start[p] .. start[p] + count[p]) = those rows, ascending; every position from there up to start[p + 1] holds -1.  rows has
 * n + 32 P entries, of which those at or past start[P] are not written; start has P + 1 entries, count P.  A row whose owner is
 * >= P is listed nowhere.  scratch: one int32 per owner and per block of GD_LIVE_ROWS_BLOCK rows, P * ((n + GD_LIVE_ROWS_BLOCK -
 * 1) / GD_LIVE_ROWS_BLOCK) of them.  count_copy [P], or NULL: a second place for the counts.  Two launches on `stream`; equal
 * input gives equal bytes.  GD_ERR_INVALID, before any launch: a null pointer (but count_copy), rows, start, count, scratch or
 * count_copy not 4-byte aligned, n outside [1, 2^20], n_policies outside [1, GD_POLICY_SET_MAX]. */
#define GD_POLICY_SET_MAX 8
int gd_owned_rows(const uint8_t *mask, const uint8_t *owner, int32_t n, int32_t n_policies, int32_t *rows, int32_t *start,
                  int32_t *count, int32_t *scratch, int32_t *count_copy, void *stream);
/* The policies of one forward on an owned list.  They share num_rows = N, max_agents, ego_width and n_actions (so the layout of
 * their blobs); of each gd_policy the sizes, blob and blob_floats are read, its own features and logits are not used. */
typedef struct gd_policy_set {
    int32_t n_policies;          /* P, 1 .. GD_POLICY_SET_MAX */
    int32_t reserved;            /* 0 */
    gd_policy policy[GD_POLICY_SET_MAX];  /* the first P are read */
    float *features;             /* [N + 32 P][192] scratch indexed by list position, 16-byte aligned */
    float *logits;               /* [N + 32 P][NA] scratch indexed by list position */
} gd_policy_set;
/* gd_policy_forward (always the unmasked forward) on an owned list, every row with the weights of its owner: rows, start and
 * count as gd_owned_rows writes them.  For a row r listed under p the call reads obs[r] and u[r] and writes actions[r],
 * logprob[r], entropy[r], value[r] and logits_out[r], every bit what gd_policy_forward of policy p writes for that row.  Rows
 * that are not listed are NOT written, in any output.  Three launches whatever P is, with grids sized for the N + 32 P
 * positions; a wave in the padding or past the last segment returns at once; set->features and set->logits hold nothing
 * specified afterwards.  A position belongs to segment p when start[p] <= q < start[p] + count[p] and q < N + 32 P; an entry
 * outside [0, N) is skipped: for memory safety only (starts that are no multiples of 32 give a row another policy's weights;
 * entries must be distinct).  No LDS.
 * GD_ERR_INVALID, before any launch: whatever gd_policy_forward refuses of any of the P policies (but its features and logits),
 * n_policies outside [1, GD_POLICY_SET_MAX], reserved != 0, policies that differ in num_rows, max_agents, ego_width or
 * n_actions, null or misaligned set->features / set->logits, a null or not 4-byte aligned rows, start or count. */
int gd_policy_forward_owned(const gd_policy_set *set, const float *obs, const float *u, int32_t deterministic, int64_t *actions,
                            float *logprob, float *entropy, float *value, float *logits_out, const int32_t *rows,
                            const int32_t *start, const int32_t *count, void *stream);
/* The episode with P policies in the loop.  Device pointers owned by the caller; N = buffers->n_rows, P = set->n_policies. */
typedef struct gd_multi_policy_buffers {
    const uint8_t *owner;        /* [N] the policy index of every row; a row whose owner is >= P is never listed */
    int32_t *rows;               /* [N + 32 P] the owned list of the current step */
    int32_t *start;              /* [P + 1] */
    int32_t *count;              /* [P] */
    int32_t *scratch;            /* gd_owned_rows' scratch for n = N and P policies */
    const float *denominator;    /* [W] the reference's controlled_per_scene: what every policy's fractions are divided by */
    /* per policy and world, [P][W] each: the rows of policy p in world w whose sum is > 0, and count / denominator[w] (NaN for
     * 0 / 0: kept); n_rows: the rows of policy p in world w */
    float *goal_achieved_count, *frac_goal_achieved, *collided_count, *frac_collided, *off_road_count, *frac_off_road, *n_rows;
    float *summary;              /* [P][4] per policy the totals of the three counts (goal_achieved, collided, off_road), n_rows */
    int32_t *list_count;         /* [91][P] the lengths of step t's segments, or NULL; entries t >= n_steps are not written */
    int32_t reserved;            /* 0 */
} gd_multi_policy_buffers;
/* For t in [0, n_steps), on the simulator's stream: gd_owned_rows on buffers->live and owner (its second launch also stores
 * list_count[t]), gd_policy_forward_owned on that list with u + t * N, then the action kernel, the step and the bookkeeping
 * kernel of gd_policy_rollout: 7 launches per step beside the step's own, whatever P is.  Policies own disjoint rows, so the
 * reference's per-policy accumulators are `buffers`' per-row ones read through owner.  At the end gd_policy_rollout's two
 * kernels, so that every output gd_policy_rollout defines is produced over all rows (as in gd_policy_rollout_compact: actions,
 * logprob, entropy and value of a row hold the forward of the last step the row was live at), then a per-world kernel for the
 * per-policy counts and fractions and a one-workgroup summary.  Iterations after every world is inactive change no output.  With
 * n_steps < 91 the result is the prefix of the full episode.  It does not reset and does not advance the log playback.
 * GD_ERR_INVALID / GD_ERR_UNSUPPORTED: whatever gd_policy_rollout refuses (of the set's first policy, whose num_rows must be
 * n_rows), whatever gd_owned_rows and gd_policy_forward_owned refuse, a null or misaligned buffer of gd_multi_policy_buffers
 * (but list_count, which may be null), reserved != 0. */
int gd_multi_policy_rollout(gd_sim *sim, const gd_policy_set *set, const gd_policy_rollout_buffers *buffers,
                            const gd_multi_policy_buffers *multi, int32_t n_steps);
/* gd_bc_forward on the rows of a list: rows [n] int32 of which the first *count are read, count one int32 on the device
 * (gd_live_rows writes both).  For a listed row r the call reads obs[r], both masks' row r, u[r], z[r] and expert_actions[r] and
 * writes index r of every output given (context, means, log_covariances, covariances, weights, actions, nll, ego_attn_score,
 * component), every bit what gd_bc_forward writes for that row: no result of a sample depends on the samples beside it, and the
 * draw is keyed on r, not on the position in the list.  Rows that are not listed are NOT written, in any output.  A list
 * position q belongs to chunk q / chunk_rows and to slot q % chunk_rows of p->scratch, which holds nothing specified afterwards.
 * The host does not know the length: all ceil(n / chunk_rows) chunks are launched with gd_bc_forward's grids, 2 fusion_layers
 * + 2 branch_layers + 3 launches each, and every workgroup whose position is past *count returns at its first load.  An entry
 * outside [0, n) is skipped and a count above n is read as n, for memory safety only; entries must be distinct (a row listed
 * twice is written by two workgroups).  No host synchronisation, no allocation, no atomics.
 * GD_ERR_INVALID, before any launch: whatever gd_bc_forward refuses, a null or not 4-byte aligned rows or count. */
int gd_bc_forward_rows(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                       int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                       const int32_t *rows, const int32_t *count, void *stream);
/* gd_bc_rollout with the list in the loop.  Device pointers owned by the caller; N = buffers->n_rows. */
typedef struct gd_bc_rollout_rows {
    int32_t *rows;               /* [N] the list of the current step */
    int32_t *count;              /* [1] its length */
    int32_t *scratch;            /* gd_live_rows' scratch for n = N */
    int32_t *live_count;         /* [91] the length of step t's list (the rows not dead before step t), or NULL; entries
                                  * t >= n_steps are not written */
    int32_t reserved;            /* 0 */
} gd_bc_rollout_rows;
/* For t in [0, n_steps): the row kernel of gd_bc_rollout on every row (a dead row's window, masks and goal distance keep
 * moving), the list of the rows with dead[n] == 0 (gd_live_rows' two launches on the complement of the byte; the second also
 * stores live_count[t]), gd_bc_forward_rows on that list with u + t * N and z + t * N * 3, then the action kernel, the step and
 * the bookkeeping kernel of gd_bc_rollout, and its summary at the end: 2 launches per step more than gd_bc_rollout.  When
 * iteration t does not exist every row is dead, the list is empty and the forward returns at once.  Every output
 * gd_bc_rollout defines is the same, bit for bit, but row_actions: a dead row's holds the action of the last step the row was
 * live at, not the last step's (the action kernel reads live rows only; `actions` records zeros for dead rows either way).
 * GD_ERR_INVALID / GD_ERR_UNSUPPORTED: whatever gd_bc_rollout refuses; a null rows argument, a null or not 4-byte aligned rows,
 * count or scratch, a live_count that is not 4-byte aligned, reserved != 0. */
int gd_bc_rollout_compact(gd_sim *sim, const gd_bc_policy *policy, const gd_bc_rollout_buffers *buffers,
                          const gd_bc_rollout_rows *rows, int32_t n_steps);
/* The hidden states a linear probe reads (the reference's forward hooks, baselines/il/linear_probing.py:68-95): out [n][A][64]
 * float32, 16-byte aligned, receives tokens 0 .. A - 1 (the ego, then the partners) of the last_hidden_state of the tapped
 * block -- fusion_attn after its fusion_layers self layers, or ro_attn after its branch_layers more.  Per chunk gd_bc_forward's
 * own kernels run and stop at the tap (for GD_LP_TAP_FUSION no branch layer, no cross attention and no head is launched), then
 * one copy launch.  Every byte of out is stored by every call.  No host synchronisation, no allocation.  GD_ERR_INVALID: an
 * unknown tap, a null or misaligned out, whatever gd_bc_forward refuses. */
enum { GD_LP_TAP_FUSION = 0, GD_LP_TAP_RO = 1 };
int gd_bc_hidden(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n, int32_t tap,
                 float *out, void *stream);
/* Device linear probe: the reference's LinearProbPosition (an nn.Linear(K, 64) over 8 x 8 position classes) trained and scored
 * on the labels gd_il_future_batch writes (baselines/il/linear_probing.py:169-342).  csrc/lp_rule.hpp states the rule.
 * model: GD_LP_EARLY reads the fusion_attn tap, GD_LP_LATE the ro_attn tap (K = 64 both), GD_LP_BASELINE reads obs itself (no
 * policy: p is NULL): for 'ego' the row is obs[b][:][0..6) flattened (K = 6 R), for 'other' [ego 6 | partner j's 6] per time
 * index (K = 12 R <= 64).  exp: GD_IL_FUTURE_OTHER (the rows of sample b are its A - 1 partner tokens 1 .. A - 1; selected where
 * the mask byte is 0) or GD_IL_FUTURE_EGO (token 0; selected where the mask byte is not 0).  With a policy max_agents and
 * num_stack must be the policy's.  Every pointer is a device pointer owned by the caller. */
enum { GD_LP_EARLY = 0, GD_LP_LATE = 1, GD_LP_BASELINE = 2 };
enum { GD_LP_EVAL_WORDS = 208 };  /* gd_lp_eval_accumulate's acc, int32 words */
typedef struct gd_lp_probe {
    int32_t model, exp;
    int32_t in_features;   /* K */
    int32_t num_partials;  /* 1 .. 4096 */
    int32_t max_agents, num_stack;
    int32_t reserved[2];   /* 0 */
    float eps, weight_decay;
    double beta1, beta2;
    float *weight;       /* [64 K + 64] head.weight [64][K], then head.bias: the flat layout */
    float *packed;       /* [4160] the weight in bc_policy.py's `mfma` form, columns K .. 63 zero, then the bias; 16-byte aligned */
    float *exp_avg;      /* [64 K + 64] */
    float *exp_avg_sq;   /* [64 K + 64] */
    const float *lr;     /* [1] */
    int32_t *step;       /* [1] */
    double *beta_pow;    /* [2] beta1^step, beta2^step */
    float *grad;         /* [64 K + 64] the last update's gradient of the mean loss (not written when no row was selected) */
    float *part_f;       /* [num_partials][64 K + 64] */
    double *part_d;      /* [num_partials][2] */
    int32_t *part_i;     /* [num_partials][392] */
    float *stats;        /* [8] the last non-empty batch: loss, accuracy, macro F1, the OOD rows' loss sum, correct count and count,
                          * M, bad labels */
    double *sums;        /* [3] the sums of loss, accuracy and macro F1 over the updates that were not skipped */
    int32_t *counts;     /* [3] updates made, updates skipped (M == 0), selected rows dropped for a label outside [0, 63] */
    float *scal;         /* [4] what the reduce launch leaves for the AdamW launch */
} gd_lp_probe;
/* Per-row outputs, [n][A - 1] for 'other' and [n] for 'ego'; each may be NULL.  logits [..][64] (16-byte aligned); loss_row:
 * logsumexp - logit[label] for every row whose label is in [0, 63], selected or not, 0 otherwise; pred: the first index of
 * the maximum. */
typedef struct gd_lp_rows {
    float *logits;
    float *loss_row;
    int64_t *pred;
} gd_lp_rows;
/* LinearProbPosition.forward / .predict: rows->logits and / or rows->pred (loss_row must be NULL: there are no labels).  The tap's
 * launches and one row launch per chunk. */
int gd_lp_forward(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                  int32_t n, const gd_lp_rows *rows, void *stream);
/* One gradient step as one call: per chunk the tap's launches and the row launch (logits, the row rule, the partial sums of
 * the gradient and the counters), then the reduce launch (M, grad, stats, the step's scalars) and the AdamW launch, which stores
 * each weight to `weight` and to its place in `packed`.  mask and labels: aux_mask / other_pos [n][A - 1] or future_valid_mask /
 * ego_pos [n] as gd_il_future_batch writes them (one byte per mask entry, int64 labels, 8-byte aligned).  M == 0 leaves the
 * weights, the moments, step and beta_pow untouched and advances counts[1]; the device decides it.  rows: NULL or per-row outputs.
 * No host synchronisation, no allocation, no atomics. */
int gd_lp_update(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                 int32_t n, const uint8_t *mask, const int64_t *labels, const gd_lp_rows *rows, void *stream);
/* One batch of the reference's evaluation added to acc (GD_LP_EVAL_WORDS int32 words, 8-byte aligned, zeroed by the caller before
 * the first batch): words 0 .. 7 are four float64 -- the sums of the batches' loss, accuracy and macro F1 and the sum of loss_row
 * over the OOD rows; then int32: non-empty batches, empty batches, OOD correct, OOD rows, bad labels, three unused; then the OOD
 * rows' per-class true positives [64], predicted counts [64] and label counts [64].  Nothing of the optimiser is touched. */
int gd_lp_eval_accumulate(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask,
                          const uint8_t *road_mask, int32_t n, const uint8_t *mask, const int64_t *labels, const gd_lp_rows *rows,
                          int32_t *acc, void *stream);
/* gd_bc_hidden at any self-attention layer of the tapped block: layer in [0, fusion_layers) for GD_LP_TAP_FUSION, in
 * [0, branch_layers) for GD_LP_TAP_RO; the forward's kernels stop after that layer of the block.  The block's last layer gives
 * gd_bc_hidden's bits.  (GD_LP_TAP_RO, 0) is the layer the reference's baselines/il/test/intervention.py hooks (ro_attn's child
 * '0').  GD_ERR_INVALID: a layer outside the block, whatever gd_bc_hidden refuses. */
int gd_bc_hidden_layer(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                       int32_t tap, int32_t layer, float *out, void *stream);
/* Probe read-outs inside the BC forward (csrc/bc_readout.hip, csrc/bc_readout_rule.hpp): what the reference's
 * baselines/il/test/intervention.py reads per step from pairs of trained LinearProbPosition heads, taken from the chunk's
 * scratch right after self layer (tap, layer) while it still holds that layer's output.  A probe is its two device buffers,
 * read at call time (gd_lp_probe's `packed` and `weight`; K = 64): a probe that trains between two calls is followed in place. */
enum { GD_BC_READOUT_MAX = 8 };
typedef struct gd_bc_readout_probe {
    const float *packed;         /* [4160] gd_lp_probe.packed; 16-byte aligned */
    const float *weight;         /* [64 * 64 + 64] gd_lp_probe.weight; read for the 'other' probes of an intervention only */
} gd_bc_readout_probe;
typedef struct gd_bc_readout {
    int32_t tap, layer;          /* as gd_bc_hidden_layer's */
    int32_t n_other, n_ego;      /* 0 .. GD_BC_READOUT_MAX each, at least one in total */
    int32_t intervene;           /* 0, or 1: ego_pred_prime is written; needs n_other == n_ego, pair p is (ego[p], other[p]) */
    int32_t reserved;            /* 0 */
    gd_bc_readout_probe other[GD_BC_READOUT_MAX], ego[GD_BC_READOUT_MAX];
    const int64_t *labels;       /* [n] the label of every row (8-byte aligned), or NULL: `label` for every row */
    int64_t label;
    /* the outputs, one byte per class (0 .. 63); row r of each starts at r * its stride (bytes) */
    uint8_t *other_pred;         /* row: [n_other][A - 1], the class of partner token 1 + j under other[q] (padded columns too) */
    uint8_t *ego_pred;           /* row: [n_ego], the class of token 0 under ego[q] */
    uint8_t *ego_pred_prime;     /* row: [n_ego], the class of fl32(token 0 + other[p].weight row label) under ego[p]; a label
                                  * outside [0, 63] is no intervention (ego_pred's value) and the row counts in bad_labels */
    int64_t other_stride, ego_stride, prime_stride;  /* >= n_other * (A - 1), n_ego, n_ego */
    int32_t *bad_labels;         /* [1] += the rows read whose label is outside [0, 63] (once per row); required with intervene */
} gd_bc_readout;
/* gd_bc_forward / gd_bc_forward_rows plus ONE launch per chunk, whatever the number of probes, right after the tapped layer:
 * every output of `out` given is gd_bc_forward's, bit for bit.  With the list only listed rows are read and written, keyed on
 * the row.  Where the tap is a probe's own, other_pred / ego_pred are gd_lp_forward's pred of that probe.  No atomics, no host
 * synchronisation, no allocation.  GD_ERR_INVALID, before any launch: whatever the forward refuses; a null readout, an unknown
 * tap, a layer outside the block, counts outside their range or both 0, reserved != 0, intervene with unequal counts, a null or
 * misaligned buffer of a probe that is read, a null output for a non-zero count, a stride below the row, labels that are not
 * 8-byte aligned, a null or misaligned bad_labels with intervene. */
int gd_bc_forward_readout(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                          int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                          const gd_bc_readout *readout, void *stream);
int gd_bc_forward_rows_readout(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                               int32_t n, int32_t deterministic, const float *u, const float *z, const float *expert_actions,
                               const gd_bc_outputs *out, const gd_bc_readout *readout, const int32_t *rows, const int32_t *count,
                               void *stream);
/* The per-step read-outs of a closed-loop episode, step-major: the slice of step t is contiguous.  Device pointers owned by the
 * caller, who fills them before the call: 0.0 in ego_attn_score, 255 in the classes. */
typedef struct gd_bc_rollout_reads {
    float *ego_attn_score;        /* [91][N][4][A - 1] gd_bc_outputs.ego_attn_score of every step, or NULL */
    const gd_bc_readout *readout; /* or NULL.  Its outputs are [91][N] rows each: step t's rows start at t * N * stride; labels
                                   * is [N], by row */
} gd_bc_rollout_reads;
/* gd_bc_rollout (rows == NULL) or gd_bc_rollout_compact with the read-outs in the loop: step t's forward is
 * gd_bc_forward(_rows)_readout with the outputs' slices of step t.  A row that is live before step t gets that call's bits; a
 * row that is dead before step t, and every row of a step whose iteration does not exist or is >= n_steps, keeps the caller's
 * fill.  With the list only live rows are computed.  Without it the forward runs on dead rows too: k_bc_readout drops a row
 * whose `dead` byte is set (it is neither stored nor counted in bad_labels), and one more launch per step stores 0.0 over the
 * scores of dead rows.  Every other output is gd_bc_rollout's (gd_bc_rollout_compact's), bit for bit.
 * GD_ERR_INVALID / GD_ERR_UNSUPPORTED: whatever gd_bc_rollout (gd_bc_rollout_compact) and gd_bc_forward_readout refuse; a null
 * reads, a reads with neither member, an ego_attn_score that is not 4-byte aligned. */
int gd_bc_rollout_readout(gd_sim *sim, const gd_bc_policy *policy, const gd_bc_rollout_buffers *buffers,
                          const gd_bc_rollout_rows *rows, const gd_bc_rollout_reads *reads, int32_t n_steps);
/* The BC policy at another network_dim: gd_bc_policy, whose size is fixed, with the encoder's width beside it.  128 is the model
 * of the reference's sweep (baselines/il/sweep.yaml: network_dim 128, head_dim 64, num_layer [4, 3]): every embedder Linear,
 * LayerNorm, q / k / v / o projection and MLP Linear is 128 wide, the 4 heads have 32 channels (q is multiplied once, after the
 * bias, by the float32 nearest to 32^-1/2), the context is [n][384], head.input_layer is 384 -> 64 and the GMM head behind it
 * stays 64 wide.  At 128: base.blob_floats is the layout's at that width (`pack_index(..., network_dim=128)`) and
 * base.scratch_floats >= chunk_rows * 3 * (A + 200) * 128.  The forward, the closed loop, the backward (gd_bc_backward_dim)
 * and the update (gd_bc_update_dim) take it; gd_bc_hidden, the linear probes and the read-outs take a gd_bc_policy and stay 64
 * wide. */
typedef struct gd_bc_policy_dim {
    gd_bc_policy base;
    int32_t network_dim;  /* 64 or 128 */
    int32_t reserved;     /* 0 */
} gd_bc_policy_dim;
/* gd_bc_forward and gd_bc_forward_rows at p->network_dim: the same arguments, checks and guarantees; out->context is
 * [n][3 * network_dim].  At 64 they run gd_bc_forward's (gd_bc_forward_rows') own kernels and give its bits.  At 128: the same
 * kernels at T = 4 (csrc/bc_policy.hip), 2 fusion_layers + 2 branch_layers + 3 launches per chunk as at 64, no host synchronisation, no
 * allocation, no atomics.  GD_ERR_INVALID, before any launch: whatever those refuse, a network_dim other than 64 or 128,
 * reserved != 0, blob_floats or scratch_floats not that width's. */
int gd_bc_forward_dim(const gd_bc_policy_dim *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                      int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                      void *stream);
int gd_bc_forward_rows_dim(const gd_bc_policy_dim *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                           int32_t n, int32_t deterministic, const float *u, const float *z, const float *expert_actions,
                           const gd_bc_outputs *out, const int32_t *rows, const int32_t *count, void *stream);
/* gd_bc_backward at p->network_dim: the same arguments, checks, guarantees and stages.  At 64 it runs gd_bc_backward's own
 * launches and gives its bits.  At 128 (csrc/bc_grad.hip at T = 4): g->grad_floats is the parameters' count at that width,
 * g->scratch_floats >= blob_floats rounded up to 64 + chunk_rows * (A + 200) * (128 * (fusion_layers + branch_layers + 5) + 16);
 * nll is gd_bc_forward_dim's bit for bit; the head's stage is a workgroup of 128 threads per row whose sums across its two
 * waves go through LDS in ascending order.  No atomics; equal inputs, chunk_rows and num_partials give equal bits.
 * GD_ERR_INVALID, before any launch: whatever gd_bc_backward refuses, a network_dim other than 64 or 128, reserved != 0, a
 * blob, scratch, grad_floats or grad scratch_floats not that width's. */
int gd_bc_backward_dim(const gd_bc_policy_dim *p, const gd_bc_grad *g, const float *obs, const uint8_t *partner_mask,
                       const uint8_t *road_mask, int32_t n, const float *expert_actions, const float *grad_nll, float *nll,
                       float *grad, void *stream);
/* gd_bc_adamw on the parameters of the policy at network_dim: the same arguments, checks, guarantees and three launches (the
 * kernels have no width in them).  opt->grad_floats and opt->blob_floats are checked against the parameters' count and the
 * layout's size at that width, opt->blob_of is the inverse of that width's layout; opt->reserved stays 0.  At 64 it is
 * gd_bc_adamw.  At 128 with the sweep's layer counts G = 1,399,274 and T = 252.
 * GD_ERR_INVALID, before any launch: a network_dim other than 64 or 128, then whatever gd_bc_adamw refuses at that width. */
int gd_bc_adamw_dim(const gd_bc_opt *opt, int32_t network_dim, const float *grad, void *stream);
/* gd_bc_update at p->network_dim: gd_bc_forward_dim(p, deterministic), gd_bc_train_rows, gd_bc_backward_dim,
 * gd_bc_adamw_dim(opt, p->network_dim) as one call on `stream`, with gd_bc_update's arguments and guarantees; the results are
 * bit for bit those of the four calls.  At 64 it runs gd_bc_update's own launches and gives its bits.  p->base.blob must be
 * opt->blob, and g and opt carry the sizes of that width.
 * GD_ERR_INVALID, before any launch: a null p, a network_dim other than 64 or 128, reserved != 0, then whatever gd_bc_update
 * refuses, in its order, each size checked at that width. */
int gd_bc_update_dim(const gd_bc_policy_dim *p, const gd_bc_grad *g, const gd_bc_opt *opt, const float *obs,
                     const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n, const float *expert_actions, void *stream);
/* The closed-loop episode at p->network_dim: gd_bc_rollout (rows == NULL, reads == NULL), gd_bc_rollout_compact (rows) or
 * gd_bc_rollout_readout (reads) with that forward in the loop, every output as those define it.  reads->ego_attn_score is
 * allowed at either width; reads->readout must be NULL unless network_dim is 64 (GD_ERR_INVALID: the probes read 64-wide
 * tokens).  Otherwise GD_ERR_INVALID / GD_ERR_UNSUPPORTED: whatever those three and gd_bc_forward_dim refuse. */
int gd_bc_rollout_dim(gd_sim *sim, const gd_bc_policy_dim *policy, const gd_bc_rollout_buffers *buffers,
                      const gd_bc_rollout_rows *rows, const gd_bc_rollout_reads *reads, int32_t n_steps);
/* Episode bookkeeping on the device: PufferGPUDrive.step()'s tracking of live agents,
 * episode returns / lengths / collision and off-road counts, finished worlds and their asynchronous reset
 * (gpudrive/env/env_puffer.py:250-403; rewards gpudrive/env/env_torch.py:469-505) without a host round trip.
 * Call after gd_step.  All pointers are device pointers owned by the caller, [W][A] unless noted. */
enum { GD_EPISODE_REWARD_WEIGHTED = 0,  /* "weighted_combination": cw*collided + gw*goal_achieved + ow*off_road */
       GD_EPISODE_REWARD_SPARSE = 1,    /* "sparse_on_goal_achieved": the simulator's reward tensor */
       GD_EPISODE_REWARD_CONDITIONED = 2,  /* "reward_conditioned" (env_torch.py:507-522): (w0*collided + w1*goal_achieved)
                                            * + w2*off_road with w = reward_weights[w][a][0..3) */
       GD_EPISODE_REWARD_LOG_DISTANCE = 3 };  /* "distance_to_logs" (env_torch.py:566-603): the weighted combination
                                               * + log_distance_weight * exp(-|log_pos[w][a][t] - pos[w][a]|), pos = columns 0, 1
                                               * of absolute_self_observation, log_pos = expert_trajectory[w][a][2t .. 2t+2),
                                               * t = (int)episode_lengths[w][0] BEFORE this step's increment (env_puffer.py:251-256),
                                               * clamped to [0, 90] (a guard: the reference would index out of range).  t counts
                                               * from the episode's start, not from the simulator's step: after
                                               * gd_advance_log_playback it lags the simulator, as it does in the reference loop. */
/* How the reward weights of the conditioned reward are drawn (env_torch.py:247-401) */
enum { GD_CONDITION_RANDOM = 0,  /* lb + u * f32(ub - lb) per component, u in [0, 1) from a counter-based generator:
                                  * key (seed, world, weight_draws[world]), counter (slot, component); see episode.hip */
       GD_CONDITION_PRESET = 1,  /* the three weights of gd_episode_config, resolved by the caller from a named preset */
       GD_CONDITION_FIXED = 2 }; /* the three weights of gd_episode_config, given by the caller */
enum { GD_EPISODE_STAT_EPISODES = 0,    /* finished worlds */
       GD_EPISODE_STAT_FINISHED_AGENTS, /* controlled agents in them */
       GD_EPISODE_STAT_RETURN_SUM,      /* sum of agent_episode_returns over those agents */
       GD_EPISODE_STAT_OFF_ROAD_AGENTS, /* agents with offroad_in_episode > 0 */
       GD_EPISODE_STAT_COLLIDED_AGENTS, /* agents with collided_in_episode > 0 */
       GD_EPISODE_STAT_GOAL_ACHIEVED,   /* sum of info.goal_achieved */
       GD_EPISODE_STAT_TRUNCATED_AGENTS,
       GD_EPISODE_STAT_LENGTH_SUM,      /* sum of episode_lengths over ALL slots of the finished worlds */
       GD_EPISODE_STAT_TOTAL_COLLISIONS, GD_EPISODE_STAT_TOTAL_OFF_ROAD, /* sums over all slots */
       GD_EPISODE_STATS = 12 };
typedef struct gd_episode_config {
    float collision_weight, goal_achieved_weight, off_road_weight;
    int32_t reward_type;  /* GD_EPISODE_REWARD_* */
    int32_t auto_reset;   /* raise the reset flag of finished worlds and reset them (resetSystem + observations) */
    /* appended; zero-initialised they change nothing for the two reward types above */
    float log_distance_weight;  /* GD_EPISODE_REWARD_LOG_DISTANCE (reference default 0.01) */
    int32_t condition_mode;     /* GD_CONDITION_*: how a finished world's weights are redrawn (GD_EPISODE_REWARD_CONDITIONED) */
    float weights[3];           /* preset / fixed: collision, goal_achieved, off_road */
    float lb[3], ub[3];         /* random: bounds per component */
    uint64_t seed;              /* random: the generator's seed */
} gd_episode_config;
typedef struct gd_episode_buffers {
    const uint8_t *controlled_mask;  /* cont_agent_mask captured at t = 0 (bool) */
    /* running state, read and written */
    float *agent_episode_returns, *episode_lengths, *collided_in_episode, *offroad_in_episode;
    uint8_t *live_agent_mask;
    /* per-step outputs */
    float *reward_out;
    uint8_t *terminal_out, *truncated_out, *mask_out;
    int32_t *done_worlds;  /* [W] 1 for worlds whose episode ended in this step */
    float *stats;          /* [GD_EPISODE_STATS] running sums over finished episodes (the caller zeroes them) */
    float *world_stats;    /* [W][GD_EPISODE_STATS] the same for the last finished episode of each world */
    /* appended; required by GD_EPISODE_REWARD_CONDITIONED only */
    float *reward_weights;  /* [W][A][3] collision, goal_achieved, off_road weights of every agent slot */
    int32_t *weight_draws;  /* [W] draws of each world's weights so far (the generator's draw counter) */
    /* appended; optional flat outputs through the learner rows (gd_set_learner_rows), [n_rows] each: reward_out[mask],
     * terminal_out[mask], truncated_out[mask], mask_out[mask] bit for bit.  Any of them non-NULL without learner rows is
     * GD_ERR_INVALID. */
    float *reward_rows;
    uint8_t *terminal_rows, *truncated_rows, *mask_rows;
} gd_episode_buffers;
/* With GD_EPISODE_REWARD_CONDITIONED a finished world's reward_weights are redrawn in cfg->condition_mode by the same kernel,
 * before the reset pass, so the observation of the reset world carries its new weights (env_puffer.py:375-390). */
int gd_episode_step(gd_sim *sim, const gd_episode_config *cfg, const gd_episode_buffers *buffers);
/* Warm-up of the device auto-reset (the reference's init_steps: GPUDriveTorchEnv.reset -> advance_sim_with_log_playback,
 * gpudrive/env/env_torch.py:403-452, 1274-1293, also for the worlds PufferGPUDrive.step() resets, env_puffer.py:375-390).
 * With init_steps = k > 0 the reset pass that gd_episode_step launches with auto_reset advances every warmed world k state steps
 * (movement, collision, reward, step counter, done) after resetting the flagged ones; step t feeds every agent slot the logged
 * action of time t (what gd_advance_log_playback writes), and the observations are written once, at the end.  Scopes:
 *   GD_WARMUP_RESET_WORLDS: the worlds reset in this step, each ending bit for bit as gd_reset of it + gd_advance_log_playback(k)
 *                           leaves it; every other world is untouched.
 *   GD_WARMUP_ALL_WORLDS:   the reference as it is: when any world was reset, EVERY world is advanced k steps, as gd_reset(list) +
 *                           gd_advance_log_playback(k) do (the latter steps the whole batch).
 * The episode bookkeeping is unchanged (episode lengths count learner steps only).  k = 0 (the default) launches nothing extra.
 * Neither gd_reset nor any other reset pass is affected.  init_steps outside [0, 90] or an unknown scope: GD_ERR_INVALID. */
enum { GD_WARMUP_RESET_WORLDS = 0, GD_WARMUP_ALL_WORLDS = 1 };
int gd_episode_set_warmup(gd_sim *sim, int32_t init_steps, int32_t scope);
/* Draw the reward weights of the listed worlds (host array of n world indices; NULL = every world) in cfg->condition_mode
 * into buffers->reward_weights and count the draw in buffers->weight_draws (EpisodeTracker.set_reward_weights, the
 * reference's _set_reward_weights(env_idx_list, condition_mode, agent_type), env_torch.py:247-401). */
int gd_episode_draw_weights(gd_sim *sim, const gd_episode_config *cfg, const gd_episode_buffers *buffers,
                            const int32_t *worlds, int32_t n);

/* Block until everything launched so far has finished (the reference's step() is synchronous). */
int gd_sync(gd_sim *sim);
/* Change the launch stream (e.g. torch's current stream). */
int gd_set_stream(gd_sim *sim, void *stream);
/* Attach the BEV tensor after construction (replaces the reference's always-on BevObservations export,
 * src/mgr.cpp:870-880 + src/sim.cpp:462-555: there the raster exists from the start; here it is created on the first
 * bev_observation_tensor() call).  `bev` is a device buffer of gd_tensor_shape(GD_T_BEV) floats that the
 * caller keeps alive.  The rasters of the current state are computed at once; every later step / reset refreshes them. */
int gd_attach_bev(gd_sim *sim, float *bev);
/* Engine counters (tests and diagnostics).  which: 0 = steps replayed from the captured hipGraph,
 * 1 = steps launched kernel by kernel, 2 = hipGraph captures; the schedule the engine chose for this batch (it never
 * changes a result): 3 = set-order road kernel stores its rows itself (0 / 1), 4 = its agents per wave, 5 = live agents,
 * 6 = agents per wave of the reference-order road kernel (compile-time GD_MAP_OBS_AW of this build), 7 = the
 * reference-order road selection takes the rank replay (0 / 1).  Developer builds (tools/build_expt.sh) add 8 = the most
 * crowded ranking bucket (-DGD_DIAG with GPUDRIVE_RANK_DBG=9) and 10..17 = clock ticks per phase of k_knn_rank, then
 * 18..20 = k_knn_replay's rounds of its first wave / candidates beyond K / inserts (-DGD_CLOCKS; tools/rank_spikes.py),
 * all since the last read.  Every build: 21 = accesses the rank replay's bounds audit found out of range since its buffers
 * exist (must stay 0), 22 = checkpoint rows the rank replay's set-up kernel wrote in the last selection (agents that are not
 * bounded by their own checkpoints; every ranked agent with GPUDRIVE_RANK_SCAN_ROWS=1), 30 = agents whose road rows were left in place because their pose bits had not changed, since the last
 * read, 31 = BEV rasters painted by the last pass that rasterised (the others could not have changed and were left in
 * place), 44 = agents whose LiDAR returns the last pass marked for tracing (likewise), 45 = action indices outside the table
 * that gd_set_discrete_actions met since the simulator was created, 46 = worlds the warm-up of the device auto-reset
 * (gd_episode_set_warmup) advanced since the simulator was created, 47 = the state step runs the set-up of the rank replay's
 * selection itself (1; 0: the rank replay is off for this batch, or GPUDRIVE_RANK_SCAN_KERNEL=1 keeps it a launch of its
 * own).  Otherwise GD_ERR_INVALID. */
int gd_stat(gd_sim *sim, int32_t which, int64_t *out);

/* Timing hooks for the bench: HIP events around the named kernel on the engine's stream (a fixed ring of event pairs,
 * created by the enable call; steps run kernel by kernel, not from the hipGraph, while it is on).  Enabling again
 * while enabled zeroes the sums.  kernel: 0 = state step, 1 = road observation, 2 = LiDAR, 3 = BEV,
 * 4 = partner rows (on the engine's second stream, beside the road observation; no launches when they are written by the
 * state step, which is the default; GPUDRIVE_SPLIT_PARTNER=1 moves them there). */
int gd_kernel_timing_enable(gd_sim *sim, int32_t enable);
int gd_kernel_timing_read(gd_sim *sim, int32_t kernel, double *total_ms, int64_t *launches);

/* Internal agent state for teacher-forced parity tests: 11 floats per agent slot
 * {pos xyz, quat wxyz, vel xyz, collided}.  Device-to-host / host-to-device copies. */
int gd_debug_get_state(gd_sim *sim, float *host_out);
int gd_debug_set_state(gd_sim *sim, const float *host_in);
/* Which kernel selected every agent slot's roads in the last reference-order selection: > 0 the rank replay
 * (map_obs_rank.hip; the value is the agent's candidate count), -1 the history replay on keys (k_map_obs, the fallback:
 * first selection after a map change, jumps, overflow; -1 because another agent of its group of 32 needed it, -10 no usable
 * checkpoints or a world too small for the rank path, -11 more candidates than the buffer holds, -12 more than 32 equal keys, -13 the group bypasses the rank kernels
 * after three fallbacks in a row and retries every 64th selection), -3 no road of the world within reach of the radius (no rows),
 * 0 no selection (padding slot), -2 the rank replay is not in use (set order, linear scan, GPUDRIVE_NO_RANK_REPLAY).  out: [W][A] int32 on the host. */
int gd_debug_road_path(gd_sim *sim, int32_t *out);

/* Host-only scene pipeline (no device): parse + build world `scene` exactly as gd_create would
 * and return the init-time rows, for CPU tests of the host logic.
 * Replaces MapReader::parseAndWriteOut + createPersistentEntities (src/MapReader.cpp:55-61,
 * src/level_gen.cpp:396-465).  Caller frees with gd_host_world_free. */
typedef struct gd_host_world {
    int32_t num_agents, num_roads, num_collidable_roads, max_agents;
    float mean[3];
    int32_t map_name[32], scenario_id[32];
    float *map_obs;          /* [10000][9] */
    float *trajectory;       /* [A][1456] */
    int32_t *controlled, *response_type, *agent_id, *entity_type, *metadata /* [A][4] */;
    float *vehicle_size;     /* [A][3] */
    float *goal;             /* [A][2] */
} gd_host_world;
int gd_host_world_build(const char *scene, const gd_params *params, int32_t max_agents,
                        const int32_t *deleted_ids, int32_t n_deleted, gd_host_world *out);
void gd_host_world_free(gd_host_world *w);

/* Binary scene cache: parse `scene` (JSON) once the way MapReader::parseAndWriteOut +
 * from_json(Map) do (src/MapReader.cpp:46-61, src/json_serialization.hpp) and write the parsed, polyline-reduced
 * map to `out_path`, which must end in ".gdsm".  A ".gdsm" path is accepted wherever a scene path is (gd_create,
 * gd_set_maps, gd_host_world_build) and loads ~100x faster than the JSON; the worlds built from it are bit-identical.
 * The threshold is stored: asking for another one later is GD_ERR_INVALID.  Host only, no device needed. */
int gd_scene_cache_write(const char *scene, float polyline_reduction_threshold, const char *out_path);

#ifdef __cplusplus
}
#endif
#endif /* GPUDRIVE_AMD_H */
