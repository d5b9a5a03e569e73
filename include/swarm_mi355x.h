/*
 * swarm_mi355x.h — C-ABI of the MI355X-native vectorised drone-swarm step/observe/reward path.
 *
 * One call steps E independent swarm envs of N drones on the GPU (gfx950).  It replaces the
 * reference's per-env Python hot path:
 *
 *   swarm_step    <- DroneSwarmEnv.step            src/swarm_marl/envs/drone_swarm_env.py:92-174
 *                    (+ _clip_speed :179-183, _collision_mask :185-208,
 *                     _formation_penalties :210-224, _build_obs :226-243,
 *                     _nearest_neighbor_features :245-271, _nearest_obstacle_features :273-291,
 *                     _global_state :293-302)
 *                 <- DronePhysicsEnv.step          src/swarm_marl/envs/drone_physics_env.py:279-419
 *                    (point-mass restatement of the PyBullet force/substep loop :320-360,
 *                     _get_obs :421-462, _get_infos :540-583)
 *   swarm_reset   <- DroneSwarmEnv.reset           drone_swarm_env.py:65-90 (device RNG draws;
 *                    the seeded NumPy-stream reset stays on the host and uses swarm_observe)
 *                 <- DronePhysicsEnv.reset         drone_physics_env.py:174-263
 *   swarm_observe <- the observation/info half of reset(): drone_swarm_env.py:82-90
 *                    (_build_obs for every agent, distance_to_goal, global_state)
 *
 * Conventions
 *  - Every buffer is device memory owned by the caller (PyTorch tensors in the Python host
 *    package).  All buffers are dense, C-contiguous, and must not overlap each other.
 *  - Calls are asynchronous on `hip_stream` (a hipStream_t; NULL = the null stream).  No
 *    allocation, no host synchronisation, no exceptions cross the ABI: 0 on success, a negative
 *    SWARM_E* code otherwise; swarm_last_error() gives a thread-local message.
 *  - Reentrant for distinct state/out buffers.
 */
#ifndef SWARM_MI355X_H
#define SWARM_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWARM_ABI_VERSION 5

/* error codes */
#define SWARM_OK 0
#define SWARM_EINVAL -1    /* bad argument / unsupported configuration */
#define SWARM_ENULL -2     /* required pointer is NULL */
#define SWARM_ELIMIT -3    /* size exceeds a documented limit (N, K, Ms, LDS budget) */
#define SWARM_EHIP -4      /* HIP launch / runtime error */

/* dynamics modes */
#define SWARM_DYN_KINEMATIC 0         /* DroneSwarmEnv Euler integrator (drone_swarm_env.py:103-117) */
#define SWARM_DYN_POINTMASS_PHYSICS 1 /* DronePhysicsEnv force model as a point mass (drone_physics_env.py:320-360) */

/* reward modes */
#define SWARM_REW_SWARM 0    /* progress + formation + goal + collision (drone_swarm_env.py:137-172) */
#define SWARM_REW_PHYSICS 1  /* -0.1*dist, -10 collision, +50 goal (drone_physics_env.py:374-417) */

/* kernel selection (swarm_params_t.kernel_path) */
#define SWARM_PATH_AUTO 0     /* specialised kernels where they apply (swarm_step64 for the headline shape) */
#define SWARM_PATH_GENERIC 1  /* always the generic swarm_kernel (A/B parity checks, diagnostics) */

/* kernel actually launched (swarm_launch_info_t.kernel_id) */
#define SWARM_KERNEL_GENERIC 0  /* swarm_kernel<KIND, DYN, KS, MSL, LM> */
#define SWARM_KERNEL_STEP64 1   /* swarm_step64_once: N = 64, K = 3, Ms = 4, 4 <= M <= 16, kinematic step;
                                   one wave per env, 4 envs per workgroup (physics: swarm_step64_phys_once) */
#define SWARM_KERNEL_STEP64_PERSISTENT 2  /* swarm_step64: the same step on a persistent grid of
                                   waves_per_simd waves per SIMD with per-XCD env queues
                                   (E > grid; needs state.work, else STEP64 is launched) */
#define SWARM_KERNEL_STEP16Q 3  /* swarm_step16q: N = 16, K = 3, Ms = 4, 4 <= M <= 16, kinematic step; one
                                   env per 64-lane wave, four lanes per drone (BASELINE config 2) */
#define SWARM_KERNEL_STEP256 4  /* swarm_step256: N = 256, K = 3, Ms = 4, 4 <= M <= 16, kinematic step; one
                                   env per 256-thread workgroup, every pair evaluated once (BASELINE config 5) */

/* env_done bits ([E] u8) */
#define SWARM_ENV_TERMINATED 1u  /* terminated["__all__"] */
#define SWARM_ENV_TRUNCATED 2u   /* truncated["__all__"] */
#define SWARM_ENV_RESET 4u       /* the env was auto-reset in this call; obs/state are the new episode's */

/* info_flags bits ([E,N] u8) */
#define SWARM_AGENT_STEPPED 1u    /* agent had a reward/terminated/truncated entry this step */
#define SWARM_AGENT_REACHED 2u    /* infos["reached_goal"] */
#define SWARM_AGENT_COLLISION 4u  /* infos["collision"] */
#define SWARM_AGENT_HAS_OBS 8u    /* obs/infos entry emitted by the dict API (continuing agent) */

/*
 * Environment parameters.  Field meaning follows DroneEnvConfig (src/swarm_marl/envs/common.py:7-25)
 * plus `num_drones` (drone_swarm_env.py:32-34); floating fields are the Python (double) values,
 * the library derives the float32 constants the reference's NumPy code actually compares against.
 */
typedef struct swarm_params {
  int32_t abi_version;       /* must be SWARM_ABI_VERSION */
  int32_t num_envs;          /* E (local shard) */
  int32_t num_drones;        /* N, 1..1024 */
  int32_t num_obstacles;     /* M >= 0 */
  int32_t sensed_obstacles;  /* Ms (<= 16 supported); <= 0 -> no obstacle block in obs */
  int32_t neighbor_k;        /* K (<= 16 supported); <= 0 -> no neighbour block in obs */
  int32_t max_steps;
  int32_t dynamics;          /* SWARM_DYN_* */
  int32_t reward_mode;       /* SWARM_REW_* */
  int32_t auto_reset;        /* swarm_step: reset envs whose episode ended, in-kernel (device RNG) */
  int32_t physics_substeps;  /* physics: int(dt*240) (drone_physics_env.py:323) */
  int32_t damping_law;       /* physics: 0 = btMultiBody -d*(1+|v|)*v (default), 1 = btRigidBody v*=(1-d)^h */
  int64_t env_offset;        /* global index of local env 0 (RNG key; sharding across ranks) */
  uint64_t seed;             /* device-RNG key */
  double world_size;
  double dt;
  double max_speed;
  double max_accel;
  double collision_radius;
  double goal_radius;
  double obstacle_radius;
  double desired_spacing;
  double reward_progress_scale;
  double reward_goal;
  double reward_collision;
  double reward_formation_scale;
  /* physics-mode constants (drone_physics_env.py:135,343; drone.urdf geometry) */
  double gravity;            /* -9.81 */
  double gravity_comp;       /* 9.5 */
  double substep_dt;         /* 1/240 */
  double drone_contact_radius;    /* contact approximation radius of the 0.3x0.3x0.05 box */
  double ground_contact_height;   /* z at or below which the box touches the plane */
  int32_t kernel_path;       /* SWARM_PATH_* (default AUTO) */
  int32_t waves_per_simd;    /* 0 (default): swarm_step64_once, one wave per env; 1..8: persistent
                                swarm_step64 grid of that many waves per SIMD (needs state.work) */
} swarm_params_t;

/* Per-env state, device SoA blocks (all dense, C-contiguous). */
typedef struct swarm_state {
  float* pos;          /* [E,N,3] */
  float* vel;          /* [E,N,3] */
  float* goal;         /* [E,3] */
  float* obstacles;    /* [E,M,3] (may be NULL iff M == 0) */
  uint8_t* active;     /* [E,N]  agent still in env.agents */
  int32_t* step_count; /* [E] */
  uint32_t* episode;   /* [E]  device-RNG episode counter (incremented by every device reset) */
  float* damping;      /* [E,N] physics linear damping (NULL allowed in kinematic mode) */
  uint32_t* work;      /* [SWARM_WORK_WORDS] env-queue heads of the persistent swarm_step64: zeroed
                          once by the caller, left zeroed by every call; NULL = one workgroup per
                          env.  Belongs to this state: concurrent calls need distinct buffers. */
  struct swarm_env_cfg* env_cfg;             /* [E] per-env parameters (NULL: every env uses
                                                swarm_params_t); see swarm_env_cfg_set */
  const struct swarm_env_cfg* env_cfg_next;  /* [E] parameters of each env's NEXT episode: a reset
                                                (auto or swarm_reset) copies it into env_cfg before
                                                drawing.  NULL: episodes keep env_cfg.  Needs env_cfg. */
} swarm_state_t;

/*
 * Per-env parameters (curriculum stages configs/curriculum_v1.yaml:9-60 and
 * domain randomisation configs/domain_randomization_v1.yaml:9-57 as per-env tensors).  One 64-B
 * record per env, derived on the device by swarm_env_cfg_set from per-env values exactly as the
 * library derives the uniform constants from swarm_params_t, so that an env with record r behaves
 * bit-for-bit like a launch whose swarm_params_t carries r's values.  K, Ms, rewards and radii
 * other than the obstacle radius stay uniform (they fix the tensor shapes or are not randomised);
 * N fixes the slots per env, of which an env may use fewer (num_drones).
 * With env_cfg set, swarm_step launches the generic kernel (the step64 specialisation assumes
 * uniform parameters).
 */
typedef struct swarm_env_cfg {
  float half_w;          /* (float)(world_size / 2)  world clip and reset draw bounds */
  float neg_half_w;      /* (float)(-world_size / 2) */
  float width_w;         /* (float)world_size */
  float dt;              /* kinematic integrator step (physics: substeps stay uniform) */
  float max_speed;
  float max_accel;
  float s_vmax;          /* largest s with sqrtf(s) <= (float)max_speed */
  float s_obst;          /* same for (float)(collision_radius + obstacle_radius) */
  float s_phys_obst;     /* same for (float)(obstacle_radius + drone_contact_radius) */
  int32_t max_steps;
  int32_t num_obstacles; /* active obstacles, 0..swarm_params_t.num_obstacles (the state keeps M
                            slots; slots >= num_obstacles are zero and ignored) */
  int32_t num_drones;    /* drones of this env, 1..swarm_params_t.num_drones; 0 (what swarm_env_cfg_set
                            writes) = all of them.  Slots >= num_drones do not exist: see
                            swarm_env_cfg_set_drones */
  double max_speed_d;    /* max_speed as given (physics observation clamp) */
  double world_size;     /* as given (for readers) */
} swarm_env_cfg_t;

/* Per-env values for swarm_env_cfg_set: each pointer is a device array [E] or NULL (= the
 * swarm_params_t value for every env). */
typedef struct swarm_env_overrides {
  const double* world_size;
  const double* dt;
  const double* max_speed;
  const double* max_accel;
  const double* obstacle_radius;
  const int32_t* max_steps;
  const int32_t* num_obstacles;  /* clamped to [0, swarm_params_t.num_obstacles] */
} swarm_env_overrides_t;

#define SWARM_WORK_WORDS 256  /* 8 dequeue heads (one per XCD), one 128-B line each */

/* Outputs.  Optional pointers may be NULL. */
typedef struct swarm_out {
  float* obs;            /* [E,N,D], D = 9 + 4*max(K,0) + 4*max(Ms,0) */
  float* reward;         /* [E,N]   (0 for agents without a reward entry) */
  uint8_t* terminated;   /* [E,N] */
  uint8_t* truncated;    /* [E,N] */
  uint8_t* env_done;     /* [E]     SWARM_ENV_* bits */
  float* dist_goal;      /* [E,N]   optional: infos["distance_to_goal"] */
  uint8_t* info_flags;   /* [E,N]   optional: SWARM_AGENT_* bits */
  float* global_state;   /* [E,6N+3] optional: concat(pos, vel, goal) (drone_swarm_env.py:293-302) */
  const struct swarm_eval* eval;  /* optional HOST pointer to an eval tracker's state (swarm_eval_t,
                             its `flags` holding SWARM_EVAL_STEP_FUSED): the step accumulates the
                             evaluation protocol's per-step terms in its write-back — episode reward,
                             steps, first all-reached step, collision vote, path length — and
                             swarm_eval_update then adds only the formation error and closes the
                             ended episodes.  Kinematic swarm_step64 launches only (SWARM_KERNEL_STEP64
                             from swarm_query_launch, no env_cfg): other launches return SWARM_EINVAL */
} swarm_out_t;

/* Launch geometry actually used (for tests / profiling). */
typedef struct swarm_launch_info {
  int32_t threads_per_block;
  int32_t envs_per_block;
  int32_t lanes_per_env;
  int32_t blocks;
  int32_t lds_bytes;
  int32_t neighbor_slots;   /* compile-time top-K slots of the chosen kernel variant */
  int32_t obstacle_slots;
  int32_t obs_dim;
  int32_t staged_obs;       /* 1: obs staged through LDS and stored coalesced; 0: rows stored from
                               registers (small latency-bound launches, lanes_per_env != 64) */
  int32_t kernel_id;        /* SWARM_KERNEL_* swarm_step launches for these params (aligned buffers) */
} swarm_launch_info_t;

int swarm_abi_version(void);
const char* swarm_last_error(void);

/* Fill swarm_params_t with DroneEnvConfig defaults (common.py:9-24), num_drones = 3. */
void swarm_params_default(swarm_params_t* p);

/* Observation width D for `p` (drone_swarm_env.py:41-45). */
int swarm_obs_dim(const swarm_params_t* p);

/* Geometry of the kernel `swarm_step` would launch for `p`. */
int swarm_query_launch(const swarm_params_t* p, swarm_launch_info_t* info);

/*
 * One env step for every env: integrate, clip, distances, collision, formation, rewards,
 * terminations, (auto-reset), kNN observation, optional infos/global_state.
 * actions: [E,N,3] f32.  action_mask: [E,N] u8 or NULL (= every agent supplied an action;
 * a missing action is a zero action in swarm mode, no thrust in physics mode).
 * obs/global_state describe the state AFTER the call (post-reset for auto-reset envs).
 */
int swarm_step(const swarm_params_t* p, const swarm_state_t* s, const float* actions,
               const uint8_t* action_mask, const swarm_out_t* o, void* hip_stream);

/*
 * swarm_step for a batch split into env groups, one launch per group in one call (the batch's
 * env groups overlap on their streams: one group's launch burst and tail run beside the others'
 * steady state).  p / s / o / actions / action_mask describe the whole batch of p->num_envs envs;
 * group g is rows [lo_g, lo_g + group_envs[g]) (lo_g = the sum of the earlier groups), stepped on
 * hip_streams[g] exactly as swarm_step would step those rows with env_offset + lo_g — results are
 * bitwise those of one swarm_step over the batch.  group_envs must sum to p->num_envs.  s->work
 * (persistent kernel only), if set, holds `groups` x SWARM_WORK_WORDS words, one block per group.
 * No ordering between the streams is added: the caller makes every stream wait for the inputs.
 * Replaces the per-group Python launch loop (one ctypes call per step instead of G).
 */
int swarm_step_groups(const swarm_params_t* p, const swarm_state_t* s, const float* actions,
                      const uint8_t* action_mask, const swarm_out_t* o, int groups,
                      const int32_t* group_envs, void* const* hip_streams);

/*
 * Device reset: draw a new episode (Philox4x32-10 keyed by seed, global env index and
 * episode counter) for the envs with env_mask[e] != 0 (NULL = all) and write their obs,
 * dist_goal, global_state.  Outputs of envs not in the mask are left untouched.
 */
int swarm_reset(const swarm_params_t* p, const swarm_state_t* s, const uint8_t* env_mask,
                const swarm_out_t* o, void* hip_stream);

/*
 * Observation only: obs / dist_goal / global_state for the current state of the masked envs
 * (NULL = all).  The state is not modified.  Used after a host-side seeded reset.
 */
int swarm_observe(const swarm_params_t* p, const swarm_state_t* s, const uint8_t* env_mask,
                  const swarm_out_t* o, void* hip_stream);


/*
 * On-device actor inference: the reference's exported policy
 * (scripts/export_onnx.py:120-141: RLlib TorchFC, fcnet_hiddens [256, 256], relu;
 * src/swarm_marl/training/config_builders.py:53-56, models.py:75-81)
 *     logits = W3 relu(W2 relu(W1 x + b1) + b2) + b3,   logits = [mean | log_std]
 * run on the GPU over the env's observation tensor, writing logits and/or the next actions
 * (RLlib TorchDiagGaussian: deterministic = mean; sampled = mean + exp(log_std) * N(0, 1)).
 * It replaces the policy forward the reference runs on the host per agent
 * (algo.compute_single_action / the ONNX graph, scripts/evaluate_protocol.py:152-170).
 */
#define SWARM_POLICY_HIDDEN 256
#define SWARM_POLICY_MAX_IN 47      /* obs dim (one pad column carries the layer-1 bias) */
#define SWARM_POLICY_MAX_OUT 12     /* logits (2 x action dim) */
#define SWARM_POLICY_BF16 0         /* v_mfma_f32_32x32x16_bf16: bf16 operands, f32 accumulation */
#define SWARM_POLICY_F32 1          /* v_mfma_f32_16x16x4_f32: f32 operands and sums */
#define SWARM_POLICY_F32X3 2        /* v_mfma_f32_32x32x16_f16, three passes: every f32 operand split
                                       into f16 hi + lo, products hi*hi + hi*lo + lo*hi (~2^-21
                                       relative per product: the f32 path's tolerance at f16-MFMA
                                       speed); obs, weights and activations must be < 65504 in
                                       magnitude (f16 range).  swarm_policy_pack returns SWARM_EINVAL
                                       and leaves host_out untouched when a W1, b1, W2 or W3 entry is
                                       not finite or rounds past 65504 in f16 (|v| >= 65520); b2 and
                                       b3 stay f32 and are not checked */
#define SWARM_POLICY_ACT_MEAN 0     /* actions = mean (deterministic) */
#define SWARM_POLICY_ACT_SAMPLE 1   /* actions = mean + exp(log_std) * N(0,1), Philox(seed; row, counter); every
                                       precision, the same normals in each */

typedef struct swarm_policy {
  int32_t in_dim;        /* observation width D */
  int32_t out_dim;       /* logits width (even) */
  int32_t precision;     /* SWARM_POLICY_BF16 / SWARM_POLICY_F32 / SWARM_POLICY_F32X3 */
  int32_t reserved;
  const void* weights;   /* device copy of the swarm_policy_pack blob (16-B aligned) */
} swarm_policy_t;

/* Bytes of the packed weight blob (negative SWARM_E* code for unsupported dims). */
long long swarm_policy_packed_bytes(int in_dim, int out_dim, int precision);

/* Pack row-major f32 weights (PyTorch / ONNX Gemm transB layout: w1 [256,in], w2 [256,256],
 * w3 [out,256]) into the kernel's fragment-order blob at host_out (host memory). */
int swarm_policy_pack(int in_dim, int out_dim, int precision, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* w3, const float* b3, void* host_out);

/* logits [rows,out] (nullable) and/or actions [rows,out/2] (nullable) for obs [rows,in]; async on
 * hip_stream, no allocation, no sync.  SWARM_POLICY_ACT_SAMPLE works in every precision: row r
 * draws its normals from Philox(seed; r, counter) whatever the precision (and in
 * swarm_attn_policy_forward), and a = mean + expf(log_std) * z is formed in the same f32 order, so
 * equal logits give equal actions bit for bit.  The logits written are those of a mean-mode launch. */
int swarm_policy_forward(const swarm_policy_t* p, const float* obs, long long rows, float* logits, float* actions,
                         int action_mode, unsigned long long seed, unsigned long long counter, void* hip_stream);

const char* swarm_policy_last_error(void);

/*
 * Training the SWARM_POLICY_BF16 actor on the device (csrc/swarm_train.hip): float32 master weights
 * stay with the caller (torch parameters under Adam); the forward is swarm_policy_forward itself, the
 * backward below runs on the same bf16 MFMA operands with f32 accumulation, and a device packer
 * rebuilds the inference blob from the masters.  All calls are async on hip_stream, allocate nothing,
 * read nothing back, use no atomics and launch grids that depend on `rows` only (never on the
 * device's CU count), so a call repeats bit for bit.  Errors via swarm_policy_train_last_error,
 * before any launch.  Limits are the bf16 policy's: in_dim 1..SWARM_POLICY_MAX_IN, out_dim even in
 * 2..SWARM_POLICY_MAX_OUT, anything else SWARM_ELIMIT.
 *
 * Notation: bf(v) is v rounded to bf16, round to nearest even.  x~ is the obs row widened with
 * x~[in_dim] = 1 (the bias column).  W1~ = [W1 | b1].  Every product below is of two bf16 values (exact
 * in f32) and every sum is an f32 MFMA accumulation.
 *
 * swarm_policy_backward, per row r (obs must be finite; the weights too):
 *     h1 = relu(bf(bf(W1~) bf(x~)))                  the inference kernel's h1: the same fragments, the
 *     h2 = relu(bf(bf(W2) h1 + b2))                  same MFMA order, relu after the rounding
 *     g  = bf(grad_logits[r])
 *     dz2 = bf(bf(W3)^T g) where h2 > 0, else 0      16 terms per sum (m >= out_dim are zeros)
 *     dz1 = bf(bf(W2)^T dz2) where h1 > 0, else 0    256 terms, o = 0..255 in 16 k-steps of 16
 * and over the rows, in f32:
 *     dW3[m][u] = sum_r g[m] h2[u]      db3[m] = sum_r g[m]
 *     dW2[o][i] = sum_r dz2[o] h1[i]    db2[o] = sum_r dz2[o]
 *     dW1[o][k] = sum_r dz1[o] bf(x[k]) db1[o] = sum_r dz1[o]     (db1 is column in_dim of dz1 x~^T)
 * Reduction order of every one of those sums: rows are padded to a multiple of 32 (a padded row has
 * g = 0: every dz of it is exactly 0); slab s holds rows [SWARM_TRAIN_SLAB s, SWARM_TRAIN_SLAB (s + 1));
 * a slab's partial sum is one MFMA accumulator chain over its rows in ascending 16-row k-steps (the bias
 * sums are the same chain against a B operand of ones); the result is partial 0 + partial 1 + ... in
 * slab order.  So the longest chain of f32 additions behind an element is
 *     L = SWARM_TRAIN_SLAB + nslabs - 1,   nslabs = ceil(rows / SWARM_TRAIN_SLAB)
 * and |error| <= L 2^-24 sum|terms| against the exact sum of the same bf16 products.
 * A row whose grad_logits are all zero adds exactly zero to every gradient (the collector writes zero
 * obs rows for invalid agents and the loss head zero gradients).  rows == 0 is a no-op: nothing is
 * written.  Gradients are written, not accumulated into.
 *
 * Launches: (a) h1, h2, dz2 and (b) dz1, one wave per 32-row tile, 8 waves per workgroup, at most
 * SWARM_TRAIN_MAX_BLOCKS workgroups (further tiles in further passes); (c) three weight-gradient
 * launches of one workgroup per slab; (d) the finalising sum, one thread per gradient element.
 */
#define SWARM_TRAIN_SLAB 1024        /* rows per weight-gradient slab */
#define SWARM_TRAIN_MAX_BLOCKS 256   /* workgroups of the tile launches (a) and (b) */
#define SWARM_TRAIN_MAX_ROWS (1LL << 28)  /* rows of one backward call (32-bit lane offsets); more: SWARM_ELIMIT */

/* Bytes of the training workspace for backward calls of up to `rows` rows (negative SWARM_E* code for
 * unsupported dims or rows < 0).  Its first bytes hold the packer's transposed blobs: the workspace a
 * backward call is given must be the one the last swarm_policy_pack_device wrote. */
long long swarm_policy_train_workspace_bytes(int in_dim, int out_dim, long long rows);

/*
 * Device packer, one launch.  Reads the six float32 master arrays (device memory, PyTorch layout:
 * w1 [256,in], b1 [256], w2 [256,256], b2 [256], w3 [out,256], b3 [out]) and writes
 *   - `weights` (device, swarm_policy_packed_bytes(in, out, SWARM_POLICY_BF16) bytes, 16-B aligned):
 *     byte for byte what swarm_policy_pack writes for the same arrays — bf16 round to nearest even,
 *     W1 with b1 in column `in`, W2 / W3 in the accumulator-chained k order, b2 / b3 in f32, zeros
 *     in the padding.  Written in place: a swarm_policy_t pointing at it stays valid.
 *   - the head of `workspace` (16-B aligned): bf(W2)^T and bf(W3)^T in MFMA-fragment order for
 *     swarm_policy_backward.
 */
int swarm_policy_pack_device(int in_dim, int out_dim, const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* w3, const float* b3, void* weights, void* workspace, void* hip_stream);

typedef struct swarm_policy_backward_args {
  const void* weights;       /* the SWARM_POLICY_BF16 blob (device, 16-B aligned) */
  const float* obs;          /* [rows, in_dim] finite */
  const float* grad_logits;  /* [rows, out_dim] */
  void* workspace;           /* swarm_policy_train_workspace_bytes(.., rows) bytes, 16-B aligned, private
                                to the call while it runs, head written by swarm_policy_pack_device */
  float* dw1;                /* [256, in_dim] */
  float* db1;                /* [256] */
  float* dw2;                /* [256, 256] */
  float* db2;                /* [256] */
  float* dw3;                /* [out_dim, 256] */
  float* db3;                /* [out_dim] */
  uint16_t* h1;              /* optional stage outputs: bf16 bit patterns [rows, 256], row-major, natural */
  uint16_t* h2;              /* unit order, 8-B aligned; NULL: nothing extra is written */
  uint16_t* dz2;
  uint16_t* dz1;
  long long rows;
  int32_t in_dim, out_dim;
} swarm_policy_backward_args_t;

int swarm_policy_backward(const swarm_policy_backward_args_t* args, void* hip_stream);

const char* swarm_policy_train_last_error(void);

/*
 * On-device attention actor: the reference's CentralizedCriticModel(use_attention=True) actor
 * (src/swarm_marl/training/models.py:104-137, scripts/train_attention.py), eval mode.  For one
 * observation row x of width D = 9 + 4K + 4Ms, own = x[0:9], nb_j = x[9+4j : 13+4j] (j < K),
 * obst = x[9+4K : D]:
 *     o   = relu(W_own own + b_own)                     (32)   own_embed.0
 *     e_j = relu(W_nb nb_j + b_nb)                      (32)   neighbor_embed.0
 *     q = Wq o + bq,  k_j = Wk e_j + bk,  v_j = Wv e_j + bv    in_proj rows 0:32, 32:64, 64:96
 *     a = softmax_j(q . k_j / sqrt(32)),  c = Wout (sum_j a_j v_j) + bout
 *     logits = W3 relu(W2 relu(W1 [own | c | obst] + b1) + b2) + b3      (W1 [256, 41 + 4Ms])
 * Every one of the K neighbour slots is attended to, a zero-filled one included.
 * K in 1..SWARM_ATTN_MAX_K, Ms in 0..SWARM_ATTN_MAX_MS, out_dim even in 2..SWARM_POLICY_MAX_OUT;
 * anything else is SWARM_ELIMIT.  precision: SWARM_POLICY_BF16 or SWARM_POLICY_F32
 * (SWARM_POLICY_F32X3: SWARM_ELIMIT).
 *
 * SWARM_POLICY_F32 evaluates the formulas above as written (f32 products and sums).
 * SWARM_POLICY_BF16 is one fused launch on two exact identities, folded by the packer in double:
 *     score_j = (A o + c0) . e_j + (terms equal for every j),  A = Wk^T Wq / sqrt(32),
 *                                                              c0 = Wk^T bq / sqrt(32)
 *     W1[:, 9:41] c = F s + d,   s = sum_j a_j e_j,   F = W1[:, 9:41] Wout Wv,
 *                                                     d = W1[:, 9:41] (Wout bv + bout)
 * The front end (o, A o + c0, e_j, the softmax with the running row maximum subtracted, s) runs in f32; the
 * trunk runs on v_mfma_f32_32x32x16_bf16 with f32 accumulation over the 64-wide layer-1 input
 * [s (32) | own (9) | obst (4Ms) | 1 | 0...], whose weights [F | W1[:, 0:9] | W1[:, 41:] | b1 + d]
 * are rounded to bf16 once.
 *
 * bf16 blob layout (bytes; `out` = out_dim): W2 fragments at 0 (131072), W3 fragments (512 out),
 * b2 (1024), b3 (128), layer-1 fragments (32768), then the f32 front end: W_own [32,9], b_own [32],
 * W_nb [32,4], b_nb [32], A [32,32] (row i, column m: t_i = c0_i + sum_m A[i][m] o_m), c0 [32].
 * Fragment order is swarm_policy_pack's; layer-1 fragment column k < 32 carries
 * s[16 ((k >> 3) & 1) + 8 (k >> 4) + (k & 7)], column 32 + t the t-th of [own | obst | 1].
 */
#define SWARM_ATTN_EMBED 32         /* embed_dim of the reference's attention block (one head) */
#define SWARM_ATTN_MAX_K 16         /* neighbour slots */
#define SWARM_ATTN_MAX_MS 5         /* sensed obstacles: 41 + 4 Ms + the bias column fit a 64-wide K */

typedef struct swarm_attn_policy {
  int32_t neighbor_k;        /* K */
  int32_t sensed_obstacles;  /* Ms */
  int32_t out_dim;           /* logits width (even) */
  int32_t precision;         /* SWARM_POLICY_BF16 / SWARM_POLICY_F32 */
  const void* weights;       /* device copy of the swarm_attn_policy_pack blob (16-B aligned) */
} swarm_attn_policy_t;

/* Row-major f32 parameters (PyTorch layouts), named after the reference's state_dict. */
typedef struct swarm_attn_weights {
  const float* neighbor_w;   /* neighbor_embed.0.weight [32,4] */
  const float* neighbor_b;   /* neighbor_embed.0.bias [32] */
  const float* own_w;        /* own_embed.0.weight [32,9] */
  const float* own_b;        /* own_embed.0.bias [32] */
  const float* in_proj_w;    /* attn_block.attn.in_proj_weight [96,32] */
  const float* in_proj_b;    /* attn_block.attn.in_proj_bias [96] */
  const float* out_proj_w;   /* attn_block.attn.out_proj.weight [32,32] */
  const float* out_proj_b;   /* attn_block.attn.out_proj.bias [32] */
  const float* w1;           /* trunk [256, 41 + 4Ms] */
  const float* b1;
  const float* w2;           /* [256,256] */
  const float* b2;
  const float* w3;           /* [out,256] */
  const float* b3;
} swarm_attn_weights_t;

/* Bytes of the packed weight blob (negative SWARM_E* code for unsupported dims). */
long long swarm_attn_policy_packed_bytes(int neighbor_k, int sensed_obstacles, int out_dim, int precision);

/* Fold (double) and pack the parameters into the kernel's blob at host_out (host memory). */
int swarm_attn_policy_pack(int neighbor_k, int sensed_obstacles, int out_dim, int precision,
                           const swarm_attn_weights_t* w, void* host_out);

/* logits [rows,out] (nullable) and/or actions [rows,out/2] (nullable) for obs [rows,D]; async on
 * hip_stream, no allocation, no sync.  rows == 0 is a no-op.  SWARM_POLICY_ACT_SAMPLE draws the
 * normals of swarm_policy_forward at the same (seed, row, counter), in either precision. */
int swarm_attn_policy_forward(const swarm_attn_policy_t* p, const float* obs, long long rows, float* logits,
                              float* actions, int action_mode, unsigned long long seed, unsigned long long counter,
                              void* hip_stream);

const char* swarm_attn_policy_last_error(void);

/*
 * On-device centralized critic (the reference's CTDE value function: CentralizedCriticModel's
 * `value_model`, a TorchFC [256, 256] on global_state of width G = 6N + 3 with one output;
 * src/swarm_marl/training/models.py):
 *     value[r] = W3 relu(W2 relu(W1 gs[r] + b1) + b2) + b3
 * over rows of global_state read in place (swarm_out_t.global_state, or any [rows, in_dim] f32
 * block).  precision: SWARM_POLICY_BF16 (bf16 MFMA operands, f32 accumulation; W1 streams from
 * L2 in fragment order) or SWARM_POLICY_F32 (f32 products and sums); SWARM_POLICY_F32X3 is
 * rejected with SWARM_ELIMIT.
 */
#define SWARM_CRITIC_MAX_IN 1539    /* 6 * 256 + 3 */

typedef struct swarm_critic {
  int32_t in_dim;        /* global_state width G */
  int32_t precision;     /* SWARM_POLICY_BF16 / SWARM_POLICY_F32 */
  const void* weights;   /* device copy of the swarm_critic_pack blob (16-B aligned) */
} swarm_critic_t;

/* Bytes of the packed weight blob (negative SWARM_E* code if unsupported). */
long long swarm_critic_packed_bytes(int in_dim, int precision);

/* Pack row-major f32 weights (PyTorch layout: w1 [256,in], w2 [256,256], w3 [1,256]) into the
 * kernel's blob at host_out (host memory). */
int swarm_critic_pack(int in_dim, int precision, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* w3, const float* b3, void* host_out);

/* value [rows] for gs [rows,in_dim]; async on hip_stream, no allocation, no sync.  rows == 0 is a
 * no-op. */
int swarm_critic_forward(const swarm_critic_t* c, const float* gs, long long rows, float* value, void* hip_stream);

const char* swarm_critic_last_error(void);

/*
 * RLlib TorchDiagGaussian.logp of `actions` [rows,adim] under logits [rows,2*adim] = [mean | log_std]:
 *     logp = sum_k(-0.5 z_k^2 - log_std_k) - 0.5 adim log(2 pi),   z_k = (a_k - mean_k) exp(-log_std_k)
 * (the unclipped sampled action, as RLlib stores it).  Async; errors via swarm_critic_last_error.
 */
int swarm_gaussian_logp(const float* logits, const float* actions, long long rows, int adim, float* logp,
                        void* hip_stream);

/*
 * Generalized advantage estimation over a fragment of T steps of E envs x N agents.  One thread
 * per (e, n) walks t = T-1 .. 0 in f32, in exactly this order (no fused multiply-add):
 *     gl = gamma * lam;  carry = 0
 *     if !valid[t,e,n]: advantage = value_target = 0; carry = 0; continue
 *     done  = terminated[t,e,n] | truncated[t,e,n] | (env_done[t,e] & (TERMINATED | TRUNCATED)) != 0
 *     nv    = done ? 0 : value[t+1,e];   prev = done ? 0 : carry
 *     delta = (reward[t,e,n] + gamma * nv) - value[t,e]
 *     carry = delta + gl * prev
 *     advantage[t,e,n] = carry;  value_target[t,e,n] = carry + value[t,e]
 * value [T+1,E] is V(global_state) before step t, shared by the env's agents; row T bootstraps
 * the fragment end.  Any episode end (the agent's own termination or truncation, or the env's
 * __all__) stops the bootstrap.  Async; errors via swarm_critic_last_error.
 */
int swarm_gae(const float* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated,
              const uint8_t* env_done, const uint8_t* valid, int T, int E, int N, float gamma, float lam,
              float* advantage, float* value_target, void* hip_stream);

/*
 * On-device per-agent critic (csrc/swarm_value.hip): the value tower of RLlib's default TorchFC with
 * vf_share_layers=False (the reference's build_multi_agent_ppo_config / build_single_agent_ppo_config,
 * src/swarm_marl/training/config_builders.py: fcnet_hiddens [256, 256], relu), evaluated on each
 * agent's own observation row:
 *     value[r] = W3 relu(W2 relu(W1 obs[r] + b1) + b2) + b3          (obs -> 256 -> 256 -> 1)
 * in_dim is 1 .. SWARM_POLICY_MAX_IN (anything else: SWARM_ELIMIT).  precision:
 *   SWARM_POLICY_BF16  the actor kernel's design with a one-output last layer: the whole blob
 *       (W1 and W2 in MFMA-fragment order, b2, w3, b3: 157,712 B) is staged in LDS once per
 *       workgroup; one wave per 32-row tile computes layers 1 and 2 transposed on
 *       v_mfma_f32_32x32x16_bf16 (bf16 operands, f32 accumulation; the layer-1 bias rides in the pad
 *       column k = in_dim, x = 1; relu'd accumulators re-rounded to bf16 are layer 2's B operand);
 *       layer 3 is relu(h2) rounded to bf16 times the bf16-rounded w3 in f32 on the VALU (no fused
 *       multiply-add), summed per lane over out blocks 0 .. 7 and registers 0 .. 15 in that order,
 *       the two lane halves joined by one cross-half add, plus b3.  A value depends on its own row
 *       only: the same row gives the same bits wherever it sits in a tile or in the grid.
 *   SWARM_POLICY_F32   parity with an f32 learner, no speed claim: swarm_critic_pack's f32 blob and
 *       swarm_critic_forward's f32 kernel at this in_dim.
 *   SWARM_POLICY_F32X3 is rejected with SWARM_ELIMIT.
 * Rows past `rows` are read from clamped addresses and never written.
 */
typedef struct swarm_value {
  int32_t in_dim;        /* observation width D */
  int32_t precision;     /* SWARM_POLICY_BF16 / SWARM_POLICY_F32 */
  const void* weights;   /* device copy of the swarm_value_pack blob (16-B aligned) */
} swarm_value_t;

/* Bytes of the packed weight blob (negative SWARM_E* code if unsupported). */
long long swarm_value_packed_bytes(int in_dim, int precision);

/* Pack row-major f32 weights (PyTorch layout: w1 [256,in], w2 [256,256], w3 [1,256]) into the
 * kernel's blob at host_out (host memory). */
int swarm_value_pack(int in_dim, int precision, const float* w1, const float* b1, const float* w2,
                     const float* b2, const float* w3, const float* b3, void* host_out);

/* value [rows] for obs [rows,in_dim]; async on hip_stream, no allocation, no sync.  rows == 0 is a
 * no-op. */
int swarm_value_forward(const swarm_value_t* v, const float* obs, long long rows, float* value, void* hip_stream);

/*
 * swarm_gae with a per-agent value [T+1,E,N] (row t: V(obs[t,e,n]) before step t; row T bootstraps
 * the fragment end).  One thread per (e, n) walks t = T-1 .. 0 in f32, in exactly this order (no
 * fused multiply-add):
 *     gl = gamma * lam;  carry = 0
 *     if !valid[t,e,n]: advantage = value_target = 0; carry = 0; continue
 *     done  = terminated[t,e,n] | truncated[t,e,n] | (env_done[t,e] & (TERMINATED | TRUNCATED)) != 0
 *     nv    = done ? 0 : value[t+1,e,n];   prev = done ? 0 : carry
 *     delta = (reward[t,e,n] + gamma * nv) - value[t,e,n]
 *     carry = delta + gl * prev
 *     advantage[t,e,n] = carry;  value_target[t,e,n] = carry + value[t,e,n]
 * value[t,e,n] is not read when valid[t,e,n] == 0, value[t+1,e,n] is not read when the step is
 * invalid or done (either may be NaN).  Any episode end stops the bootstrap, a truncation included.
 * Async; errors via swarm_value_last_error.
 */
int swarm_gae_agent(const float* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated,
                    const uint8_t* env_done, const uint8_t* valid, int T, int E, int N, float gamma, float lam,
                    float* advantage, float* value_target, void* hip_stream);

const char* swarm_value_last_error(void);

/*
 * Actuation and sensing perturbations (csrc/swarm_perturb.hip): the control delay, thrust noise and
 * sensing noise of the reference's configs/domain_randomization_v1.yaml, as a layer before and
 * after the env step.  swarm_step itself is unchanged: swarm_actuate turns the policy's actions into
 * the actions the step is given, swarm_sense turns the step's obs into the obs the policy sees.
 * Both are one async launch on hip_stream, allocate nothing, do not synchronise and keep no host
 * state; every argument is a device pointer or a constant.  num_envs == 0 is a no-op.  Errors via
 * swarm_perturb_last_error, before any launch.
 *
 * Noise: Philox4x32-10 with key (seed lo, seed hi) on the counter words
 *     (g, n | block << 16 | stream << 30, episode[e], step)
 * g = (uint32)(env_offset + e) the global env index, n the agent slot, episode[e] and
 * step = step_count[e] read from the env state (swarm_state_t) when the kernel runs; stream 0
 * actuation, 1 sensing, 2 the delay draw.  A block x0..x3 gives four normals, pair (x0, x1) z0, z1
 * and pair (x2, x3) z2, z3, in f32:
 *     u1 = ((x >> 8) + 0.5) * 2^-24;  u2 = (x' >> 8) * 2^-24;  r = sqrtf(-2 logf(u1))
 *     z = r cosf(2 pi u2),  z' = r sinf(2 pi u2)              (2 pi = 6.28318530717958647692f)
 * So the noise depends on (seed, global env, agent, episode, step) only: not on the calls made
 * before, on how the envs are split into groups, or on env_offset shards.
 */
#define SWARM_PERTURB_MAX_DELAY 7      /* control delay in steps */
#define SWARM_PERTURB_MAX_AGENTS 256   /* N */
#define SWARM_PERTURB_MAX_K 16         /* neighbour slots */
#define SWARM_PERTURB_MAX_MS 5         /* sensed obstacles */

/* The discrete delay distribution: `count` values with cum[i] = (float)(probs[0] + .. + probs[i])
 * (the sum in double), cum[count - 1] == 1. */
typedef struct swarm_delay_table {
  int32_t count;                                  /* 1 .. SWARM_PERTURB_MAX_DELAY + 1 */
  int32_t values[SWARM_PERTURB_MAX_DELAY + 1];    /* each in [0, ring_slots) */
  float cum[SWARM_PERTURB_MAX_DELAY + 1];
} swarm_delay_table_t;

/*
 * swarm_actuate, per env e and agent n, with s = step_count[e] (the episode step about to be taken):
 *     d = delay_override[e] if delay_override and delay_override[e] >= 0, else values[i] for the
 *         first i with u < cum[i], u = (x0 >> 8) * 2^-24 of the block (g, 2 << 30, episode[e], 0)
 *         (one draw per env and episode; a single-entry table draws nothing); d = min(d, ring_slots - 1)
 *     c = fminf(fmaxf(actions[e,n,:], -1), 1);   ring[s % ring_slots, e, n, :] = c
 *     u = ring[(s - d) % ring_slots, e, n, :] if d <= s else 0   (nothing commanded yet this episode)
 *     eff[e,n,k] = u_k + thrust_noise_std[e] * z_k, k = 0..2, z of block 0 of stream 0 at step s;
 *                  u_k itself, bit for bit, where thrust_noise_std is NULL or 0 for the env
 *     delay_out[e] = d                                        (if delay_out is not NULL)
 * The noise goes in before the env's own clip to [-1, 1].  A new episode (step_count back at 0, a
 * new episode number: an auto-reset or swarm_reset) draws a new delay and starts an empty line with
 * no host action.  Call it once per step, before swarm_step, from the first step of an episode on.
 * With actions == NULL (then ring and eff must be NULL too) only delay_out is written.
 */
typedef struct swarm_actuate_args {
  const float* actions;           /* [E,N,3] the policy's actions */
  float* ring;                    /* [ring_slots,E,N,3] the delay line, owned by the caller */
  const int32_t* delay_override;  /* [E] fixed delay, -1: draw; NULL: draw everywhere */
  const float* thrust_noise_std;  /* [E]; NULL: none */
  const int32_t* step_count;      /* [E] swarm_state_t.step_count */
  const uint32_t* episode;        /* [E] swarm_state_t.episode */
  float* eff;                     /* [E,N,3] what swarm_step is given */
  int32_t* delay_out;             /* [E] or NULL */
  swarm_delay_table_t delays;
  int32_t ring_slots;             /* R in [1, SWARM_PERTURB_MAX_DELAY + 1], > every table value */
  int32_t num_envs, num_drones;   /* E >= 0, N in [1, SWARM_PERTURB_MAX_AGENTS] */
  int32_t reserved;
  uint64_t seed;
  int64_t env_offset;             /* global index of env 0 */
} swarm_actuate_args_t;

int swarm_actuate(const swarm_actuate_args_t* args, void* hip_stream);

/*
 * swarm_sense: out [E,N,D] from obs [E,N,D], D = 9 + 4 K + 4 Ms, row layout
 * [pos 3 | vel 3 | goal - pos 3 | K x (rel 3, dist) | Ms x (rel 3, dist)]; obs is not written and
 * out is another buffer.  step = step_count[e] and episode[e] as they stand after the step or reset
 * that produced obs; sp / sv / so the env's position / velocity / obstacle std; f32 without fused
 * multiply-add:
 *   own block     n_k = sp z_k (block 0);  pos'_k = pos_k + n_k;  (goal - pos)'_k = (goal - pos)_k - n_k
 *                 vel'_k = vel_k + sv z_k (block 1)
 *   neighbour j   rel'_k = rel_k + sp z_k (block 2 + j);  dist' = sqrtf((x' x' + y' y') + z' z')
 *   obstacle j    dist' = fmaxf(dist + so z0, 0) (block 2 + K + j); the vector stays
 * Copied bit for bit: rows with active[e,n] == 0, neighbour and obstacle slots whose four floats are
 * all zero (the padding of K > N - 1 or Ms > M), and every group whose std is NULL or 0 for the env.
 * The same state gives the same out.
 */
typedef struct swarm_sense_args {
  const float* obs;                 /* [E,N,D] */
  const uint8_t* active;            /* [E,N] swarm_state_t.active */
  const float* position_noise_std;  /* [E]; NULL: none */
  const float* velocity_noise_std;  /* [E]; NULL: none */
  const float* obstacle_noise_std;  /* [E]; NULL: none */
  const int32_t* step_count;        /* [E] */
  const uint32_t* episode;          /* [E] */
  float* out;                       /* [E,N,D] */
  uint64_t seed;
  int64_t env_offset;
  int32_t num_envs, num_drones;     /* E >= 0, N in [1, SWARM_PERTURB_MAX_AGENTS] */
  int32_t neighbor_k;               /* K in [0, SWARM_PERTURB_MAX_K] */
  int32_t sensed_obstacles;         /* Ms in [0, SWARM_PERTURB_MAX_MS] */
} swarm_sense_args_t;

int swarm_sense(const swarm_sense_args_t* args, void* hip_stream);

const char* swarm_perturb_last_error(void);

/*
 * Rollout fragments as one replayed graph (csrc/swarm_rollout.hip): sampling with the Philox counter
 * in device memory, and the per-step copies of a fragment in one launch.  Both are one async launch
 * on hip_stream, allocate nothing, do not synchronise, use no atomics and repeat bit for bit;
 * errors via swarm_rollout_last_error, before any launch.
 */
#define SWARM_ROLLOUT_MAX_ACT 6        /* act_dim: the actors' out_dim / 2 */
#define SWARM_ROLLOUT_MAX_SEGMENTS 8   /* segments of one record launch */

/*
 * actions [rows, A] from logits [rows, 2A] = [mean | log_std], A = act_dim in 1..6:
 *     counter = (counter_dev ? *counter_dev : 0) + counter_add      (64-bit: the low word's carry
 *               goes into the high word; the sum wraps at 2^64)
 *     z_0..5  = the normals of row r from Philox(seed; r, counter), as SWARM_POLICY_ACT_SAMPLE draws them
 *     actions[r, k] = logits[r, k] + expf(logits[r, A + k]) * z_k   (f32, the product rounded first)
 * the expression and order of swarm_policy_forward and swarm_attn_policy_forward in
 * SWARM_POLICY_ACT_SAMPLE, so for the logits those write, the same seed and the same counter this
 * gives their actions bit for bit.  counter_dev is a device pointer to one 64-bit word (8-byte
 * aligned), read when the kernel runs: a captured launch follows the word from replay to replay.
 * counter_dev NULL: the counter is counter_add.  rows == 0 is a no-op.  One lane per row.
 */
int swarm_rollout_sample(const float* logits, long long rows, int act_dim, unsigned long long seed,
                         const unsigned long long* counter_dev, unsigned long long counter_add, float* actions,
                         void* hip_stream);

typedef struct swarm_rollout_segment {
  const void* src;   /* device */
  void* dst;         /* device; NULL: the segment is skipped */
  uint64_t bytes;    /* 0: the segment is skipped */
} swarm_rollout_segment_t;

/*
 * Copy every segment, dst[0, bytes) = src[0, bytes), in one launch: nothing outside [dst, dst + bytes)
 * is written.  Any alignment: a segment whose src and dst are both 16-byte aligned moves in 16-byte
 * loads and stores (and a tail), one whose src and dst are both 4-byte aligned in 4-byte ones, any
 * other byte by byte.  The segments of one call must not overlap each other, and no dst range may
 * overlap any src range: the order in which bytes move is not defined.  count == 0, or every segment
 * skipped, is a no-op.
 */
typedef struct swarm_rollout_record {
  int32_t count;     /* 0 .. SWARM_ROLLOUT_MAX_SEGMENTS */
  int32_t reserved;
  swarm_rollout_segment_t segments[SWARM_ROLLOUT_MAX_SEGMENTS];
} swarm_rollout_record_t;

int swarm_rollout_record(const swarm_rollout_record_t* record, void* hip_stream);

const char* swarm_rollout_last_error(void);

/*
 * PPO loss head (csrc/swarm_ppo.hip): RLlib's PPOTorchPolicy.loss over a collected fragment, value
 * and gradient in one pass.  Rows are grouped by env-row: an env-row is one (t, e) with its N
 * consecutive agent rows (the collector's [T,E,N,...] flatten); values are per env-row.
 * Both entry points are async on hip_stream, allocate nothing and do not synchronise; rows == 0
 * is a no-op (nothing is written); errors via swarm_ppo_last_error.  Every sum over rows is a
 * two-stage f64 reduction without atomics: per-block partials go to `workspace`
 * (SWARM_PPO_WORKSPACE_BYTES of device memory, 8-B aligned, private to the launch while it runs),
 * and a one-wave finalising launch adds them in index order, in groups of 16 (lane j adds
 * partials 16j .. 16j+15 in order, lane 0 then adds the 64 group sums in order).  The grid depends
 * on `rows` (and N) only, so a launch repeats bit for bit.
 */
#define SWARM_PPO_MAX_ACT 6                 /* action dims A: logits are 2A <= SWARM_POLICY_MAX_OUT wide */
#define SWARM_PPO_MAX_AGENTS 256            /* agents N of an env-row */
#define SWARM_PPO_MAX_BLOCKS 1024           /* workgroups of a launch = partials of a sum */
#define SWARM_PPO_WORKSPACE_BYTES 65536     /* SWARM_PPO_MAX_BLOCKS x 8 doubles */
#define SWARM_PPO_MOMENTS 4                 /* doubles of a swarm_masked_moments result */
#define SWARM_PPO_STATS 7                   /* doubles of swarm_ppo_loss's stats */

/*
 * RLlib's standardized(): over the rows with valid != 0,
 *     out[0] = count,  out[1] = mean,  out[2] = population std (ddof 0),  out[3] = 1 / max(std, 1e-4)
 * as four doubles on the device.  With count 0: mean 0, std 0 and out[3] = 1e4.  x of a row with
 * valid == 0 is never used (it may be NaN).  Arithmetic, all f64:
 *     thread:  p = its first valid x;  n, s = sum(x - p), q = sum((x - p)^2) over its valid rows
 *     block :  nb = sum n,  mb = sum(n p + s) / nb,  M2b = sum(q - 2 (mb - p) s + n (mb - p)^2)
 *              (fixed-shape tree: __shfl_down 32..1 in a wave, then the 4 wave sums in order)
 *     final :  count = sum nb,  mean = sum(nb mb) / count,
 *              std = sqrt(sum(M2b + nb (mb - mean)^2) / count)        (sums in index order, above)
 */
int swarm_masked_moments(const float* x, const uint8_t* valid, long long rows, void* workspace, double* out,
                         void* hip_stream);

typedef struct swarm_ppo_args {
  const float* logits;         /* [R,2A] new policy [mean | log_std]; 8-B aligned */
  const float* behaviour_logits; /* [R,2A] the policy that acted; 8-B aligned */
  const float* actions;        /* [R,A]  */
  const float* logp;           /* [R]    behaviour log-prob of the action */
  const float* advantage;      /* [R]    raw (not standardised) */
  const float* value_target;   /* [R]    */
  const float* value;          /* [R/N]  new value of the env-row */
  const uint8_t* valid;        /* [R]    */
  const double* adv_moments;   /* swarm_masked_moments result used to standardise the advantages */
  const double* valid_moments; /* swarm_masked_moments result over these R rows: [0] is M */
  float* grad_logits;          /* [R,2A] d total / d logits; exactly 0 on invalid rows; 8-B aligned */
  float* grad_value;           /* [R/N]  d total / d value */
  double* stats;               /* [SWARM_PPO_STATS] */
  void* workspace;             /* SWARM_PPO_WORKSPACE_BYTES */
  long long rows;              /* R, a multiple of num_agents */
  int32_t num_agents;          /* N in [1, SWARM_PPO_MAX_AGENTS] */
  int32_t act_dim;             /* A in [1, SWARM_PPO_MAX_ACT] */
  float clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff;
} swarm_ppo_args_t;

/*
 * Per row with valid != 0 (nothing but the valid byte is read from any other row), in f32 without
 * fused multiply-add, k over the A action dims, (mu, s) = logits, (mu0, s0) = behaviour_logits,
 * v = value[row / N], c = clip_param:
 *     adv  = (advantage - (float)adv_moments[1]) * (float)adv_moments[3]
 *     e_k  = exp(-s_k);  z_k = (a_k - mu_k) e_k
 *     lp   = sum_k(-0.5 z_k^2 - s_k) - 0.5 A log(2 pi)             (swarm_gaussian_logp's expression)
 *     r    = exp(lp - logp)
 *     surr = min(adv r, adv clamp(r, 1 - c, 1 + c))
 *     clipped = (adv > 0 and r > 1 + c) or (adv < 0 and r < 1 - c)
 *     d    = v - value_target;  vf = min(d^2, vf_clip_param)
 *     H    = sum_k s_k + 0.5 A log(2 pi e)
 *     u_k  = exp(2 s0_k) + (mu0_k - mu_k)^2
 *     KL   = sum_k(s_k - s0_k + 0.5 u_k e_k^2 - 0.5)                (KL(behaviour || new))
 *     loss = -surr + vf_loss_coeff vf - entropy_coeff H + kl_coeff KL
 * and with M = valid_moments[0], inv = M > 0 ? 1 / M : 0, w = clipped ? 0 : -adv r:
 *     grad_logits[row, k]     = inv (w z_k e_k + kl_coeff (mu_k - mu0_k) e_k^2)
 *     grad_logits[row, A + k] = inv (w (z_k^2 - 1) - entropy_coeff + kl_coeff (1 - u_k e_k^2))
 *     g_row = d^2 < vf_clip_param ? inv vf_loss_coeff 2 d : 0
 *     grad_value[env-row] = sum of g_row over its agents in index order, in groups of 16 (group
 *         sums first, then the group sums in order; invalid agents add 0; no atomics), so an
 *         env-row without a valid agent gets 0
 * grad_logits of a row with valid == 0 is 0.  stats (f64 sums of the f32 row terms, reduced like
 * the moments: per-thread sums in row order, the block tree, the finalising launch):
 *     [0] rows with valid != 0 (counted here)   [1] total = [2] + vf_loss_coeff [3] - entropy_coeff [4] + kl_coeff [5]
 *     [2] inv sum(-surr)   [3] inv sum vf   [4] inv sum H   [5] inv sum KL   [6] inv sum clipped
 * With M == 0 every gradient and stats [1..6] are 0.
 */
int swarm_ppo_loss(const swarm_ppo_args_t* args, void* hip_stream);

const char* swarm_ppo_last_error(void);

/*
 * On-device evaluation metrics: the per-episode summary of
 * scripts/evaluate_protocol.py:237-331 (`_run_single_episode_multi_agent`; formation error
 * :103-116) accumulated on the device from a step's outputs (obs, reward, info_flags, env_done:
 * the env must be stepped with infos).  swarm_eval_update after every swarm_step appends one
 * record per finished episode; the host aggregates the records like `_aggregate` (:334-350).
 * Replaces the host-side per-agent loop over the dict outputs of every evaluation step.
 */
#define SWARM_EVAL_LIVE 1u       /* status: an episode is being accumulated */
#define SWARM_EVAL_COLLIDED 2u   /* status: an observed agent reported a collision */
#define SWARM_EVAL_STEP_FUSED 1  /* swarm_eval_t.flags: per-step accumulation done by the step (out.eval) */
#define SWARM_EVAL_SLOT_COUNTS 2 /* swarm_eval_t.flags: the batch has per-env drone counts (swarm_env_cfg_set_drones):
                                    a slot not stepped on an episode's first step is no drone of that
                                    episode (every drone of a fresh episode is stepped) and is left out of
                                    its path-efficiency mean (traveled[e][slot] = -1 marks it); begin the
                                    tracker at episode starts.  Unfused updates only */
#define SWARM_EVAL_RECORD 9      /* doubles per record: global env index, success, collision_free, time_to_goal
                                    (NaN if never all-reached), formation_error, path_efficiency,
                                    episode_reward, steps, update_index of the closing update */
#define SWARM_EVAL_SEGMENTS 64   /* record counters: an episode of global env g is appended to segment
                                    g % 64 (64 counters on distinct lines instead of one contended
                                    device-scope atomic) */

typedef struct swarm_eval {
  double* ep_reward;      /* [E] sum over steps of the mean reward of the stepped agents */
  int32_t* ep_steps;      /* [E] */
  int32_t* reached_step;  /* [E] first step whose observed agents all reached (-1: none yet) */
  uint8_t* status;        /* [E] SWARM_EVAL_* bits */
  double* fe_sum;         /* [E] sum over steps of the formation error */
  float* start;           /* [E,N,3] positions at the episode start */
  float* goal;            /* [E,N,3] start + obs[6:9] (the reference's goal estimate) */
  float* last;            /* [E,N,3] last observed positions */
  double* traveled;       /* [E,N]   path length */
  double* records;        /* [capacity, SWARM_EVAL_RECORD] finished episodes; segment s owns the row
                             block b = (s - seg_base) mod 64 (< segments): rows [b*C, (b+1)*C),
                             C = capacity / segments */
  uint32_t* count;        /* [SWARM_EVAL_SEGMENTS] records appended per segment (may exceed C: the
                             rest are dropped) */
  int32_t capacity;       /* a multiple of `segments` */
  int32_t update_index;   /* stamped into the records this update closes (the caller counts updates) */
  int32_t flags;          /* SWARM_EVAL_STEP_FUSED: the step launches carry this state in out.eval;
                             SWARM_EVAL_SLOT_COUNTS: per-env drone counts */
  int32_t seg_base;       /* segment of the tracker's first global env (its env_offset mod 64) */
  int32_t segments;       /* record segments that receive episodes: min(envs, 64) (0 = 64): a
                             batch of E < 64 envs holds only E row blocks */
  const float* state_pos;   /* [E,N,3] optional: the env state's positions after the step (bitwise
                               obs[..., 0:3]), read contiguously instead of from the obs rows */
  const float* state_goal;  /* [E,3] optional (with state_pos): the goal; obs[..., 6:9] = goal - pos */
} swarm_eval_t;

/* Start an episode in the masked envs (all if NULL) from the current obs (after a reset). */
int swarm_eval_begin(const swarm_params_t* p, const swarm_eval_t* ev, const swarm_out_t* out,
                     const uint8_t* env_mask, void* hip_stream);

/* Accumulate one step's outputs; close finished episodes (and open the next one of an env the
 * step auto-reset).  Async on hip_stream, no allocation, no sync. */
int swarm_eval_update(const swarm_params_t* p, const swarm_eval_t* ev, const swarm_out_t* out, void* hip_stream);

/* Single-agent protocol (scripts/evaluate_protocol.py:193-234 `_run_single_episode_single_agent`
 * over SingleDroneEnv): a batch of E single-drone envs (num_drones 1, neighbor_k 0, stepped with
 * infos and auto_reset 0, ev->state_pos / state_goal set).  Unlike the swarm protocol the
 * terminal step counts: its collision / reached_goal info and its position (the state, not yet
 * reset).  Per env and step: reward sum, path length, first reached step, any collision; at
 * terminated or truncated one record (formation_error 0) and reset_mask[e] = 1 (0 otherwise):
 * the caller then runs swarm_reset(reset_mask) and swarm_eval_begin(reset_mask) — the next
 * episode — without a host sync.  Replaces the reference's per-episode host loop. */
int swarm_eval_single_update(const swarm_params_t* p, const swarm_eval_t* ev, const swarm_out_t* out,
                             uint8_t* reset_mask, void* hip_stream);

const char* swarm_eval_last_error(void);

/*
 * Write the per-env parameter records cfg[e] (device, [E] swarm_env_cfg_t) of the masked envs
 * (env_mask NULL = all) from `ov` and the uniform fields of `p`.  Async on hip_stream.  Point
 * swarm_state_t.env_cfg (the current episode) or .env_cfg_next (the next episode, e.g. a domain
 * randomisation draw made after the step that reset the env) at the result.
 */
int swarm_env_cfg_set(const swarm_params_t* p, const swarm_env_overrides_t* ov, const uint8_t* env_mask,
                      swarm_env_cfg_t* cfg, void* hip_stream);

/*
 * Per-env drone counts: write cfg[e].num_drones of the masked envs (env_mask NULL = all) from
 * drones[e] (device int32 [E], clamped to [1, swarm_params_t.num_drones]; drones NULL = every
 * slot).  Only that field is written, async on hip_stream; swarm_env_cfg_set writes it as 0
 * (= every slot), so call this after it.
 *
 * Env e with count n then behaves exactly like env env_offset + e of a batch built with
 * num_drones = n: slots 0..n-1 are its drones; slots >= n do not exist — never a neighbour,
 * never in a collision or formation pair, no vote in any env-level reduction, their actions
 * ignored (a drone that ended earlier, by contrast, stays a frozen neighbour).  Buffers keep
 * their N-slot strides.  Every step and reset writes zeros for a slot that does not exist: obs
 * row, reward, terminated, truncated, active, dist_goal, info_flags, state pos / vel and its
 * global_state entries (global_state [6N+3] is the zero-padded embedding of the 6n+3 vector);
 * swarm_observe writes the output zeros and leaves the state alone.  A device reset draws drone t
 * from Philox block t, obstacle m from block n + m, the goal from block n + num_obstacles[e]: the
 * blocks of the n-drone batch.
 *
 * In env_cfg_next the count takes effect at the env's next reset (auto or explicit), which draws,
 * activates and observes with it; it may grow or shrink.  Written to env_cfg (the current
 * episode) it must be followed by a swarm_reset, or by new state, of those envs before their next
 * step: the step does not read the state of slots >= n, and slots < n must hold drones.
 */
int swarm_env_cfg_set_drones(const swarm_params_t* p, const int32_t* drones, const uint8_t* env_mask,
                             swarm_env_cfg_t* cfg, void* hip_stream);

/*
 * Keyed domain randomisation (csrc/swarm_dr.hip): per-episode parameter records as a pure function
 * of (seed, global env index, episode number), drawn and derived on the device by one async launch
 * on hip_stream, one thread per env.  No allocation, no synchronisation, no atomics, no host state;
 * every argument is a device pointer or a constant, so the launch can be captured, and repeating it
 * on the same state rewrites the same bytes.  num_envs == 0 is a no-op.  Errors via
 * swarm_dr_last_error, before any launch: a NULL p / table / episode / cfg, abi_version, num_envs < 0,
 * an enabled parameter with lo <= 0 or lo > hi (or a NaN), dt enabled with
 * dynamics == SWARM_DYN_POINTMASS_PHYSICS (the physics substeps are uniform).
 *
 * Env e of the launch is written iff mask == NULL || (mask[e] & mask_bits) != 0 (an [E] bool mask with
 * mask_bits = 0xFF; swarm_out_t.env_done with mask_bits = SWARM_ENV_RESET).  For a written env, with
 *     g  = (uint32)(p->env_offset + e)
 *     ep = episode[e] + episode_add            (uint32, wrapping; episode[e] read when the kernel runs)
 * parameter i (0 world_size, 1 dt, 2 max_speed, 3 max_accel, 4 obstacle_radius) takes word x = i & 3 of
 * the Philox4x32-10 block with key (seed lo, seed hi) and counter words
 *     (g, 3u << 30 | (i >> 2) << 16, ep, 0)
 * — the perturbation layer's counter layout (above) with stream 3, which that layer does not use, so
 * a seed shared with it never shares a block — and, in double, every operation rounded on its own
 * (no fused multiply-add):
 *     u     = ((x >> 8) + 0.5) * 2^-24                        (exact; 0 < u < 1)
 *     value = base_i * (lo_i + (hi_i - lo_i) * u)             base_i the parameter's swarm_params_t value
 * A parameter with enabled[i] == 0 is base_i itself and draws nothing.
 *
 * From the five values the record takes exactly the fields swarm_env_cfg_set derives from them, bit
 * for bit as swarm_env_cfg_set writes them for the same five doubles: half_w, neg_half_w, width_w,
 * dt, max_speed, max_accel, s_vmax, s_obst, s_phys_obst, max_speed_d, world_size.  max_steps,
 * num_obstacles and num_drones of cfg[e] are NOT written: the randomiser owns only what it
 * randomises, and what a curriculum, swarm_env_cfg_set or swarm_env_cfg_set_drones put there stays.
 * Envs outside the mask keep all 64 bytes.
 *
 * With env_cfg[e] = record(episode[e]) and env_cfg_next[e] = record(episode[e] + 1) (episode_add 0
 * and 1), a reset moves the next record in and increments episode[e]; one launch on env_cfg_next
 * with episode_add = 1 over the envs that reset restores both equalities.
 */
#define SWARM_DR_PARAMS 5

typedef struct swarm_dr_table {     /* index: 0 world_size, 1 dt, 2 max_speed, 3 max_accel, 4 obstacle_radius */
  double lo[SWARM_DR_PARAMS], hi[SWARM_DR_PARAMS];  /* scale range of parameter i */
  uint8_t enabled[SWARM_DR_PARAMS]; /* 0: the parameter keeps its swarm_params_t value */
} swarm_dr_table_t;

int swarm_env_cfg_randomize(const swarm_params_t* p, const swarm_dr_table_t* table, uint64_t seed,
                            const uint32_t* episode /* [E] swarm_state_t.episode */, uint32_t episode_add,
                            const uint8_t* mask /* [E] or NULL */, uint8_t mask_bits,
                            swarm_env_cfg_t* cfg /* [E] */, void* hip_stream);

const char* swarm_dr_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* SWARM_MI355X_H */
