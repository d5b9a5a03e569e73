"""ctypes binding of the C-ABI in include/swarm_mi355x.h (libswarm_mi355x.so, built for gfx950).

The library is the product's compute path: there is no CPU fallback.  If it is missing the
import of the engine fails loudly (NativeLibraryError) — build it with
`python -c "import __graft_entry__ as g; g.build()"` from the repository root.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

LIB_NAME = "libswarm_mi355x.so"
LIB_DIR = Path(__file__).resolve().parent / "_lib"
LIB_PATH = LIB_DIR / LIB_NAME

ABI_VERSION = 5
WORK_WORDS = 256  # SWARM_WORK_WORDS: u32 env-queue heads of the persistent swarm_step64

PATH_AUTO = 0
PATH_GENERIC = 1
KERNEL_GENERIC = 0
KERNEL_STEP64 = 1
KERNEL_STEP64_PERSISTENT = 2
KERNEL_STEP16Q = 3
KERNEL_STEP256 = 4

SWARM_OK = 0
SWARM_EINVAL = -1
SWARM_ENULL = -2
SWARM_ELIMIT = -3
SWARM_EHIP = -4

DYN_KINEMATIC = 0
DYN_POINTMASS_PHYSICS = 1
REW_SWARM = 0
REW_PHYSICS = 1

ENV_TERMINATED = 1
ENV_TRUNCATED = 2
ENV_RESET = 4

AGENT_STEPPED = 1
AGENT_REACHED = 2
AGENT_COLLISION = 4
AGENT_HAS_OBS = 8

POLICY_HIDDEN = 256
POLICY_MAX_IN = 47
POLICY_MAX_OUT = 12
POLICY_BF16 = 0
POLICY_F32 = 1
POLICY_F32X3 = 2
POLICY_ACT_MEAN = 0
POLICY_ACT_SAMPLE = 1
ATTN_EMBED = 32
ATTN_MAX_K = 16
ATTN_MAX_MS = 5
CRITIC_MAX_IN = 1539
EVAL_LIVE = 1
EVAL_COLLIDED = 2
EVAL_STEP_FUSED = 1
EVAL_SLOT_COUNTS = 2
EVAL_RECORD = 9
EVAL_SEGMENTS = 64
PPO_MAX_ACT = 6
PPO_MAX_AGENTS = 256
PPO_WORKSPACE_BYTES = 65536
PPO_MOMENTS = 4
PPO_STATS = 7
PERTURB_MAX_DELAY = 7
PERTURB_MAX_AGENTS = 256
PERTURB_MAX_K = 16
PERTURB_MAX_MS = 5
ROLLOUT_MAX_ACT = 6
ROLLOUT_MAX_SEGMENTS = 8
TRAIN_SLAB = 1024        # SWARM_TRAIN_SLAB: rows per weight-gradient slab
TRAIN_MAX_BLOCKS = 256   # SWARM_TRAIN_MAX_BLOCKS: workgroups of the backward's tile launches
TRAIN_MAX_ROWS = 1 << 28

# every symbol include/swarm_mi355x.h declares
EXPORTED_SYMBOLS = (
    "swarm_abi_version", "swarm_last_error", "swarm_params_default", "swarm_obs_dim",
    "swarm_query_launch", "swarm_step", "swarm_step_groups", "swarm_reset", "swarm_observe",
    "swarm_policy_packed_bytes", "swarm_policy_pack", "swarm_policy_forward", "swarm_policy_last_error",
    "swarm_attn_policy_packed_bytes", "swarm_attn_policy_pack", "swarm_attn_policy_forward",
    "swarm_attn_policy_last_error",
    "swarm_eval_begin", "swarm_eval_update", "swarm_eval_single_update", "swarm_eval_last_error",
    "swarm_env_cfg_set", "swarm_env_cfg_set_drones",
    "swarm_value_packed_bytes", "swarm_value_pack", "swarm_value_forward", "swarm_gae_agent", "swarm_value_last_error",
    "swarm_actuate", "swarm_sense", "swarm_perturb_last_error",
    "swarm_rollout_sample", "swarm_rollout_record", "swarm_rollout_last_error",
    "swarm_env_cfg_randomize", "swarm_dr_last_error",
    "swarm_policy_train_workspace_bytes", "swarm_policy_pack_device", "swarm_policy_backward",
    "swarm_policy_train_last_error",
    "swarm_critic_packed_bytes", "swarm_critic_pack", "swarm_critic_forward", "swarm_critic_last_error",
    "swarm_gaussian_logp", "swarm_gae",
    "swarm_masked_moments", "swarm_ppo_loss", "swarm_ppo_last_error",
)
# the rollout half (csrc/swarm_critic.hip) and the PPO loss head (csrc/swarm_ppo.hip); a diagnostic
# build given by path may leave either unit out
ROLLOUT_SYMBOLS = EXPORTED_SYMBOLS[-9:-3]
PPO_SYMBOLS = EXPORTED_SYMBOLS[-3:]
ATTN_SYMBOLS = tuple(s for s in EXPORTED_SYMBOLS if s.startswith("swarm_attn_"))  # csrc/swarm_attn.hip
VALUE_SYMBOLS = tuple(s for s in EXPORTED_SYMBOLS if s.startswith("swarm_value_")) + ("swarm_gae_agent",)  # csrc/swarm_value.hip
PERTURB_SYMBOLS = ("swarm_actuate", "swarm_sense", "swarm_perturb_last_error")  # csrc/swarm_perturb.hip
GRAPH_SYMBOLS = ("swarm_rollout_sample", "swarm_rollout_record", "swarm_rollout_last_error")  # csrc/swarm_rollout.hip
DR_SYMBOLS = ("swarm_env_cfg_randomize", "swarm_dr_last_error")  # csrc/swarm_dr.hip
TRAIN_SYMBOLS = ("swarm_policy_train_workspace_bytes", "swarm_policy_pack_device", "swarm_policy_backward",
                 "swarm_policy_train_last_error")  # csrc/swarm_train.hip
ENV_CFG_BYTES = 64  # sizeof(swarm_env_cfg_t)
DR_PARAMS = ("world_size", "dt", "max_speed", "max_accel", "obstacle_radius")  # swarm_dr_table_t's index order


class NativeLibraryError(RuntimeError):
    pass


class SwarmParams(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("num_envs", ctypes.c_int32),
        ("num_drones", ctypes.c_int32),
        ("num_obstacles", ctypes.c_int32),
        ("sensed_obstacles", ctypes.c_int32),
        ("neighbor_k", ctypes.c_int32),
        ("max_steps", ctypes.c_int32),
        ("dynamics", ctypes.c_int32),
        ("reward_mode", ctypes.c_int32),
        ("auto_reset", ctypes.c_int32),
        ("physics_substeps", ctypes.c_int32),
        ("damping_law", ctypes.c_int32),
        ("env_offset", ctypes.c_int64),
        ("seed", ctypes.c_uint64),
        ("world_size", ctypes.c_double),
        ("dt", ctypes.c_double),
        ("max_speed", ctypes.c_double),
        ("max_accel", ctypes.c_double),
        ("collision_radius", ctypes.c_double),
        ("goal_radius", ctypes.c_double),
        ("obstacle_radius", ctypes.c_double),
        ("desired_spacing", ctypes.c_double),
        ("reward_progress_scale", ctypes.c_double),
        ("reward_goal", ctypes.c_double),
        ("reward_collision", ctypes.c_double),
        ("reward_formation_scale", ctypes.c_double),
        ("gravity", ctypes.c_double),
        ("gravity_comp", ctypes.c_double),
        ("substep_dt", ctypes.c_double),
        ("drone_contact_radius", ctypes.c_double),
        ("ground_contact_height", ctypes.c_double),
        ("kernel_path", ctypes.c_int32),
        ("waves_per_simd", ctypes.c_int32),
    ]


class SwarmState(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("pos", "vel", "goal", "obstacles", "active", "step_count", "episode", "damping",
                 "work", "env_cfg", "env_cfg_next")]


class SwarmEnvCfg(ctypes.Structure):
    """swarm_env_cfg_t: one env's derived parameters (64 B)."""
    _fields_ = [(name, ctypes.c_float) for name in
                ("half_w", "neg_half_w", "width_w", "dt", "max_speed", "max_accel", "s_vmax", "s_obst",
                 "s_phys_obst")] + [("max_steps", ctypes.c_int32), ("num_obstacles", ctypes.c_int32),
                                    ("num_drones", ctypes.c_int32), ("max_speed_d", ctypes.c_double),
                                    ("world_size", ctypes.c_double)]


ENV_OVERRIDE_FIELDS = ("world_size", "dt", "max_speed", "max_accel", "obstacle_radius", "max_steps",
                       "num_obstacles")


class SwarmEnvOverrides(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ENV_OVERRIDE_FIELDS]


class SwarmOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "reward", "terminated", "truncated", "env_done", "dist_goal",
                 "info_flags", "global_state", "eval")]  # eval: host pointer to a SwarmEval (fused)


class SwarmPolicy(ctypes.Structure):
    _fields_ = [("in_dim", ctypes.c_int32), ("out_dim", ctypes.c_int32), ("precision", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("weights", ctypes.c_void_p)]


class SwarmPolicyBackwardArgs(ctypes.Structure):
    """swarm_policy_backward_args_t."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("weights", "obs", "grad_logits", "workspace", "dw1", "db1", "dw2", "db2", "dw3", "db3",
                 "h1", "h2", "dz2", "dz1")] + [("rows", ctypes.c_longlong), ("in_dim", ctypes.c_int32),
                                               ("out_dim", ctypes.c_int32)]


class SwarmAttnPolicy(ctypes.Structure):
    """swarm_attn_policy_t."""
    _fields_ = [("neighbor_k", ctypes.c_int32), ("sensed_obstacles", ctypes.c_int32), ("out_dim", ctypes.c_int32),
                ("precision", ctypes.c_int32), ("weights", ctypes.c_void_p)]


ATTN_WEIGHT_FIELDS = ("neighbor_w", "neighbor_b", "own_w", "own_b", "in_proj_w", "in_proj_b", "out_proj_w",
                      "out_proj_b", "w1", "b1", "w2", "b2", "w3", "b3")


class SwarmAttnWeights(ctypes.Structure):
    """swarm_attn_weights_t: host pointers to the row-major f32 parameters."""
    _fields_ = [(name, ctypes.POINTER(ctypes.c_float)) for name in ATTN_WEIGHT_FIELDS]


class SwarmCritic(ctypes.Structure):
    _fields_ = [("in_dim", ctypes.c_int32), ("precision", ctypes.c_int32), ("weights", ctypes.c_void_p)]


class SwarmValue(ctypes.Structure):
    """swarm_value_t."""
    _fields_ = [("in_dim", ctypes.c_int32), ("precision", ctypes.c_int32), ("weights", ctypes.c_void_p)]


class SwarmDelayTable(ctypes.Structure):
    """swarm_delay_table_t."""
    _fields_ = [("count", ctypes.c_int32), ("values", ctypes.c_int32 * (PERTURB_MAX_DELAY + 1)),
                ("cum", ctypes.c_float * (PERTURB_MAX_DELAY + 1))]


class SwarmActuateArgs(ctypes.Structure):
    """swarm_actuate_args_t."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("actions", "ring", "delay_override", "thrust_noise_std", "step_count", "episode", "eff",
                 "delay_out")] + [("delays", SwarmDelayTable)] + [
        (name, ctypes.c_int32) for name in ("ring_slots", "num_envs", "num_drones", "reserved")] + [
        ("seed", ctypes.c_uint64), ("env_offset", ctypes.c_int64)]


class SwarmSenseArgs(ctypes.Structure):
    """swarm_sense_args_t."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "active", "position_noise_std", "velocity_noise_std", "obstacle_noise_std", "step_count",
                 "episode", "out")] + [("seed", ctypes.c_uint64), ("env_offset", ctypes.c_int64)] + [
        (name, ctypes.c_int32) for name in ("num_envs", "num_drones", "neighbor_k", "sensed_obstacles")]


class SwarmDrTable(ctypes.Structure):
    """swarm_dr_table_t: scale range and switch of each DR_PARAMS entry."""
    _fields_ = [("lo", ctypes.c_double * len(DR_PARAMS)), ("hi", ctypes.c_double * len(DR_PARAMS)),
                ("enabled", ctypes.c_uint8 * len(DR_PARAMS))]


class SwarmRolloutSegment(ctypes.Structure):
    """swarm_rollout_segment_t."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("bytes", ctypes.c_uint64)]


class SwarmRolloutRecord(ctypes.Structure):
    """swarm_rollout_record_t."""
    _fields_ = [("count", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("segments", SwarmRolloutSegment * ROLLOUT_MAX_SEGMENTS)]


class SwarmPpoArgs(ctypes.Structure):
    """swarm_ppo_args_t."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("logits", "behaviour_logits", "actions", "logp", "advantage", "value_target", "value", "valid",
                 "adv_moments", "valid_moments", "grad_logits", "grad_value", "stats", "workspace")] + [
        ("rows", ctypes.c_longlong), ("num_agents", ctypes.c_int32), ("act_dim", ctypes.c_int32)] + [
        (name, ctypes.c_float) for name in ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff")]


class SwarmEval(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("ep_reward", "ep_steps", "reached_step", "status", "fe_sum", "start", "goal", "last",
                 "traveled", "records", "count")] + [("capacity", ctypes.c_int32), ("update_index", ctypes.c_int32),
                                                     ("flags", ctypes.c_int32), ("seg_base", ctypes.c_int32),
                                                     ("segments", ctypes.c_int32),
                                                     ("state_pos", ctypes.c_void_p), ("state_goal", ctypes.c_void_p)]


class SwarmLaunchInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in
                ("threads_per_block", "envs_per_block", "lanes_per_env", "blocks", "lds_bytes",
                 "neighbor_slots", "obstacle_slots", "obs_dim", "staged_obs", "kernel_id")]


_LIB = None


def load_library(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """Load libswarm_mi355x.so (once) and declare its signatures."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    if path is None and os.environ.get("SWARM_MI355X_LIB"):
        path = os.environ["SWARM_MI355X_LIB"]  # diagnostic builds (tools/ablate.sh)
    p = Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise NativeLibraryError(
            f"{p} is missing: the MI355X swarm engine has no CPU fallback. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` in the repository root.")
    lib = ctypes.CDLL(str(p))
    P, S, O = ctypes.POINTER(SwarmParams), ctypes.POINTER(SwarmState), ctypes.POINTER(SwarmOut)
    vp = ctypes.c_void_p
    lib.swarm_abi_version.restype = ctypes.c_int
    lib.swarm_abi_version.argtypes = []
    lib.swarm_last_error.restype = ctypes.c_char_p
    lib.swarm_last_error.argtypes = []
    lib.swarm_params_default.restype = None
    lib.swarm_params_default.argtypes = [P]
    lib.swarm_obs_dim.restype = ctypes.c_int
    lib.swarm_obs_dim.argtypes = [P]
    lib.swarm_query_launch.restype = ctypes.c_int
    lib.swarm_query_launch.argtypes = [P, ctypes.POINTER(SwarmLaunchInfo)]
    lib.swarm_step.restype = ctypes.c_int
    lib.swarm_step.argtypes = [P, S, vp, vp, O, vp]
    lib.swarm_step_groups.restype = ctypes.c_int
    lib.swarm_step_groups.argtypes = [P, S, vp, vp, O, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(ctypes.c_void_p)]
    lib.swarm_reset.restype = ctypes.c_int
    lib.swarm_reset.argtypes = [P, S, vp, O, vp]
    lib.swarm_observe.restype = ctypes.c_int
    lib.swarm_observe.argtypes = [P, S, vp, O, vp]
    fp = ctypes.POINTER(ctypes.c_float)
    lib.swarm_policy_packed_bytes.restype = ctypes.c_longlong
    lib.swarm_policy_packed_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.swarm_policy_pack.restype = ctypes.c_int
    lib.swarm_policy_pack.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, fp, vp]
    lib.swarm_policy_forward.restype = ctypes.c_int
    lib.swarm_policy_forward.argtypes = [ctypes.POINTER(SwarmPolicy), vp, ctypes.c_longlong, vp, vp, ctypes.c_int,
                                         ctypes.c_ulonglong, ctypes.c_ulonglong, vp]
    lib.swarm_policy_last_error.restype = ctypes.c_char_p
    lib.swarm_policy_last_error.argtypes = []
    if path is None or all(hasattr(lib, name) for name in ATTN_SYMBOLS):
        lib.swarm_attn_policy_packed_bytes.restype = ctypes.c_longlong
        lib.swarm_attn_policy_packed_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.swarm_attn_policy_pack.restype = ctypes.c_int
        lib.swarm_attn_policy_pack.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(SwarmAttnWeights), vp]
        lib.swarm_attn_policy_forward.restype = ctypes.c_int
        lib.swarm_attn_policy_forward.argtypes = [ctypes.POINTER(SwarmAttnPolicy), vp, ctypes.c_longlong, vp, vp,
                                                  ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, vp]
        lib.swarm_attn_policy_last_error.restype = ctypes.c_char_p
        lib.swarm_attn_policy_last_error.argtypes = []
    ev = ctypes.POINTER(SwarmEval)
    lib.swarm_eval_begin.restype = ctypes.c_int
    lib.swarm_eval_begin.argtypes = [P, ev, O, vp, vp]
    lib.swarm_eval_update.restype = ctypes.c_int
    lib.swarm_eval_update.argtypes = [P, ev, O, vp]
    lib.swarm_eval_single_update.restype = ctypes.c_int
    lib.swarm_eval_single_update.argtypes = [P, ev, O, vp, vp]
    lib.swarm_eval_last_error.restype = ctypes.c_char_p
    lib.swarm_eval_last_error.argtypes = []
    lib.swarm_env_cfg_set.restype = ctypes.c_int
    lib.swarm_env_cfg_set.argtypes = [P, ctypes.POINTER(SwarmEnvOverrides), vp, vp, vp]
    if path is None or hasattr(lib, "swarm_env_cfg_set_drones"):  # (a library given by path may predate it)
        lib.swarm_env_cfg_set_drones.restype = ctypes.c_int
        lib.swarm_env_cfg_set_drones.argtypes = [P, vp, vp, vp, vp]
    if path is None or all(hasattr(lib, name) for name in ROLLOUT_SYMBOLS):
        lib.swarm_critic_packed_bytes.restype = ctypes.c_longlong
        lib.swarm_critic_packed_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.swarm_critic_pack.restype = ctypes.c_int
        lib.swarm_critic_pack.argtypes = [ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, fp, vp]
        lib.swarm_critic_forward.restype = ctypes.c_int
        lib.swarm_critic_forward.argtypes = [ctypes.POINTER(SwarmCritic), vp, ctypes.c_longlong, vp, vp]
        lib.swarm_critic_last_error.restype = ctypes.c_char_p
        lib.swarm_critic_last_error.argtypes = []
        lib.swarm_gaussian_logp.restype = ctypes.c_int
        lib.swarm_gaussian_logp.argtypes = [vp, vp, ctypes.c_longlong, ctypes.c_int, vp, vp]
        lib.swarm_gae.restype = ctypes.c_int
        lib.swarm_gae.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_float, ctypes.c_float, vp, vp, vp]
    if path is None or all(hasattr(lib, name) for name in VALUE_SYMBOLS):
        lib.swarm_value_packed_bytes.restype = ctypes.c_longlong
        lib.swarm_value_packed_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.swarm_value_pack.restype = ctypes.c_int
        lib.swarm_value_pack.argtypes = [ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, fp, vp]
        lib.swarm_value_forward.restype = ctypes.c_int
        lib.swarm_value_forward.argtypes = [ctypes.POINTER(SwarmValue), vp, ctypes.c_longlong, vp, vp]
        lib.swarm_gae_agent.restype = ctypes.c_int
        lib.swarm_gae_agent.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_float, vp, vp, vp]
        lib.swarm_value_last_error.restype = ctypes.c_char_p
        lib.swarm_value_last_error.argtypes = []
    if path is None or all(hasattr(lib, name) for name in PERTURB_SYMBOLS):
        lib.swarm_actuate.restype = ctypes.c_int
        lib.swarm_actuate.argtypes = [ctypes.POINTER(SwarmActuateArgs), vp]
        lib.swarm_sense.restype = ctypes.c_int
        lib.swarm_sense.argtypes = [ctypes.POINTER(SwarmSenseArgs), vp]
        lib.swarm_perturb_last_error.restype = ctypes.c_char_p
        lib.swarm_perturb_last_error.argtypes = []
    if path is None or all(hasattr(lib, name) for name in GRAPH_SYMBOLS):
        lib.swarm_rollout_sample.restype = ctypes.c_int
        lib.swarm_rollout_sample.argtypes = [vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_ulonglong, vp,
                                             ctypes.c_ulonglong, vp, vp]
        lib.swarm_rollout_record.restype = ctypes.c_int
        lib.swarm_rollout_record.argtypes = [ctypes.POINTER(SwarmRolloutRecord), vp]
        lib.swarm_rollout_last_error.restype = ctypes.c_char_p
        lib.swarm_rollout_last_error.argtypes = []
    if path is None or all(hasattr(lib, name) for name in DR_SYMBOLS):
        lib.swarm_env_cfg_randomize.restype = ctypes.c_int
        lib.swarm_env_cfg_randomize.argtypes = [P, ctypes.POINTER(SwarmDrTable), ctypes.c_uint64, vp, ctypes.c_uint32,
                                                vp, ctypes.c_uint8, vp, vp]
        lib.swarm_dr_last_error.restype = ctypes.c_char_p
        lib.swarm_dr_last_error.argtypes = []
    if path is None or all(hasattr(lib, name) for name in TRAIN_SYMBOLS):
        lib.swarm_policy_train_workspace_bytes.restype = ctypes.c_longlong
        lib.swarm_policy_train_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
        lib.swarm_policy_pack_device.restype = ctypes.c_int
        lib.swarm_policy_pack_device.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.swarm_policy_backward.restype = ctypes.c_int
        lib.swarm_policy_backward.argtypes = [ctypes.POINTER(SwarmPolicyBackwardArgs), vp]
        lib.swarm_policy_train_last_error.restype = ctypes.c_char_p
        lib.swarm_policy_train_last_error.argtypes = []
    if path is None or all(hasattr(lib, name) for name in PPO_SYMBOLS):
        lib.swarm_masked_moments.restype = ctypes.c_int
        lib.swarm_masked_moments.argtypes = [vp, vp, ctypes.c_longlong, vp, vp, vp]
        lib.swarm_ppo_loss.restype = ctypes.c_int
        lib.swarm_ppo_loss.argtypes = [ctypes.POINTER(SwarmPpoArgs), vp]
        lib.swarm_ppo_last_error.restype = ctypes.c_char_p
        lib.swarm_ppo_last_error.argtypes = []
    got = lib.swarm_abi_version()
    if got != ABI_VERSION:
        raise NativeLibraryError(f"{p}: ABI version {got}, expected {ABI_VERSION}")
    if path is None:
        _LIB = lib
    return lib


# the component whose last-error string explains a return code (`check`'s `which`)
LAST_ERROR = {"policy": "swarm_policy_last_error", "attn": "swarm_attn_policy_last_error",
              "eval": "swarm_eval_last_error", "critic": "swarm_critic_last_error", "ppo": "swarm_ppo_last_error",
              "value": "swarm_value_last_error", "perturb": "swarm_perturb_last_error", "rollout": "swarm_rollout_last_error",
              "dr": "swarm_dr_last_error", "train": "swarm_policy_train_last_error"}


def check(rc: int, lib: ctypes.CDLL | None = None, which: str | None = None) -> None:
    """Raise on a negative return code (bad arguments -> ValueError, HIP errors -> RuntimeError).
    `which` names the component whose last-error string explains it (a key of LAST_ERROR; the env's
    swarm_last_error otherwise)."""
    if rc == SWARM_OK:
        return
    lib = lib or load_library()
    err = getattr(lib, LAST_ERROR.get(which, "swarm_last_error"))  # looked up now: a library given by path may lack a unit
    msg = (err() or b"").decode(errors="replace")
    if rc in (SWARM_EINVAL, SWARM_ENULL, SWARM_ELIMIT):
        raise ValueError(f"swarm_mi355x error {rc}: {msg}")
    raise RuntimeError(f"swarm_mi355x error {rc}: {msg}")
