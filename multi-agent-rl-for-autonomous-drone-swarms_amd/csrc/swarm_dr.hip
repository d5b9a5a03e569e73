// swarm_dr.hip — keyed domain randomisation (gfx950): an env's per-episode parameters as a pure
// function of (seed, global env index, episode number), drawn and derived into swarm_env_cfg_t
// records by one launch (the arithmetic is written out in include/swarm_mi355x.h).
//
//   swarm_env_cfg_randomize   one lane per env: the masked envs' records of episode[e] + episode_add;
//                             the fields swarm_env_cfg_set derives from world_size, dt, max_speed,
//                             max_accel and obstacle_radius, bit for bit as it derives them, and
//                             nothing else of the record
//
// Stateless on the host: Philox4x32-10 keyed by the seed on the counter (global env, stream 3 << 30 |
// block << 16, episode, 0), the episode read from the env state on the device.  No LDS, no atomics, no
// host synchronisation; every argument is a device pointer or a constant, so the launch can be
// captured, and a repeated launch rewrites the same bytes.
#include "swarm_nn.h"
#include "swarm_env_cfg.h"

#pragma clang fp contract(off)

namespace {

thread_local UnitError g_err;

constexpr uint32_t STREAM_DR = 3u;  // the stream swarm_perturb.hip leaves unused
constexpr int THREADS = 256;
constexpr int P_WORLD = 0, P_DT = 1, P_VMAX = 2, P_AMAX = 3, P_ORAD = 4;

struct DrArgs {
  const uint32_t* episode;
  const uint8_t* mask;
  swarm_env_cfg_t* cfg;
  swarm_dr_table_t table;
  double base[SWARM_DR_PARAMS];
  double collision_radius, drone_contact_radius;
  long long env_offset;
  uint32_t seed_lo, seed_hi, episode_add, mask_bits;
  int E;
};

// base * (lo + (hi - lo) * u), u = ((x >> 8) + 0.5) 2^-24: double, each operation rounded on its own
__device__ __forceinline__ double scaled(double base, double lo, double hi, uint32_t x) {
  const double u = ((double)(x >> 8) + 0.5) * 0x1p-24;
  const double span = hi - lo;
  const double scale = lo + span * u;
  return base * scale;
}

__global__ void __launch_bounds__(THREADS) randomize_kernel(const DrArgs A) {
  const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
  if (e >= (uint32_t)A.E) return;
  if (A.mask != nullptr && (A.mask[e] & A.mask_bits) == 0u) return;
  const uint32_t g = (uint32_t)(A.env_offset + (long long)e);
  const uint32_t ep = A.episode[e] + A.episode_add;
  // parameters 0..3 are the words of block 0, parameter 4 is word 0 of block 1 (constant indices
  // throughout: a run-time index into the by-value table would move it to scratch)
  double v[SWARM_DR_PARAMS];
#pragma unroll
  for (int i = 0; i < SWARM_DR_PARAMS; ++i) v[i] = A.base[i];
  if (A.table.enabled[0] | A.table.enabled[1] | A.table.enabled[2] | A.table.enabled[3]) {
    uint32_t c[4] = {g, STREAM_DR << 30, ep, 0u};
    philox(c, A.seed_lo, A.seed_hi);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (A.table.enabled[i]) v[i] = scaled(A.base[i], A.table.lo[i], A.table.hi[i], c[i]);
  }
  if (A.table.enabled[4]) {
    uint32_t c[4] = {g, (STREAM_DR << 30) | (1u << 16), ep, 0u};
    philox(c, A.seed_lo, A.seed_hi);
    v[4] = scaled(A.base[4], A.table.lo[4], A.table.hi[4], c[0]);
  }
  // env_cfg_set_kernel's derivations of the same five doubles (swarm_kernel.hip), field by field;
  // max_steps, num_obstacles and num_drones are not this unit's: they are left as they are
  const double ws = v[P_WORLD], vmax = v[P_VMAX], orad = v[P_ORAD];
  swarm_env_cfg_t* out = A.cfg + e;
  const float max_speed = (float)vmax;
  out->half_w = (float)(ws / 2.0);
  out->neg_half_w = (float)(-ws / 2.0);
  out->width_w = (float)ws;
  out->dt = (float)v[P_DT];
  out->max_speed = max_speed;
  out->max_accel = (float)v[P_AMAX];
  out->s_vmax = s_threshold_dev(max_speed);
  out->s_obst = s_threshold_dev((float)(A.collision_radius + orad));
  out->s_phys_obst = s_threshold_dev((float)(orad + A.drone_contact_radius));
  out->max_speed_d = vmax;
  out->world_size = ws;
}

}  // namespace

extern "C" {

const char* swarm_dr_last_error(void) { return g_err.msg; }

int swarm_env_cfg_randomize(const swarm_params_t* p, const swarm_dr_table_t* table, uint64_t seed, const uint32_t* episode,
                            uint32_t episode_add, const uint8_t* mask, uint8_t mask_bits, swarm_env_cfg_t* cfg,
                            void* hip_stream) {
  if (!p) return g_err.fail(SWARM_ENULL, "params is NULL");
  if (!table) return g_err.fail(SWARM_ENULL, "table is NULL");
  if (p->abi_version != SWARM_ABI_VERSION) return g_err.fail(SWARM_EINVAL, "abi_version mismatch");
  if (p->num_envs < 0) return g_err.fail(SWARM_EINVAL, "num_envs < 0");
  if (p->dynamics != SWARM_DYN_KINEMATIC && p->dynamics != SWARM_DYN_POINTMASS_PHYSICS)
    return g_err.fail(SWARM_EINVAL, "unknown dynamics");
  for (int i = 0; i < SWARM_DR_PARAMS; ++i) {
    if (!table->enabled[i]) continue;
    if (!(table->lo[i] > 0.0)) return g_err.fail(SWARM_EINVAL, "a scale range needs lo > 0");
    if (!(table->lo[i] <= table->hi[i]) || __builtin_isinf(table->hi[i]))
      return g_err.fail(SWARM_EINVAL, "a scale range needs lo <= hi (finite)");
  }
  if (table->enabled[P_DT] && p->dynamics == SWARM_DYN_POINTMASS_PHYSICS)
    return g_err.fail(SWARM_EINVAL, "dt applies to the kinematic integrator only (physics substeps are uniform)");
  if (p->num_envs == 0) return SWARM_OK;
  if (!episode) return g_err.fail(SWARM_ENULL, "episode is NULL");
  if (!cfg) return g_err.fail(SWARM_ENULL, "env_cfg is NULL");
  DrArgs k;
  k.episode = episode;
  k.mask = mask;
  k.cfg = cfg;
  k.table = *table;
  k.base[P_WORLD] = p->world_size;
  k.base[P_DT] = p->dt;
  k.base[P_VMAX] = p->max_speed;
  k.base[P_AMAX] = p->max_accel;
  k.base[P_ORAD] = p->obstacle_radius;
  k.collision_radius = p->collision_radius;
  k.drone_contact_radius = p->drone_contact_radius;
  k.env_offset = p->env_offset;
  k.seed_lo = (uint32_t)seed;
  k.seed_hi = (uint32_t)(seed >> 32);
  k.episode_add = episode_add;
  k.mask_bits = mask_bits;
  k.E = p->num_envs;
  hipLaunchKernelGGL(randomize_kernel, dim3((p->num_envs + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)hip_stream, k);
  return g_err.launch_status();
}

}  // extern "C"
