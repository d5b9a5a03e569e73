// swarm_perturb.hip — the actuation and sensing half of the domain-randomisation recipe (gfx950):
// a per-episode control delay with a delay line, per-step thrust noise, and per-step sensing noise
// on the observation, as an opt-in layer before and after the env step (the
// arithmetic is written out in include/swarm_mi355x.h).
//
//   swarm_actuate   one lane per agent: clip the command, put it in the delay line, take the command
//                   of d steps ago, add thrust noise -> eff [E,N,3] (what the env step is given)
//   swarm_sense     one lane per 4-float slot of an observation row (the own block, 9 floats, is one
//                   lane): out [E,N,D] = obs with noise; obs is not written
//
// Both are stateless on the host: all noise is Philox4x32-10 keyed by the perturbation's seed on the
// counter (global env, agent | block << 16 | stream << 30, episode[e], step_count[e]), the last two
// read from the env state on the device.  No LDS, no atomics, no host synchronisation; every
// argument is a device pointer or a constant, so both launches can be captured.
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

thread_local UnitError g_err;

constexpr uint32_t STREAM_ACT = 0u, STREAM_SENSE = 1u, STREAM_DELAY = 2u;
constexpr int THREADS = 256;

// The four Box-Muller normals of one Philox block (SWARM_NORMALS' expressions: words (x0, x1) give
// z0, z1 and (x2, x3) give z2, z3).  NZ: how many the caller uses; the others are not computed.
template <int NZ>
__device__ __forceinline__ void block_normals(uint32_t g, uint32_t n, uint32_t block, uint32_t stream, uint32_t episode,
                                              uint32_t step, uint32_t k0, uint32_t k1, float (&z)[4]) {
  uint32_t c[4] = {g, n | (block << 16) | (stream << 30), episode, step};
  philox(c, k0, k1);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (2 * p >= NZ) break;
    const float u1 = ((float)(c[2 * p] >> 8) + 0.5f) * 0x1p-24f;
    const float u2 = (float)(c[2 * p + 1] >> 8) * 0x1p-24f;
    const float rr = sqrtf(-2.f * logf(u1));
    z[2 * p] = rr * cosf(6.28318530717958647692f * u2);
    if (2 * p + 1 < NZ) z[2 * p + 1] = rr * sinf(6.28318530717958647692f * u2);
  }
}

// ---------------------------------------------------------------- control delay
// the env's delay this episode: the override if >= 0, else the table entry of the first cum > u
__device__ __forceinline__ int episode_delay(const swarm_delay_table_t& T, const int32_t* override, int e, uint32_t g,
                                             uint32_t episode, uint32_t k0, uint32_t k1, int max_delay) {
  int d = override ? override[e] : -1;
  if (d < 0) {
    d = T.values[0];
    if (T.count > 1) {
      uint32_t c[4] = {g, STREAM_DELAY << 30, episode, 0u};
      philox(c, k0, k1);
      const float u = (float)(c[0] >> 8) * 0x1p-24f;
      // the first i with u < cum[i] (one exists: u < 1 = cum[count - 1]), walked downwards with
      // constant indices — a run-time index into the by-value table would move it to scratch — so
      // the lowest match is the one that stays
#pragma unroll
      for (int i = SWARM_PERTURB_MAX_DELAY; i >= 0; --i)
        if (i < T.count && u < T.cum[i]) d = T.values[i];
    }
  }
  return d > max_delay ? max_delay : d;
}

struct ActArgs {
  const float* actions;
  float* ring;
  const int32_t* delay_override;
  const float* thrust_noise_std;
  const int32_t* step_count;
  const uint32_t* episode;
  float* eff;
  int32_t* delay_out;
  swarm_delay_table_t delays;
  uint32_t seed_lo, seed_hi;
  long long env_offset;
  int E, N, R;
};

__global__ void __launch_bounds__(THREADS) actuate_kernel(const ActArgs A) {
  const uint32_t i = blockIdx.x * THREADS + threadIdx.x;  // (e, n); E * N < 2^31 is checked
  if (i >= (uint32_t)A.E * (uint32_t)A.N) return;
  const uint32_t e = i / (uint32_t)A.N, n = i - e * (uint32_t)A.N;
  const uint32_t g = (uint32_t)(A.env_offset + (long long)e);
  const uint32_t ep = A.episode[e];
  const int s = A.step_count[e];
  const int d = episode_delay(A.delays, A.delay_override, (int)e, g, ep, A.seed_lo, A.seed_hi, A.R - 1);
  if (n == 0 && A.delay_out) A.delay_out[e] = d;
  const size_t slice = (size_t)A.E * A.N * 3, at = (size_t)i * 3;
  const uint32_t R = (uint32_t)A.R, su = s < 0 ? 0u : (uint32_t)s;
  float u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = fminf(fmaxf(A.actions[at + k], -1.f), 1.f);
  float* w = A.ring + (size_t)(su % R) * slice + at;
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = u[k];
  if (d > 0) {
    if ((uint32_t)d <= su) {
      const float* r = A.ring + (size_t)((su - (uint32_t)d) % R) * slice + at;  // another slot than w: d < R
#pragma unroll
      for (int k = 0; k < 3; ++k) u[k] = r[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) u[k] = 0.f;  // nothing commanded yet in this episode
    }
  }
  const float sig = A.thrust_noise_std ? A.thrust_noise_std[e] : 0.f;
  if (sig != 0.f) {
    float z[4];
    block_normals<3>(g, n, 0u, STREAM_ACT, ep, (uint32_t)s, A.seed_lo, A.seed_hi, z);
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = u[k] + sig * z[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) A.eff[at + k] = u[k];
}

// delay_out only (swarm_actuate without actions): one lane per env
__global__ void __launch_bounds__(THREADS) delay_kernel(const ActArgs A) {
  const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
  if (e >= (uint32_t)A.E) return;
  A.delay_out[e] = episode_delay(A.delays, A.delay_override, (int)e, (uint32_t)(A.env_offset + (long long)e), A.episode[e],
                                 A.seed_lo, A.seed_hi, A.R - 1);
}

// ---------------------------------------------------------------- sensing noise
struct SenseArgs {
  const float* obs;
  const uint8_t* active;
  const float* sig_p;
  const float* sig_v;
  const float* sig_o;
  const int32_t* step_count;
  const uint32_t* episode;
  float* out;
  uint32_t seed_lo, seed_hi;
  long long env_offset;
  uint32_t total;  // E * N * S lanes
  int N, K, Ms;
};

// Lane i is slot i % S of row i / S, S = 1 + K + Ms: slot 0 is the own block (floats 0..8), slot j
// the 4 floats at 9 + 4 (j - 1).  Consecutive lanes hold consecutive slots of consecutive rows, so a
// wave's loads and its stores cover one contiguous span of 64 / S rows (rows are 4 D bytes and not
// 16-B aligned: whole rows per lane would spread a wave over 64 rows).  Every lane draws one Philox
// block; the own lane draws its second one (velocity) in a pass of its own.
__global__ void __launch_bounds__(THREADS) sense_kernel(const SenseArgs A) {
  const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= A.total) return;
  const uint32_t S = 1u + (uint32_t)A.K + (uint32_t)A.Ms;
  const uint32_t row = i / S, slot = i - row * S;
  const uint32_t e = row / (uint32_t)A.N, n = row - e * (uint32_t)A.N;
  const uint32_t D = 9u + 4u * (uint32_t)(A.K + A.Ms);
  const size_t at = (size_t)row * D + (slot ? 9u + 4u * (slot - 1u) : 0u);
  const float* src = A.obs + at;
  float* dst = A.out + at;
  const bool own = slot == 0u, nbr = !own && slot <= (uint32_t)A.K;
  float v[9];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = src[k];
  if (own) {
#pragma unroll
    for (int k = 4; k < 9; ++k) v[k] = src[k];
  }
  const float sp = A.sig_p ? A.sig_p[e] : 0.f;
  const float sv = own && A.sig_v ? A.sig_v[e] : 0.f;
  const float so = A.sig_o ? A.sig_o[e] : 0.f;
  const float sig = own || nbr ? sp : so;
  bool noisy = A.active[row] != 0 && (sig != 0.f || sv != 0.f);
  if (!own) noisy = noisy && !(v[0] == 0.f && v[1] == 0.f && v[2] == 0.f && v[3] == 0.f);  // a padding slot
  if (noisy) {
    const uint32_t g = (uint32_t)(A.env_offset + (long long)e);
    const uint32_t ep = A.episode[e], st = (uint32_t)A.step_count[e];
    float z[4];
    if (sig != 0.f) {
      block_normals<3>(g, n, own ? 0u : slot + 1u, STREAM_SENSE, ep, st, A.seed_lo, A.seed_hi, z);
      if (own) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float nk = sig * z[k];
          v[k] = v[k] + nk;          // measured position
          v[6 + k] = v[6 + k] - nk;  // goal - position: the goal is known, the position carries the error
        }
      } else if (nbr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] + sig * z[k];
        v[3] = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
      } else {
        v[3] = fmaxf(v[3] + sig * z[0], 0.f);
      }
    }
    if (sv != 0.f) {  // own lanes only
      block_normals<3>(g, n, 1u, STREAM_SENSE, ep, st, A.seed_lo, A.seed_hi, z);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[3 + k] = v[3 + k] + sv * z[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[k] = v[k];
  if (own) {
#pragma unroll
    for (int k = 4; k < 9; ++k) dst[k] = v[k];
  }
}

int check_table(const swarm_delay_table_t& t, int ring_slots) {
  if (ring_slots < 1 || ring_slots > SWARM_PERTURB_MAX_DELAY + 1)
    return g_err.fail(SWARM_ELIMIT, "ring_slots out of range [1, SWARM_PERTURB_MAX_DELAY + 1]");
  if (t.count < 1 || t.count > SWARM_PERTURB_MAX_DELAY + 1)
    return g_err.fail(SWARM_EINVAL, "the delay table needs 1 .. SWARM_PERTURB_MAX_DELAY + 1 entries");
  for (int i = 0; i < t.count; ++i) {
    if (t.values[i] < 0) return g_err.fail(SWARM_EINVAL, "a delay is negative");
    if (t.values[i] > SWARM_PERTURB_MAX_DELAY) return g_err.fail(SWARM_ELIMIT, "a delay exceeds SWARM_PERTURB_MAX_DELAY");
    if (t.values[i] >= ring_slots) return g_err.fail(SWARM_EINVAL, "a delay does not fit the ring (ring_slots <= delay)");
    if (!(t.cum[i] >= 0.f && t.cum[i] <= 1.f) || (i && t.cum[i] < t.cum[i - 1]))
      return g_err.fail(SWARM_EINVAL, "cum must rise from 0 to 1");
  }
  if (t.cum[t.count - 1] != 1.f) return g_err.fail(SWARM_EINVAL, "the last cum entry must be 1");
  return SWARM_OK;
}

int check_batch(int E, int N) {
  if (E < 0) return g_err.fail(SWARM_EINVAL, "num_envs < 0");
  if (N < 1 || N > SWARM_PERTURB_MAX_AGENTS) return g_err.fail(SWARM_ELIMIT, "num_drones out of range [1, 256]");
  return SWARM_OK;
}

}  // namespace

extern "C" {

const char* swarm_perturb_last_error(void) { return g_err.msg; }

int swarm_actuate(const swarm_actuate_args_t* a, void* hip_stream) {
  if (!a) return g_err.fail(SWARM_ENULL, "args is NULL");
  if (int rc = check_batch(a->num_envs, a->num_drones)) return rc;
  if (int rc = check_table(a->delays, a->ring_slots)) return rc;
  if (a->num_envs == 0) return SWARM_OK;
  if ((long long)a->num_envs * a->num_drones > 0x7fffffffLL / 3) return g_err.fail(SWARM_ELIMIT, "num_envs * num_drones * 3 >= 2^31");
  if (!a->step_count || !a->episode) return g_err.fail(SWARM_ENULL, "step_count/episode is NULL");
  ActArgs k;
  k.actions = a->actions;
  k.ring = a->ring;
  k.delay_override = a->delay_override;
  k.thrust_noise_std = a->thrust_noise_std;
  k.step_count = a->step_count;
  k.episode = a->episode;
  k.eff = a->eff;
  k.delay_out = a->delay_out;
  k.delays = a->delays;
  k.seed_lo = (uint32_t)a->seed;
  k.seed_hi = (uint32_t)(a->seed >> 32);
  k.env_offset = a->env_offset;
  k.E = a->num_envs;
  k.N = a->num_drones;
  k.R = a->ring_slots;
  if (!a->actions) {  // the delays alone
    if (a->ring || a->eff) return g_err.fail(SWARM_ENULL, "actions is NULL");
    if (!a->delay_out) return g_err.fail(SWARM_ENULL, "actions and delay_out are NULL");
    hipLaunchKernelGGL(delay_kernel, dim3((a->num_envs + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)hip_stream, k);
    return g_err.launch_status();
  }
  if (!a->ring || !a->eff) return g_err.fail(SWARM_ENULL, "ring/eff is NULL");
  const long long lanes = (long long)a->num_envs * a->num_drones;
  hipLaunchKernelGGL(actuate_kernel, dim3((unsigned)((lanes + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)hip_stream,
                     k);
  return g_err.launch_status();
}

int swarm_sense(const swarm_sense_args_t* a, void* hip_stream) {
  if (!a) return g_err.fail(SWARM_ENULL, "args is NULL");
  if (int rc = check_batch(a->num_envs, a->num_drones)) return rc;
  if (a->neighbor_k < 0 || a->sensed_obstacles < 0) return g_err.fail(SWARM_EINVAL, "neighbor_k/sensed_obstacles < 0");
  if (a->neighbor_k > SWARM_PERTURB_MAX_K) return g_err.fail(SWARM_ELIMIT, "neighbor_k out of range [0, 16]");
  if (a->sensed_obstacles > SWARM_PERTURB_MAX_MS) return g_err.fail(SWARM_ELIMIT, "sensed_obstacles out of range [0, 5]");
  if (a->num_envs == 0) return SWARM_OK;
  const long long S = 1 + a->neighbor_k + a->sensed_obstacles;
  const long long lanes = (long long)a->num_envs * a->num_drones * S;
  if (lanes > 0x7fffffffLL) return g_err.fail(SWARM_ELIMIT, "num_envs * num_drones * (1 + K + Ms) >= 2^31");
  if (!a->obs || !a->active || !a->step_count || !a->episode || !a->out) return g_err.fail(SWARM_ENULL, "a sense buffer is NULL");
  if (a->obs == a->out) return g_err.fail(SWARM_EINVAL, "out must be another buffer than obs");
  SenseArgs k;
  k.obs = a->obs;
  k.active = a->active;
  k.sig_p = a->position_noise_std;
  k.sig_v = a->velocity_noise_std;
  k.sig_o = a->obstacle_noise_std;
  k.step_count = a->step_count;
  k.episode = a->episode;
  k.out = a->out;
  k.seed_lo = (uint32_t)a->seed;
  k.seed_hi = (uint32_t)(a->seed >> 32);
  k.env_offset = a->env_offset;
  k.total = (uint32_t)lanes;
  k.N = a->num_drones;
  k.K = a->neighbor_k;
  k.Ms = a->sensed_obstacles;
  hipLaunchKernelGGL(sense_kernel, dim3((unsigned)((lanes + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)hip_stream,
                     k);
  return g_err.launch_status();
}

}  // extern "C"
