// PPO loss head for gfx950 (include/swarm_mi355x.h, "PPO loss head"): swarm_masked_moments and
// swarm_ppo_loss.  Both are streaming kernels over agent rows followed by a one-wave finalising
// launch; every sum over rows is f64, per-thread -> block tree -> workspace -> finalise, in a fixed
// order and without atomics.
//
// ppo_loss_kernel<A>: a lane owns a row.  The 8A-byte logits rows are read and written as A float2
// per lane: the 64 rows of a wave are one contiguous 512A-byte span, so every cache line that is
// fetched is used whole.  A workgroup of 256 lanes owns a tile of G = max(1, 256 / N) whole
// env-rows (G N <= 256 rows; lanes past G N idle), so the value gradient of an env-row is summed
// inside one workgroup through LDS.  Nothing but the valid byte is read from an invalid row: its
// loads sit under the branch.  The next tile's valid byte is loaded before the current tile is
// worked on, so the dependent loads of a tile do not wait for two memory round trips.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "swarm_mi355x.h"
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PART = 8;   // doubles per workgroup in the workspace
constexpr int GROUP = 16;  // terms of a group sum (finalise, value gradient)
static_assert(SWARM_PPO_MAX_BLOCKS * PART * 8 == SWARM_PPO_WORKSPACE_BYTES, "workspace holds every block's partials");
static_assert(SWARM_PPO_MAX_AGENTS == THREADS, "an env-row fits one workgroup");
static_assert(SWARM_PPO_MAX_BLOCKS == 64 * GROUP, "the finalising wave covers every partial");
static_assert(2 * SWARM_PPO_MAX_ACT <= SWARM_POLICY_MAX_OUT, "logits no wider than the actor's");

// Sum of v over the workgroup, the same bits in every thread: __shfl_down 32..1 inside a wave, then
// the wave sums in order.  `red` is WAVES doubles of LDS; the trailing barrier frees it for reuse.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s = s + red[w];
  __syncthreads();
  return s;
}

// Sum over the nb partials work[b * PART + j], b in index order in groups of GROUP: one wave, lane
// l adds its group, every lane then adds the 64 group sums in order (same bits in every lane).
__device__ __forceinline__ double final_sum(const double* work, int nb, int j, double* red) {
  const int l = threadIdx.x;
  double s = 0.0;
  for (int b = l * GROUP; b < nb && b < (l + 1) * GROUP; ++b) s = s + work[(size_t)b * PART + j];
  red[l] = s;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < 64; ++i) t = t + red[i];
  __syncthreads();
  return t;
}

// ---------------------------------------------------------------- masked moments
struct Shifted {
  double n = 0.0, p = 0.0, s = 0.0, q = 0.0;
  __device__ __forceinline__ void add(float xf) {
    const double x = (double)xf;
    if (n == 0.0) p = x;
    const double d = x - p;
    n = n + 1.0;
    s = s + d;
    q = q + d * d;
  }
};

template <bool VEC>
__global__ void __launch_bounds__(THREADS) moments_kernel(const float* __restrict__ x, const uint8_t* __restrict__ valid,
                                                          long long rows, double* __restrict__ work) {
  __shared__ double red[WAVES];
  Shifted a;
  const long long tid = (long long)blockIdx.x * THREADS + threadIdx.x;
  const long long stride = (long long)gridDim.x * THREADS;
  if (VEC) {
    const long long quads = rows >> 2;
    for (long long g = tid; g < quads; g += stride) {
      const uchar4 v = reinterpret_cast<const uchar4*>(valid)[g];
      if (v.x | v.y | v.z | v.w) {
        const float4 f = reinterpret_cast<const float4*>(x)[g];
        if (v.x) a.add(f.x);
        if (v.y) a.add(f.y);
        if (v.z) a.add(f.z);
        if (v.w) a.add(f.w);
      }
    }
    const long long r = (quads << 2) + tid;  // the last rows % 4 rows
    if (r < rows && valid[r]) a.add(x[r]);
  } else {
    for (long long r = tid; r < rows; r += stride)
      if (valid[r]) a.add(x[r]);
  }
  const double nb = block_sum(a.n, red);
  const double sx = block_sum(a.n * a.p + a.s, red);
  const double mb = nb > 0.0 ? sx / nb : 0.0;
  const double dp = mb - a.p;
  const double m2 = block_sum(a.n > 0.0 ? (a.q - 2.0 * dp * a.s) + a.n * dp * dp : 0.0, red);
  if (threadIdx.x == 0) {
    double* w = work + (size_t)blockIdx.x * PART;
    w[0] = nb;
    w[1] = mb;
    w[2] = m2;
    w[3] = nb * mb;
  }
}

__global__ void __launch_bounds__(64) moments_final(const double* __restrict__ work, int nb, double* __restrict__ out) {
  __shared__ double red[64];
  const double count = final_sum(work, nb, 0, red);
  const double sx = final_sum(work, nb, 3, red);
  const double mean = count > 0.0 ? sx / count : 0.0;
  const int l = threadIdx.x;
  double s = 0.0;
  for (int b = l * GROUP; b < nb && b < (l + 1) * GROUP; ++b) {
    const double d = work[(size_t)b * PART + 1] - mean;
    s = s + (work[(size_t)b * PART + 2] + work[(size_t)b * PART + 0] * d * d);
  }
  red[l] = s;
  __syncthreads();
  if (l == 0) {
    double m2 = 0.0;
    for (int i = 0; i < 64; ++i) m2 = m2 + red[i];
    const double var = count > 0.0 ? m2 / count : 0.0;
    const double sd = sqrt(var > 0.0 ? var : 0.0);
    out[0] = count;
    out[1] = mean;
    out[2] = sd;
    out[3] = 1.0 / (sd > 1e-4 ? sd : 1e-4);
  }
}

// ---------------------------------------------------------------- the loss head
struct Coef {
  float clip, vf_clip, vf_coeff, ent_coeff, kl_coeff;
};

template <int A>
__global__ void __launch_bounds__(THREADS) ppo_loss_kernel(const swarm_ppo_args_t P, const long long env_rows,
                                                           const long long tiles, const int G) {
  __shared__ double red[WAVES];
  __shared__ float s_gv[THREADS];
  __shared__ float s_part[THREADS];
  const int N = P.num_agents;
  const int C = (N + GROUP - 1) / GROUP;  // group sums per env-row
  const int lane = threadIdx.x;
  const int tile_rows = G * N;
  const int my_env = lane / N;  // env-row of this lane inside the tile
  const float mean = (float)P.adv_moments[1];
  const float inv_std = (float)P.adv_moments[3];
  const double Md = P.valid_moments[0];
  const float inv = Md > 0.0 ? (float)(1.0 / Md) : 0.f;
  const float lo = 1.f - P.clip_param, hi = 1.f + P.clip_param;
  const float c_v = P.vf_loss_coeff, c_e = P.entropy_coeff, c_kl = P.kl_coeff, vf_clip = P.vf_clip_param;
  const float2* lg2 = reinterpret_cast<const float2*>(P.logits);
  const float2* bl2 = reinterpret_cast<const float2*>(P.behaviour_logits);
  float2* gl2 = reinterpret_cast<float2*>(P.grad_logits);
  double a_cnt = 0.0, a_pol = 0.0, a_vf = 0.0, a_h = 0.0, a_kl = 0.0, a_clip = 0.0;

  auto tile_valid = [&](long long tile, bool& in_range) -> uint8_t {
    const long long er = tile * G + my_env;
    in_range = tile < tiles && lane < tile_rows && er < env_rows;
    return in_range ? P.valid[tile * tile_rows + lane] : (uint8_t)0;
  };
  bool in_next;
  uint8_t v_next = tile_valid(blockIdx.x, in_next);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const bool in_range = in_next;
    const uint8_t vld = v_next;
    v_next = tile_valid(tile + gridDim.x, in_next);
    const long long row = tile * tile_rows + lane;
    float gv = 0.f;
    if (in_range) {
      float g[2 * A];
#pragma unroll
      for (int k = 0; k < 2 * A; ++k) g[k] = 0.f;
      if (vld) {
        float l[2 * A], b[2 * A], act[A];
#pragma unroll
        for (int k = 0; k < A; ++k) {
          const float2 t = lg2[row * A + k], u = bl2[row * A + k];
          l[2 * k] = t.x;
          l[2 * k + 1] = t.y;
          b[2 * k] = u.x;
          b[2 * k + 1] = u.y;
        }
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = P.actions[row * A + k];
        const float lp_old = P.logp[row];
        const float adv = (P.advantage[row] - mean) * inv_std;
        const float d = P.value[tile * G + my_env] - P.value_target[row];
        float e[A], z[A], u[A];
        float lp = 0.f, ent = 0.f, kl = 0.f;
#pragma unroll
        for (int k = 0; k < A; ++k) {
          const float s = l[A + k];
          e[k] = expf(-s);
          z[k] = (act[k] - l[k]) * e[k];
          lp = lp + (-0.5f * z[k] * z[k] - s);
          ent = ent + s;
          const float dm = b[k] - l[k];
          u[k] = expf(2.f * b[A + k]) + dm * dm;
          kl = kl + (((s - b[A + k]) + 0.5f * u[k] * (e[k] * e[k])) - 0.5f);
        }
        lp = lp - 0.5f * (float)A * 1.8378770664093453f;    // log(2 pi)
        ent = ent + 0.5f * (float)A * 2.8378770664093453f;  // log(2 pi e)
        const float r = expf(lp - lp_old);
        const float rc = fminf(fmaxf(r, lo), hi);
        const float surr = fminf(adv * r, adv * rc);
        const bool clipped = (adv > 0.f && r > hi) || (adv < 0.f && r < lo);
        const float d2 = d * d;
        const float vf = fminf(d2, vf_clip);
        gv = d2 < vf_clip ? inv * c_v * 2.f * d : 0.f;
        const float w = clipped ? 0.f : -(adv * r);
#pragma unroll
        for (int k = 0; k < A; ++k) {
          const float ee = e[k] * e[k];
          g[k] = inv * (w * z[k] * e[k] + c_kl * (l[k] - b[k]) * ee);
          g[A + k] = inv * ((w * (z[k] * z[k] - 1.f) - c_e) + c_kl * (1.f - u[k] * ee));
        }
        a_cnt = a_cnt + 1.0;
        a_pol = a_pol + (double)(-surr);
        a_vf = a_vf + (double)vf;
        a_h = a_h + (double)ent;
        a_kl = a_kl + (double)kl;
        a_clip = a_clip + (clipped ? 1.0 : 0.0);
      }
#pragma unroll
      for (int k = 0; k < A; ++k) gl2[row * A + k] = make_float2(g[2 * k], g[2 * k + 1]);
    }
    // value gradient of the tile's env-rows: group sums of 16 agents, then the groups in order
    s_gv[lane] = gv;
    __syncthreads();
    if (lane < G * C) {
      const int ge = lane / C, c = lane - ge * C;
      const int k1 = (c + 1) * GROUP < N ? (c + 1) * GROUP : N;
      float s = 0.f;
      for (int k = c * GROUP; k < k1; ++k) s = s + s_gv[ge * N + k];
      s_part[lane] = s;
    }
    __syncthreads();
    if (lane < G && tile * G + lane < env_rows) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s = s + s_part[lane * C + c];
      P.grad_value[tile * G + lane] = s;
    }
  }
  const double t0 = block_sum(a_cnt, red), t1 = block_sum(a_pol, red), t2 = block_sum(a_vf, red);
  const double t3 = block_sum(a_h, red), t4 = block_sum(a_kl, red), t5 = block_sum(a_clip, red);
  if (lane == 0) {
    double* w = static_cast<double*>(P.workspace) + (size_t)blockIdx.x * PART;
    w[0] = t0;
    w[1] = t1;
    w[2] = t2;
    w[3] = t3;
    w[4] = t4;
    w[5] = t5;
  }
}

__global__ void __launch_bounds__(64) ppo_final(const double* __restrict__ work, int nb, const double* __restrict__ valid_moments,
                                                Coef c, double* __restrict__ stats) {
  __shared__ double red[64];
  double t[6];
  for (int j = 0; j < 6; ++j) t[j] = final_sum(work, nb, j, red);
  if (threadIdx.x == 0) {
    const double M = valid_moments[0];
    const double inv = M > 0.0 ? 1.0 / M : 0.0;
    const double pol = inv * t[1], vf = inv * t[2], h = inv * t[3], kl = inv * t[4];
    stats[0] = t[0];
    stats[1] = ((pol + (double)c.vf_coeff * vf) - (double)c.ent_coeff * h) + (double)c.kl_coeff * kl;
    stats[2] = pol;
    stats[3] = vf;
    stats[4] = h;
    stats[5] = kl;
    stats[6] = inv * t[5];
  }
}

thread_local UnitError g_err;

template <int A>
void launch_loss(const swarm_ppo_args_t& a, long long env_rows, long long tiles, int G, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(ppo_loss_kernel<A>, dim3(blocks), dim3(THREADS), 0, s, a, env_rows, tiles, G);
}

}  // namespace

extern "C" {

const char* swarm_ppo_last_error(void) { return g_err.msg; }

int swarm_masked_moments(const float* x, const uint8_t* valid, long long rows, void* workspace, double* out,
                         void* hip_stream) {
  if (rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (rows == 0) return SWARM_OK;
  if (!x || !valid || !workspace || !out) return g_err.fail(SWARM_ENULL, "x/valid/workspace/out is NULL");
  if (((uintptr_t)workspace) % 8 || ((uintptr_t)out) % 8 || ((uintptr_t)x) % 4)
    return g_err.fail(SWARM_EINVAL, "workspace/out must be 8-B aligned, x 4-B aligned");
  // 4 rows per thread and pass where the pointers allow 16-B / 4-B vector loads
  const bool vec = ((uintptr_t)x) % 16 == 0 && ((uintptr_t)valid) % 4 == 0;
  const long long per_block = (long long)THREADS * (vec ? 16 : 4);
  long long nb = (rows + per_block - 1) / per_block;
  if (nb > SWARM_PPO_MAX_BLOCKS) nb = SWARM_PPO_MAX_BLOCKS;
  hipStream_t s = (hipStream_t)hip_stream;
  double* work = static_cast<double*>(workspace);
  if (vec)
    hipLaunchKernelGGL(moments_kernel<true>, dim3((int)nb), dim3(THREADS), 0, s, x, valid, rows, work);
  else
    hipLaunchKernelGGL(moments_kernel<false>, dim3((int)nb), dim3(THREADS), 0, s, x, valid, rows, work);
  hipLaunchKernelGGL(moments_final, dim3(1), dim3(64), 0, s, (const double*)work, (int)nb, out);
  return g_err.launch_status();
}

int swarm_ppo_loss(const swarm_ppo_args_t* args, void* hip_stream) {
  if (!args) return g_err.fail(SWARM_ENULL, "args is NULL");
  const swarm_ppo_args_t& a = *args;
  if (a.rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (a.act_dim < 1 || a.act_dim > SWARM_PPO_MAX_ACT) return g_err.fail(SWARM_ELIMIT, "act_dim out of range [1, 6]");
  if (a.num_agents < 1 || a.num_agents > SWARM_PPO_MAX_AGENTS)
    return g_err.fail(SWARM_ELIMIT, "num_agents out of range [1, 256]");
  if (a.rows % a.num_agents) return g_err.fail(SWARM_EINVAL, "rows is not a multiple of num_agents");
  if (a.rows == 0) return SWARM_OK;
  if (!a.logits || !a.behaviour_logits || !a.actions || !a.logp || !a.advantage || !a.value_target || !a.value ||
      !a.valid || !a.adv_moments || !a.valid_moments || !a.grad_logits || !a.grad_value || !a.stats || !a.workspace)
    return g_err.fail(SWARM_ENULL, "a PPO buffer is NULL");
  if (((uintptr_t)a.logits) % 8 || ((uintptr_t)a.behaviour_logits) % 8 || ((uintptr_t)a.grad_logits) % 8 ||
      ((uintptr_t)a.workspace) % 8 || ((uintptr_t)a.stats) % 8 || ((uintptr_t)a.adv_moments) % 8 ||
      ((uintptr_t)a.valid_moments) % 8)
    return g_err.fail(SWARM_EINVAL, "logits, behaviour_logits, grad_logits, the moments, stats and workspace must be 8-B aligned");
  const int G = THREADS / a.num_agents;  // >= 1: whole env-rows of a tile
  const long long env_rows = a.rows / a.num_agents;
  const long long tiles = (env_rows + G - 1) / G;
  const int blocks = (int)(tiles < SWARM_PPO_MAX_BLOCKS ? tiles : SWARM_PPO_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)hip_stream;
  switch (a.act_dim) {
    case 1: launch_loss<1>(a, env_rows, tiles, G, blocks, s); break;
    case 2: launch_loss<2>(a, env_rows, tiles, G, blocks, s); break;
    case 3: launch_loss<3>(a, env_rows, tiles, G, blocks, s); break;
    case 4: launch_loss<4>(a, env_rows, tiles, G, blocks, s); break;
    case 5: launch_loss<5>(a, env_rows, tiles, G, blocks, s); break;
    default: launch_loss<6>(a, env_rows, tiles, G, blocks, s); break;
  }
  const Coef c{a.clip_param, a.vf_clip_param, a.vf_loss_coeff, a.entropy_coeff, a.kl_coeff};
  hipLaunchKernelGGL(ppo_final, dim3(1), dim3(64), 0, s, (const double*)a.workspace, blocks, a.valid_moments, c, a.stats);
  return g_err.launch_status();
}

}  // extern "C"
