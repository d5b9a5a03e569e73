// swarm_value.hip — the per-agent critic of a PPO rollout batch (gfx950): V(obs) per agent row and
// GAE with a per-agent value.
//
// The reference's multi-agent and single-agent PPO set-ups (build_multi_agent_ppo_config /
// build_single_agent_ppo_config, src/swarm_marl/training/config_builders.py) use RLlib's default
// TorchFC with fcnet_hiddens [256, 256], relu and vf_share_layers=False: next to the actor a
// separate value tower obs -> 256 -> 256 -> 1, evaluated on every agent's own observation:
//     value = W3 relu(W2 relu(W1 obs + b1) + b2) + b3
// A value batch is (T+1) x E x N rows, N times the centralized critic's; at in_dim <= 47 the whole
// network fits a CU's LDS (W1 24 KB + W2 128 KB + 2 KB), as the actor's does (swarm_policy.hip).
//
// bf16 path: policy_mlp_bf16's design with critic_mlp_bf16's one-output last layer.  The blob is
// staged in LDS once per workgroup, weights in MFMA-fragment order (one 1-KB block of 64 lanes x
// 16 B per (out block, k step): every A read is one conflict-free ds_read_b128).  One wave owns a
// tile of 32 obs rows and computes layers 1 and 2 TRANSPOSED on v_mfma_f32_32x32x16_bf16,
// C[out][row] = W · X^T: the row index sits on the lane, so layer 1's f32 accumulators, relu'd and
// packed to bf16 in place, ARE layer 2's B operand; the layer-1 bias rides in the pad column
// k = in_dim of the obs fragment (x = 1).  Layer 3 has one output: relu(h2), rounded to bf16 like
// every other activation, times the bf16-rounded w3 in f32 on the VALU, summed per lane over the
// out blocks in order and the 16 registers of each in order, the two lane halves joined by one
// __shfl_xor(., 32), plus b3 — no layer-3 MFMAs (the actor spends 16 of its 168 per tile there).
// A value depends on its own row only: an MFMA output column is a function of its own B column,
// everything after it is per lane in a fixed order.
//
// f32 path (parity with an f32 learner; no speed claim): swarm_critic_pack's f32 blob and
// swarm_critic_forward's f32 kernel, which take any in_dim.
//
// swarm_gae_agent: swarm_gae's loop with value[t,e,n]; see the header.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "swarm_mi355x.h"
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

// bf16 blob: [W1F 8 x 3 blocks][W2F 8 x 16 blocks][b2 256 f32][w3 256 f32, bf16-rounded][b3, 4 f32]
constexpr size_t L_W1 = 0;
constexpr size_t L_W2 = L_W1 + (size_t)OB * KS1 * FRAG;
constexpr size_t L_B2 = L_W2 + (size_t)OB * KS2 * FRAG;
constexpr size_t L_W3 = L_B2 + H * 4;
constexpr size_t L_B3 = L_W3 + H * 4;
constexpr size_t L_TOTAL = L_B3 + 16;  // 157,712 B: one workgroup per CU (160 KiB of LDS)
static_assert(L_TOTAL % 16 == 0 && L_TOTAL <= 160 * 1024, "the blob is staged whole, in 16-B pieces");

struct ValueArgs {
  const void* w;     // packed blob (device)
  const float* obs;  // [rows, in]
  float* value;      // [rows]
  long long rows;
  int in;
};

// 8 waves per workgroup (one workgroup per CU: the LDS blob), one 32-row tile per wave: the actor's
// measured choice; ~124 registers, two waves per SIMD.  Two tiles per wave (every
// weight fragment feeding two MFMAs) do not fit 256 registers here either: that variant compiled
// with 224 spilled VGPRs and was not run.
// IN_C: compile-time obs width (0 = runtime): the obs gather's pad and bias selects fold away for the
// env's default D = 37.
template <int WAVES, int IN_C = 0>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WAVES / 4 > 0 ? WAVES / 4 : 1)))
value_mlp_bf16(const ValueArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  {  // stage the packed blob (154 KB) in LDS, once per workgroup: 8 loads in flight per thread per round
    const int4* src = reinterpret_cast<const int4*>(A.w);
    int4* dst = reinterpret_cast<int4*>(lds);
    constexpr int N16 = (int)(L_TOTAL / 16), UNR = 8, STRIDE = 64 * WAVES;
    for (int base = threadIdx.x; base < N16; base += STRIDE * UNR) {
      int4 v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int i = base + u * STRIDE;
        v[u] = src[i < N16 ? i : N16 - 1];
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int i = base + u * STRIDE;
        if (i < N16) dst[i] = v[u];
      }
    }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const long long ntiles = (A.rows + 31) / 32;
  const float* b2 = reinterpret_cast<const float*>(lds + L_B2);
  const float* w3 = reinterpret_cast<const float*>(lds + L_W3);
  const float b3 = *reinterpret_cast<const float*>(lds + L_B3);
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * WAVES) {
    // opaque per tile: what derives from the lane index and the obs width is recomputed per tile
    // instead of being hoisted out of the loop, where it would stay live next to h1 (swarm_policy.hip)
    int lane = threadIdx.x & 63, in_r = A.in;
    asm volatile("" : "+v"(lane), "+s"(in_r));
    const int in = IN_C ? IN_C : in_r;
    const int n = lane & 31, h = (lane >> 5) & 1;
    const uint32_t lb = 16u * (uint32_t)lane;
    const bf16x8* w1f = reinterpret_cast<const bf16x8*>(lds + L_W1 + lb);
    const bf16x8* w2f = reinterpret_cast<const bf16x8*>(lds + L_W2 + lb);
    const long long row = tile * 32 + n;
    const bool valid = row < A.rows;
    // ---- obs fragments (B of layer 1): x[row][16 ks + 8 h + j], x[in] = 1 (bias column).
    // Unconditional loads from clamped addresses (one wait for all of them), then selects.
    bf16x8 xb[KS1];
    {
      const float* xr = A.obs + (valid ? row : A.rows - 1) * in;
      float xv[KS1 * 8];
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * ks + 8 * h + j;
          xv[ks * 8 + j] = xr[k < in ? k : in - 1];
        }
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * ks + 8 * h + j;
          xb[ks][j] = (__bf16)(k < in ? xv[ks * 8 + j] : (k == in ? 1.f : 0.f));
        }
    }
    // ---- layer 1: 256 x (in + 1), relu -> h1 (16 k-step fragments)
    bf16x8 h1[KS2];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      f32x16 acc = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[(ob * KS1 + ks) * 64], xb[ks], acc, 0, 0, 0);
      h1[2 * ob] = pack8(acc, 0, true);
      h1[2 * ob + 1] = pack8(acc, 1, true);
      __builtin_amdgcn_sched_barrier(0);  // keep each out block's fragment reads inside it
    }
    // ---- layer 2 (256 x 256, relu) fused with layer 3 (1 x 256): each out block's relu'd bf16
    // activations are multiplied by their w3 and summed right away, so h2 is never held whole
    float v = 0.f;
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      f32x16 acc, w3v;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b = *reinterpret_cast<const float4*>(b2 + ob * 32 + 8 * g + 4 * h);
        const float4 w = *reinterpret_cast<const float4*>(w3 + ob * 32 + 8 * g + 4 * h);
        acc[4 * g + 0] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
        w3v[4 * g + 0] = w.x; w3v[4 * g + 1] = w.y; w3v[4 * g + 2] = w.z; w3v[4 * g + 3] = w.w;
      }
#pragma unroll
      for (int ks = 0; ks < KS2; ++ks) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[(ob * KS2 + ks) * 64], h1[ks], acc, 0, 0, 0);
        if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // <= 8 fragments (32 VGPRs) in flight
      }
      // register i holds hidden unit ob * 32 + (i & 3) + 8 (i >> 2) + 4 h of the lane's row; a bf16
      // pair widens to f32 with a shift and a mask
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32x4 p = pack8_u32(acc, s, true);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v = v + w3v[8 * s + 2 * q] * __uint_as_float(p[q] << 16);
          v = v + w3v[8 * s + 2 * q + 1] * __uint_as_float(p[q] & 0xffff0000u);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    v = v + __shfl_xor(v, 32);
    if (h == 0 && valid) A.value[row] = v + b3;
  }
}

constexpr int BF16_WAVES = 8;

thread_local UnitError g_err;
// an error of the f32 path's swarm_critic_* call, under this unit's name
int vcritic(int code) { return code < 0 ? g_err.fail(code, swarm_critic_last_error()) : code; }

}  // namespace

extern "C" {

const char* swarm_value_last_error(void) { return g_err.msg; }

long long swarm_value_packed_bytes(int in_dim, int precision) {
  if (in_dim < 1 || in_dim > SWARM_POLICY_MAX_IN)
    return g_err.fail(SWARM_ELIMIT, "value in_dim out of range [1, 47]"), (long long)SWARM_ELIMIT;
  if (precision == SWARM_POLICY_BF16) return (long long)L_TOTAL;
  if (precision == SWARM_POLICY_F32) return (long long)vcritic((int)swarm_critic_packed_bytes(in_dim, precision));
  if (precision == SWARM_POLICY_F32X3)
    return g_err.fail(SWARM_ELIMIT, "the per-agent critic has no f32x3 path (bf16 or f32)"), (long long)SWARM_ELIMIT;
  return g_err.fail(SWARM_EINVAL, "unknown precision"), (long long)SWARM_EINVAL;
}

int swarm_value_pack(int in_dim, int precision, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, void* host_out) {
  const long long nb = swarm_value_packed_bytes(in_dim, precision);
  if (nb < 0) return (int)nb;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !host_out) return g_err.fail(SWARM_ENULL, "null weight pointer");
  if (precision == SWARM_POLICY_F32) return vcritic(swarm_critic_pack(in_dim, precision, w1, b1, w2, b2, w3, b3, host_out));
  memset(host_out, 0, (size_t)nb);
  unsigned char* base = static_cast<unsigned char*>(host_out);
  pack_w1f(base + L_W1, w1, b1, in_dim, KS1, W1_OB_MAJOR, ToBf16());  // the actor's W1F
  pack_w2f(base + L_W2, w2, ToBf16());
  memcpy(base + L_B2, b2, H * 4);
  pack_w3_row(reinterpret_cast<float*>(base + L_W3), w3);
  memcpy(base + L_B3, b3, 4);
  return SWARM_OK;
}

int swarm_value_forward(const swarm_value_t* v, const float* obs, long long rows, float* value, void* hip_stream) {
  if (!v || !v->weights) return g_err.fail(SWARM_ENULL, "value/weights is NULL");
  const long long nb = swarm_value_packed_bytes(v->in_dim, v->precision);
  if (nb < 0) return (int)nb;
  if (rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (rows == 0) return SWARM_OK;
  if (!obs || !value) return g_err.fail(SWARM_ENULL, "obs/value is NULL");
  if (((uintptr_t)v->weights) % 16) return g_err.fail(SWARM_EINVAL, "weights must be 16-B aligned");
  if (v->precision == SWARM_POLICY_F32) {
    swarm_critic_t c;
    c.in_dim = v->in_dim;
    c.precision = v->precision;
    c.weights = v->weights;
    return vcritic(swarm_critic_forward(&c, obs, rows, value, hip_stream));
  }
  ValueArgs a;
  a.w = v->weights;
  a.obs = obs;
  a.value = value;
  a.rows = rows;
  a.in = v->in_dim;
  auto fn = v->in_dim == 37 ? value_mlp_bf16<BF16_WAVES, 37> : value_mlp_bf16<BF16_WAVES>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L_TOTAL) !=
      hipSuccess)
    return g_err.fail(SWARM_EHIP, "hipFuncSetAttribute failed");
  // one workgroup per CU at most (8 x 32 rows per pass of one): mirrored by tests/test_gpu_value.py
  const long long tiles = (rows + 31) / 32;
  hipLaunchKernelGGL(fn, dim3(grid_for((tiles + BF16_WAVES - 1) / BF16_WAVES, 1)), dim3(64 * BF16_WAVES), (int)L_TOTAL,
                     (hipStream_t)hip_stream, a);
  return g_err.launch_status();
}

int swarm_gae_agent(const float* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated,
                    const uint8_t* env_done, const uint8_t* valid, int T, int E, int N, float gamma, float lam,
                    float* advantage, float* value_target, void* hip_stream) {
  return gae_launch<true>(reward, value, terminated, truncated, env_done, valid, T, E, N, gamma, lam, advantage,
                          value_target, hip_stream, g_err);
}

}  // extern "C"
