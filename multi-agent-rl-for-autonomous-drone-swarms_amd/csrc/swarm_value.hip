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

#pragma clang fp contract(off)

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int H = SWARM_POLICY_HIDDEN;  // 256
constexpr int KP1 = 48;                 // layer-1 K (obs dim + bias column, padded)
constexpr int KS1 = KP1 / 16;           // 3 k-steps
constexpr int OB = H / 32;              // 8 out blocks of 32
constexpr int KS2 = H / 16;             // 16 k-steps over the hidden dim
constexpr int FRAG = 1024;              // bytes of one 64-lane x 16-B fragment block
static_assert(SWARM_POLICY_MAX_IN + 1 <= KP1, "the bias column sits inside the padded K");

// bf16 blob: [W1F 8 x 3 blocks][W2F 8 x 16 blocks][b2 256 f32][w3 256 f32, bf16-rounded][b3, 4 f32]
constexpr size_t L_W1 = 0;
constexpr size_t L_W2 = L_W1 + (size_t)OB * KS1 * FRAG;
constexpr size_t L_B2 = L_W2 + (size_t)OB * KS2 * FRAG;
constexpr size_t L_W3 = L_B2 + H * 4;
constexpr size_t L_B3 = L_W3 + H * 4;
constexpr size_t L_TOTAL = L_B3 + 16;  // 157,712 B: one workgroup per CU (160 KiB of LDS)
static_assert(L_TOTAL % 16 == 0 && L_TOTAL <= 160 * 1024, "the blob is staged whole, in 16-B pieces");

// hidden unit carried by k-step `ks` (of 16) of an accumulator-chained operand, lane half h, element j
// (swarm_policy.hip: the accumulator's register order)
inline int chained_k(int ks, int h, int j) { return (ks >> 1) * 32 + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }

uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf16_to_f32(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct ValueArgs {
  const void* w;     // packed blob (device)
  const float* obs;  // [rows, in]
  float* value;      // [rows]
  long long rows;
  int in;
};

// 8 accumulator values (sub-block s) -> relu'd bf16 pairs (swarm_policy.hip pack8: round to nearest
// keeps the sign, so the relu is a packed i16 max with 0 after the conversion)
__device__ __forceinline__ u32x4 pack8_relu(const f32x16& a, int s) {
  u32x4 w;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bf16x2 p = __builtin_convertvector((f32x2){a[8 * s + 2 * q], a[8 * s + 2 * q + 1]}, bf16x2);  // v_cvt_pk_bf16_f32
    s16x2 v = __builtin_bit_cast(s16x2, p);
    v = __builtin_elementwise_max(v, (s16x2){0, 0});  // v_pk_max_i16
    w[q] = __builtin_bit_cast(unsigned, v);
  }
  return w;
}

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
      h1[2 * ob] = __builtin_bit_cast(bf16x8, pack8_relu(acc, 0));
      h1[2 * ob + 1] = __builtin_bit_cast(bf16x8, pack8_relu(acc, 1));
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
        const u32x4 p = pack8_relu(acc, s);
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

struct GaeArgs {
  const float* reward;
  const float* value;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const uint8_t* env_done;
  const uint8_t* valid;
  float* advantage;
  float* value_target;
  int T, E, N;
  float gamma, lam;
};

// one thread per (env, agent), t from T - 1 down to 0: the header's loop, operation for operation
__global__ void __launch_bounds__(256) gae_agent_kernel(const GaeArgs A) {
  const long long en = (long long)A.E * A.N;
  const float gl = A.gamma * A.lam;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < en; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i / A.N;
    float carry = 0.f;
    for (int t = A.T - 1; t >= 0; --t) {
      const long long at = (long long)t * en + i;
      if (!A.valid[at]) {
        A.advantage[at] = 0.f;
        A.value_target[at] = 0.f;
        carry = 0.f;
        continue;
      }
      const bool done = (A.terminated[at] | A.truncated[at]) != 0 ||
                        (A.env_done[(long long)t * A.E + e] & (SWARM_ENV_TERMINATED | SWARM_ENV_TRUNCATED)) != 0;
      const float v = A.value[at];
      float nv = 0.f;
      if (!done) nv = A.value[at + en];
      const float prev = done ? 0.f : carry;
      const float delta = (A.reward[at] + A.gamma * nv) - v;
      carry = delta + gl * prev;
      A.advantage[at] = carry;
      A.value_target[at] = carry + v;
    }
  }
}

thread_local char g_verr[256] = "";
int vfail(int code, const char* msg) {
  strncpy(g_verr, msg, sizeof(g_verr) - 1);
  return code;
}
// an error of the f32 path's swarm_critic_* call, under this unit's name
int vcritic(int code) { return code < 0 ? vfail(code, swarm_critic_last_error()) : code; }

int device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
      (void)hipGetLastError();
      cus = 256;
    }
  }
  return cus;
}

int grid_for(long long blocks_needed, int per_cu) {
  const long long cap = (long long)device_cus() * per_cu;
  const long long g = blocks_needed < cap ? blocks_needed : cap;
  return g < 1 ? 1 : (int)g;
}

int launch_status() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return vfail(SWARM_EHIP, hipGetErrorString(e));
  return SWARM_OK;
}

}  // namespace

extern "C" {

const char* swarm_value_last_error(void) { return g_verr; }

long long swarm_value_packed_bytes(int in_dim, int precision) {
  if (in_dim < 1 || in_dim > SWARM_POLICY_MAX_IN)
    return vfail(SWARM_ELIMIT, "value in_dim out of range [1, 47]"), (long long)SWARM_ELIMIT;
  if (precision == SWARM_POLICY_BF16) return (long long)L_TOTAL;
  if (precision == SWARM_POLICY_F32) return (long long)vcritic((int)swarm_critic_packed_bytes(in_dim, precision));
  if (precision == SWARM_POLICY_F32X3)
    return vfail(SWARM_ELIMIT, "the per-agent critic has no f32x3 path (bf16 or f32)"), (long long)SWARM_ELIMIT;
  return vfail(SWARM_EINVAL, "unknown precision"), (long long)SWARM_EINVAL;
}

int swarm_value_pack(int in_dim, int precision, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, void* host_out) {
  const long long nb = swarm_value_packed_bytes(in_dim, precision);
  if (nb < 0) return (int)nb;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !host_out) return vfail(SWARM_ENULL, "null weight pointer");
  if (precision == SWARM_POLICY_F32) return vcritic(swarm_critic_pack(in_dim, precision, w1, b1, w2, b2, w3, b3, host_out));
  memset(host_out, 0, (size_t)nb);
  unsigned char* base = static_cast<unsigned char*>(host_out);
  uint16_t* w1f = reinterpret_cast<uint16_t*>(base + L_W1);
  uint16_t* w2f = reinterpret_cast<uint16_t*>(base + L_W2);
  for (int ob = 0; ob < OB; ++ob)
    for (int l = 0; l < 64; ++l) {
      const int m = ob * 32 + (l & 31), h = l >> 5;
      for (int ks = 0; ks < KS1; ++ks)
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * ks + 8 * h + j;
          const float v = k < in_dim ? w1[m * in_dim + k] : (k == in_dim ? b1[m] : 0.f);
          w1f[((ob * KS1 + ks) * 64 + l) * 8 + j] = bf16_rne(v);
        }
      for (int ks = 0; ks < KS2; ++ks)
        for (int j = 0; j < 8; ++j) w2f[((ob * KS2 + ks) * 64 + l) * 8 + j] = bf16_rne(w2[m * H + chained_k(ks, h, j)]);
    }
  memcpy(base + L_B2, b2, H * 4);
  float* w3f = reinterpret_cast<float*>(base + L_W3);
  for (int m = 0; m < H; ++m) w3f[m] = bf16_to_f32(bf16_rne(w3[m]));
  memcpy(base + L_B3, b3, 4);
  return SWARM_OK;
}

int swarm_value_forward(const swarm_value_t* v, const float* obs, long long rows, float* value, void* hip_stream) {
  if (!v || !v->weights) return vfail(SWARM_ENULL, "value/weights is NULL");
  const long long nb = swarm_value_packed_bytes(v->in_dim, v->precision);
  if (nb < 0) return (int)nb;
  if (rows < 0) return vfail(SWARM_EINVAL, "rows < 0");
  if (rows == 0) return SWARM_OK;
  if (!obs || !value) return vfail(SWARM_ENULL, "obs/value is NULL");
  if (((uintptr_t)v->weights) % 16) return vfail(SWARM_EINVAL, "weights must be 16-B aligned");
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
    return vfail(SWARM_EHIP, "hipFuncSetAttribute failed");
  // one workgroup per CU at most (8 x 32 rows per pass of one): mirrored by tests/test_gpu_value.py
  const long long tiles = (rows + 31) / 32;
  hipLaunchKernelGGL(fn, dim3(grid_for((tiles + BF16_WAVES - 1) / BF16_WAVES, 1)), dim3(64 * BF16_WAVES), (int)L_TOTAL,
                     (hipStream_t)hip_stream, a);
  return launch_status();
}

int swarm_gae_agent(const float* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated,
                    const uint8_t* env_done, const uint8_t* valid, int T, int E, int N, float gamma, float lam,
                    float* advantage, float* value_target, void* hip_stream) {
  if (T < 0 || E < 0 || N < 0) return vfail(SWARM_EINVAL, "T, E, N must be >= 0");
  if (T == 0 || E == 0 || N == 0) return SWARM_OK;
  if (!reward || !value || !terminated || !truncated || !env_done || !valid || !advantage || !value_target)
    return vfail(SWARM_ENULL, "a GAE buffer is NULL");
  GaeArgs a;
  a.reward = reward;
  a.value = value;
  a.terminated = terminated;
  a.truncated = truncated;
  a.env_done = env_done;
  a.valid = valid;
  a.advantage = advantage;
  a.value_target = value_target;
  a.T = T;
  a.E = E;
  a.N = N;
  a.gamma = gamma;
  a.lam = lam;
  const long long en = (long long)E * N;
  // the per-CU cap (32 blocks of 256 threads) is mirrored by tests/test_gpu_value_rollout.py
  hipLaunchKernelGGL(gae_agent_kernel, dim3(grid_for((en + 255) / 256, 32)), dim3(256), 0, (hipStream_t)hip_stream, a);
  return launch_status();
}

}  // extern "C"
