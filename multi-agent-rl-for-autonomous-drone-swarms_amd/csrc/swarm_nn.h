// swarm_nn.h — what the network units (swarm_policy / swarm_attn / swarm_critic / swarm_value /
// swarm_ppo .hip) must agree on, written once: the MFMA fragment geometry and the packers that
// define the blob formats, the sampling noise, GAE, and the host-side error and grid helpers.
// Internal: not installed, not part of the C-ABI (include/swarm_mi355x.h); included as
// "swarm_nn.h", next to the sources.  Everything has internal linkage: every unit compiles its own
// copy, and a library may be linked from any subset of the units.
//
// Not here: the loops that stage a blob in LDS.  Outlined into a shared inline function they
// compile to a different prologue on gfx950 (other address arithmetic and ordering), and attn's
// differs anyway (it skips the W3 block): they stay in their kernels.
#pragma once

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
constexpr int OB = H / 32;              // 8 out blocks of 32
constexpr int KS2 = H / 16;             // 16 k-steps over the hidden dim
constexpr int FRAG = 1024;              // bytes of one 64-lane x 16-B fragment block

// ---------------------------------------------------------------- blob formats (host)
// hidden unit carried by k-step `ks` (of 16) of an accumulator-chained operand, lane half h, element j:
// the accumulator's register order (swarm_policy.hip's header comment)
inline int chained_k(int ks, int h, int j) { return (ks >> 1) * 32 + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }

inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// ---------------------------------------------------------------- accumulators -> bf16 fragment (device)
// 8 accumulator values (sub-block s) -> bf16 pairs, relu'd after the conversion when `act` (a
// compile-time constant at every call): round-to-nearest keeps the sign, so relu(bf16(x)) ==
// bf16(relu(x)), and a bf16 with the sign bit set is a negative int16: one v_pk_max_i16 with 0 relus
// two values (an f32 relu costs a canonicalising v_max plus the max on MFMA outputs: 4x the
// instructions).
__device__ __forceinline__ u32x4 pack8_u32(const f32x16& a, int s, bool act) {
  u32x4 w;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bf16x2 p = __builtin_convertvector((f32x2){a[8 * s + 2 * q], a[8 * s + 2 * q + 1]}, bf16x2);  // v_cvt_pk_bf16_f32
    s16x2 v = __builtin_bit_cast(s16x2, p);
    if (act) v = __builtin_elementwise_max(v, (s16x2){0, 0});  // v_pk_max_i16
    w[q] = __builtin_bit_cast(unsigned, v);
  }
  return w;
}
// the same as the next layer's B fragment
__device__ __forceinline__ bf16x8 pack8(const f32x16& a, int s, bool act) {
  return __builtin_bit_cast(bf16x8, pack8_u32(a, s, act));
}

// ---------------------------------------------------------------- sampling noise (device)
// Philox4x32-10 (same constants as the env's device reset)
__device__ __forceinline__ void philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// The six Box-Muller normals z[0..5] of row r from Philox(seed; row, counter) (tests/policy_ref.py
// sample_noise64); the second block is drawn only for ad > 2.  A: a forward kernel's argument block
// (seed_lo, seed_hi, ctr_lo, ctr_hi).  Every sampling actor draws through this one text.  It is a
// macro because policy_mlp_bf16 expands it in place: behind a call of an inline function, whatever
// its signature, that kernel compiles to other code than with the statements written out (the
// callee is simplified on its own before it is inlined) — and attn_policy_bf16, built on the
// function, to other code with them expanded in place.  Both kernels stay as they were.
#define SWARM_NORMALS(A, r, ad, z)                                                                                  \
  {                                                                                                                 \
    uint32_t c[4] = {(uint32_t)(r), (uint32_t)((unsigned long long)(r) >> 32), (A).ctr_lo, (A).ctr_hi};             \
    philox(c, (A).seed_lo, (A).seed_hi);                                                                            \
    uint32_t c2[4] = {(uint32_t)(r), (uint32_t)((unsigned long long)(r) >> 32) ^ 0x80000000u, (A).ctr_lo, (A).ctr_hi}; \
    if ((ad) > 2) philox(c2, (A).seed_lo, (A).seed_hi);                                                             \
    const uint32_t uu[8] = {c[0], c[1], c[2], c[3], c2[0], c2[1], c2[2], c2[3]};                                    \
    _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                                 \
      const float u1 = ((float)(uu[2 * p] >> 8) + 0.5f) * 0x1p-24f;                                                 \
      const float u2 = (float)(uu[2 * p + 1] >> 8) * 0x1p-24f;                                                      \
      const float rr = sqrtf(-2.f * logf(u1));                                                                      \
      (z)[2 * p] = rr * cosf(6.28318530717958647692f * u2);                                                         \
      (z)[2 * p + 1] = rr * sinf(6.28318530717958647692f * u2);                                                     \
    }                                                                                                               \
  }
// the same as a function, for the kernels that were built on one (swarm_attn.hip)
template <class Args>
__device__ __forceinline__ void normals(const Args& A, long long r, int ad, float (&z)[6]) {
  SWARM_NORMALS(A, r, ad, z)
}

// ---------------------------------------------------------------- errors, grid sizing (host)
// A unit's last error message: each unit keeps one thread_local instance behind its swarm_*_last_error.
struct UnitError {
  char msg[256];
  int fail(int code, const char* m) {
    strncpy(msg, m, sizeof(msg) - 1);
    return code;
  }
  int launch_status() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SWARM_EHIP, hipGetErrorString(e));
    return SWARM_OK;
  }
};

inline int device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
      (void)hipGetLastError();
      cus = 256;
    }
  }
  return cus;
}
// blocks_needed, capped at per_cu workgroups per CU; at least 1
inline int grid_for(long long blocks_needed, int per_cu) {
  const long long cap = (long long)device_cus() * per_cu;
  const long long g = blocks_needed < cap ? blocks_needed : cap;
  return g < 1 ? 1 : (int)g;
}

// ---------------------------------------------------------------- GAE
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

// one thread per (env, agent), t from T - 1 down to 0: the header's loop, operation for operation.
// PER_AGENT: value is [T + 1, E, N] (swarm_gae_agent), else [T + 1, E] (swarm_gae).  The value
// behind a done step is never read: its load sits under the branch.
template <bool PER_AGENT>
__global__ void __launch_bounds__(256) gae_kernel(const GaeArgs A) {
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
      const long long vt = PER_AGENT ? at : (long long)t * A.E + e;  // this step's value; the next step's is
      const long long vstep = PER_AGENT ? en : (long long)A.E;       // one time slice further
      const float v = A.value[vt];
      float nv = 0.f;
      if (!done) nv = A.value[vt + vstep];
      const float prev = done ? 0.f : carry;
      const float delta = (A.reward[at] + A.gamma * nv) - v;
      carry = delta + gl * prev;
      A.advantage[at] = carry;
      A.value_target[at] = carry + v;
    }
  }
}

// swarm_gae / swarm_gae_agent: the checks, then one launch; at most 32 blocks of 256 threads per CU
// (mirrored by tests/test_gpu_rollout.py and tests/test_gpu_value_rollout.py)
template <bool PER_AGENT>
int gae_launch(const float* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated,
               const uint8_t* env_done, const uint8_t* valid, int T, int E, int N, float gamma, float lam,
               float* advantage, float* value_target, void* hip_stream, UnitError& err) {
  if (T < 0 || E < 0 || N < 0) return err.fail(SWARM_EINVAL, "T, E, N must be >= 0");
  if (T == 0 || E == 0 || N == 0) return SWARM_OK;
  if (!reward || !value || !terminated || !truncated || !env_done || !valid || !advantage || !value_target)
    return err.fail(SWARM_ENULL, "a GAE buffer is NULL");
  const GaeArgs a{reward, value, terminated, truncated, env_done, valid, advantage, value_target, T, E, N, gamma, lam};
  const long long en = (long long)E * N;
  hipLaunchKernelGGL(gae_kernel<PER_AGENT>, dim3(grid_for((en + 255) / 256, 32)), dim3(256), 0, (hipStream_t)hip_stream, a);
  return err.launch_status();
}

}  // namespace
