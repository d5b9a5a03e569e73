// swarm_nn.h — what the network units (swarm_policy / swarm_attn / swarm_critic / swarm_value /
// swarm_ppo / swarm_train .hip) must agree on, written once: the MFMA fragment geometry, the bf16
// blob formats (the element rules that host and device share, the host packers that loop over
// them, the actor blob's layout and dims check), the sampling noise, GAE, and the host-side error
// and grid helpers.
// Internal: not installed, not part of the C-ABI (include/swarm_mi355x.h); included as
// "swarm_nn.h", next to the sources.  Everything has internal linkage: every unit compiles its own
// copy, and a library may be linked from any subset of the units.
//
// Not here: the loops that stage a blob in LDS.  Outlined into a shared inline function they
// compile to a different prologue on gfx950 (other address arithmetic and ordering), and attn's
// differs anyway (it skips the W3 block): they stay in their kernels.  Nor the
// f32 blobs (chained_k_f32, the F32Layouts, the transposes), the other towers' layouts, the
// attention packer's float64 folds and swarm_train.hip's transposed W2^T / W3^T fragments: each
// has one user, or two with different layouts.
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
constexpr int KP1 = 48;                 // obs-tower bf16 layer-1 K (obs dim + bias column, padded)
constexpr int KS1 = KP1 / 16;           // 3 k-steps
static_assert(SWARM_POLICY_MAX_IN + 1 <= KP1, "the bias column sits inside the padded K");

// ---------------------------------------------------------------- blob formats: element rules (host and device)
// hidden unit carried by k-step `ks` (of 16) of an accumulator-chained operand, lane half h, element j:
// the accumulator's register order (swarm_policy.hip's header comment)
__host__ __device__ inline int chained_k(int ks, int h, int j) {
  return (ks >> 1) * 32 + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
}

__host__ __device__ inline uint16_t bf16_rne(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
struct ToBf16 {  // the bf16 blobs' element conversion
  __host__ __device__ uint16_t operator()(float v) const { return bf16_rne(v); }
};

// A fragment block is 64 lanes x 16 B: lane 32 h + n holds, as one 16-byte slot, the 8 elements j of
// row n of the block's 32 at the 8 k columns of k-step ks that lane half h carries.
// the slot of (block, row n, half h) among a region's slots, and back
__host__ __device__ inline int frag_slot(int blk, int n, int h) { return blk * 64 + 32 * h + n; }
struct FragSlot {
  int blk, n, h;
};
__host__ __device__ inline FragSlot frag_slot_of(int s) { return {s >> 6, s & 31, (s >> 5) & 1}; }
// W3F keeps only the `out` rows that exist: k-step ks, half h, logit m (the index of an element: 8 slot + j)
__host__ __device__ inline int w3f_slot(int out, int ks, int h, int m) { return ks * 2 * out + h * out + m; }
struct W3Slot {
  int ks, h, m;
};
__host__ __device__ inline W3Slot w3f_slot_of(int out, int s) {
  const int r = s % (2 * out);
  return {s / (2 * out), r / out, r % out};
}

// layer 1 augmented: row m, column k of [W1 | b1 | 0]
__host__ __device__ inline float l1_aug(const float* w1, const float* b1, int in, int m, int k) {
  return k < in ? w1[m * in + k] : (k == in ? b1[m] : 0.f);
}
// the slot of row m, k-step ks, half h: layer 1 in natural k order ...
template <class Cv>
__host__ __device__ inline void l1_slot(uint16_t (&e)[8], const float* w1, const float* b1, int in, int m, int ks, int h,
                                        Cv cv) {
  for (int j = 0; j < 8; ++j) e[j] = cv(l1_aug(w1, b1, in, m, 16 * ks + 8 * h + j));
}
// ... and a [*, 256] matrix read by an accumulator-chained operand (W2, W3) in chained k order
template <class Cv>
__host__ __device__ inline void chained_slot(uint16_t (&e)[8], const float* w, int m, int ks, int h, Cv cv) {
  for (int j = 0; j < 8; ++j) e[j] = cv(w[m * H + chained_k(ks, h, j)]);
}

// ---------------------------------------------------------------- blob formats: host packers
// W1F: OB x nks blocks of the augmented layer 1; block (ob, ks) at ob nks + ks (the obs towers: the
// kernels walk an out block's k-steps) or at ks OB + ob (the critic: it streams chunks of k-steps)
enum W1Order { W1_OB_MAJOR, W1_KS_MAJOR };
template <class Cv>
inline void pack_w1f(unsigned char* dst, const float* w1, const float* b1, int in, int nks, W1Order order, Cv cv) {
  uint16_t e[8];
  for (int ob = 0; ob < OB; ++ob)
    for (int ks = 0; ks < nks; ++ks)
      for (int l = 0; l < 64; ++l) {
        l1_slot(e, w1, b1, in, ob * 32 + (l & 31), ks, l >> 5, cv);
        memcpy(dst + (size_t)frag_slot(order == W1_KS_MAJOR ? ks * OB + ob : ob * nks + ks, l & 31, l >> 5) * 16, e, 16);
      }
}
// W2F: OB x KS2 blocks, block (ob, ks) at ob KS2 + ks
template <class Cv>
inline void pack_w2f(unsigned char* dst, const float* w2, Cv cv) {
  uint16_t e[8];
  for (int ob = 0; ob < OB; ++ob)
    for (int ks = 0; ks < KS2; ++ks)
      for (int l = 0; l < 64; ++l) {
        chained_slot(e, w2, ob * 32 + (l & 31), ks, l >> 5, cv);
        memcpy(dst + (size_t)frag_slot(ob * KS2 + ks, l & 31, l >> 5) * 16, e, 16);
      }
}
// W3F: KS2 k-steps x 2 halves x out rows
template <class Cv>
inline void pack_w3f(unsigned char* dst, const float* w3, int out, Cv cv) {
  uint16_t e[8];
  for (int ks = 0; ks < KS2; ++ks)
    for (int h = 0; h < 2; ++h)
      for (int m = 0; m < out; ++m) {
        chained_slot(e, w3, m, ks, h, cv);
        memcpy(dst + (size_t)w3f_slot(out, ks, h, m) * 16, e, 16);
      }
}
// the value towers' w3 row: bf16-rounded, kept as f32
inline void pack_w3_row(float* dst, const float* w3) {
  for (int m = 0; m < H; ++m) dst[m] = bf16_to_f32(bf16_rne(w3[m]));
}

// ---------------------------------------------------------------- the actor's bf16 blob
// [W1F 8x3 blocks][W2F 8x16 blocks][W3F 16 k-steps x 2*out lanes x 16 B][b2 256 f32][b3 32 f32]:
// swarm_policy_pack's bf16 blob (and, with f16 elements, each half of its f32x3 blob) and what
// swarm_train.hip's device packer writes
struct ActorLayout {
  int out;
  size_t w1, w2, w3, b2, b3, total;
  __host__ __device__ explicit ActorLayout(int o) : out(o) {
    w1 = 0;
    w2 = w1 + (size_t)OB * KS1 * FRAG;
    w3 = w2 + (size_t)OB * KS2 * FRAG;
    b2 = w3 + (size_t)KS2 * 2 * o * 16;
    b3 = b2 + H * 4;
    total = b3 + 32 * 4;
  }
};
inline bool actor_dims_ok(int in_dim, int out_dim) {
  return in_dim >= 1 && in_dim <= SWARM_POLICY_MAX_IN && out_dim >= 2 && out_dim <= SWARM_POLICY_MAX_OUT && !(out_dim & 1);
}
// the three fragment regions of one blob at `base`
template <class Cv>
inline void pack_actor_frags(unsigned char* base, const ActorLayout& L, int in, const float* w1, const float* b1,
                             const float* w2, const float* w3, Cv cv) {
  pack_w1f(base + L.w1, w1, b1, in, KS1, W1_OB_MAJOR, cv);
  pack_w2f(base + L.w2, w2, cv);
  pack_w3f(base + L.w3, w3, L.out, cv);
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
