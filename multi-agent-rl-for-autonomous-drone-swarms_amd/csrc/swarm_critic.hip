// swarm_critic.hip — the device half of a PPO rollout batch (gfx950): the centralized critic
// V(global_state), the diagonal-Gaussian action log-probability and GAE.
//
// The reference's CTDE model (CentralizedCriticModel, src/swarm_marl/training/models.py) values a
// state with `value_model`, a TorchFC [256, 256] on global_state (width G = 6N + 3) with one output:
//     value = W3 relu(W2 relu(W1 gs + b1) + b2) + b3
// Its layer 1 is a K = G GEMM (K = 387 at N = 64, 1539 at N = 256): unlike the actor's (K <= 48,
// swarm_policy.hip) its weights do not fit LDS, so they stream.
//
// bf16 path: v_mfma_f32_32x32x16_bf16, f32 accumulation, computed TRANSPOSED as in the actor
// (C[out][row] = W · X^T: a layer's accumulators, relu'd and packed to bf16 in place, are the next
// layer's B operand).  One workgroup of 4 waves owns 128 rows, each wave a 32-row tile and all 256
// outputs of it (8 accumulator blocks, 128 registers).  The weights are ONE stream of 16-KB chunks
// in MFMA-fragment order, packed by the host: W1 in chunks of 2 k-steps x 8 out blocks, then W2 in
// chunks of 1 out block x 16 k-steps.  Chunk c + 1 is fetched from L2 into registers while chunk c
// is multiplied out of LDS, stored to the other LDS buffer afterwards, one barrier per chunk: every
// fragment is read from L2 once per 128 rows and from LDS once per wave.  The global_state tile of
// a W1 chunk (128 rows x 32 columns) is loaded coalesced (a wave reads two 128-B row segments per
// instruction), converted to bf16 and staged in LDS with an 80-B row stride (conflict-free
// ds_read_b128 B fragments); the layer-1 bias rides in the pad column k = in_dim (x = 1).
// Layer 3 has one output: relu(h2), rounded to bf16 like every other activation, times the
// bf16-rounded w3 in f32 on the VALU, summed over the lane's 16 x 8 hidden units and the two lane
// halves.
//
// f32 path (parity with an f32 learner; no speed claim): plain VALU, f32 products and f32 sums.
// One workgroup of 256 threads owns 32 rows, thread j hidden unit j; the inputs of a layer sit in
// LDS transposed ([k][row], read as broadcast float4s), the weights are packed transposed
// ([k][unit]: coalesced).  Every dot product is summed in blocks of 64 terms (block sums added to
// a running total), which keeps the rounding error of the K = 1540 sum near that of a blocked
// BLAS kernel.
//
// swarm_gaussian_logp / swarm_gae: one thread per row / per (env, agent); see the header.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "swarm_mi355x.h"
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

constexpr int KC = 2;                   // layer-1 k-steps per chunk
constexpr int WCHUNK = KC * OB * FRAG;  // 16 KB: one W1 chunk; one W2 chunk (1 out block x 16 k-steps) too
static_assert(WCHUNK == KS2 * FRAG, "W1 and W2 chunks share the LDS buffers");
constexpr int TILE = 128;               // rows per workgroup (4 waves x 32)
constexpr int XCOLS = KC * 16;          // 32 global_state columns per chunk
constexpr int XSTRIDE = XCOLS * 2 + 16; // 80 B per staged row: 16-B aligned, conflict-free b128 reads
constexpr int XCHUNK = TILE * XSTRIDE;  // 10 KB
constexpr int BF16_THREADS = 256;

// bf16 blob: [W chunks: nc1 W1 chunks, 8 W2 chunks][b2 256 f32][w3 256 f32, bf16-rounded][b3, 4 f32]
struct Bf16Layout {
  int nc1;
  size_t w2, b2, w3, b3, total;
  __host__ __device__ explicit Bf16Layout(int in) {
    nc1 = (in + 1 + XCOLS - 1) / XCOLS;
    w2 = (size_t)nc1 * WCHUNK;
    b2 = w2 + (size_t)OB * WCHUNK;
    w3 = b2 + H * 4;
    b3 = w3 + H * 4;
    total = b3 + 16;
  }
};
// f32 blob (floats): [W1T in x 256][b1 256][W2T 256 x 256][b2 256][w3 256][b3, 4]
struct F32Layout {
  size_t b1, w2, b2, w3, b3, total;
  __host__ __device__ explicit F32Layout(int in) {
    b1 = (size_t)in * H;
    w2 = b1 + H;
    b2 = w2 + (size_t)H * H;
    w3 = b2 + H;
    b3 = w3 + H;
    total = b3 + 4;
  }
};

struct CriticArgs {
  const void* w;     // packed blob (device)
  const float* gs;   // [rows, in]
  float* value;      // [rows]
  long long rows;
  int in;
};

// one thread's share of a 16-KB weight chunk: four 16-B pieces, BF16_THREADS apart (named members,
// not an array: an array the optimizer cannot split is moved to LDS or scratch)
struct WPiece {
  int4 a, b, c, d;
};
__device__ __forceinline__ WPiece wchunk_load(const int4* __restrict__ src, int t) {
  WPiece w;
  w.a = src[t];
  w.b = src[t + BF16_THREADS];
  w.c = src[t + 2 * BF16_THREADS];
  w.d = src[t + 3 * BF16_THREADS];
  return w;
}
__device__ __forceinline__ void wchunk_store(int4* dst, int t, const WPiece& w) {
  dst[t] = w.a;
  dst[t + BF16_THREADS] = w.b;
  dst[t + 2 * BF16_THREADS] = w.c;
  dst[t + 3 * BF16_THREADS] = w.d;
}

// ---------------------------------------------------------------- bf16 kernel
__global__ void __launch_bounds__(BF16_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2)))
critic_mlp_bf16(const CriticArgs A) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * WCHUNK + 2 * XCHUNK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = lane & 31, h = lane >> 5;
  const int in = A.in;
  const Bf16Layout L(in);
  const int nc1 = L.nc1;
  const unsigned char* wb = static_cast<const unsigned char*>(A.w);
  const int4* wsrc = reinterpret_cast<const int4*>(wb);  // chunk c: int4s [c * 1024, (c + 1) * 1024)
  const float* b2 = reinterpret_cast<const float*>(wb + L.b2);
  const float* w3 = reinterpret_cast<const float*>(wb + L.w3);
  const float b3 = *reinterpret_cast<const float*>(wb + L.b3);
  const long long ntiles = (A.rows + TILE - 1) / TILE;
  // staging map of the global_state tile: thread t owns column xc of rows xr + 8 i (i < 16)
  const int xc = t & 31, xr = t >> 5;
  constexpr int XL = TILE / 8;  // 16 loads per thread per chunk (held as one f32x16)
  static_assert(XL == 16, "the staged tile columns are held as one f32x16");

  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * TILE;
    // the chunk's tile columns, from clamped addresses (rows past the end re-read the last row,
    // columns past the end the last column), then the pad / bias selects
    auto load_x = [&](int c, f32x16& xv) {
      const int k = c * XCOLS + xc;
      const int kk = k < in ? k : in - 1;
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        long long r = row0 + xr + 8 * i;
        r = r < A.rows ? r : A.rows - 1;
        xv[i] = A.gs[r * in + kk];
      }
    };
    auto store_x = [&](int c, const f32x16& xv, unsigned char* xbuf) {
      const int k = c * XCOLS + xc;
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const float x = k < in ? xv[i] : (k == in ? 1.f : 0.f);
        *reinterpret_cast<__bf16*>(xbuf + (xr + 8 * i) * XSTRIDE + xc * 2) = (__bf16)x;
      }
    };
    {  // chunk 0 -> LDS buffer 0
      f32x16 xv;
      const WPiece wv = wchunk_load(wsrc, t);
      load_x(0, xv);
      wchunk_store(reinterpret_cast<int4*>(lds), t, wv);
      store_x(0, xv, lds + 2 * WCHUNK);
    }
    __syncthreads();
    // ---- layer 1: 256 x (in + 1) over nc1 chunks of 2 k-steps
    f32x16 acc[OB];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) acc[ob] = f32x16{};
    for (int c = 0; c < nc1; ++c) {
      // chunk c + 1 (the first W2 chunk after the last W1 chunk) on its way while chunk c multiplies
      f32x16 xv;
      const WPiece wv = wchunk_load(wsrc + (size_t)(c + 1) * (WCHUNK / 16), t);
      const bool more = c + 1 < nc1;
      if (more) load_x(c + 1, xv);
      // the loads stay up here: without the barrier the scheduler sinks them next to the LDS stores
      // below and the whole L2 round trip is exposed in every chunk
      __builtin_amdgcn_sched_barrier(0);
      const unsigned char* wl = lds + (c & 1) * WCHUNK + lane * 16;
      const unsigned char* xl = lds + 2 * WCHUNK + (c & 1) * XCHUNK + (wave * 32 + n) * XSTRIDE + h * 16;
#pragma unroll
      for (int ks = 0; ks < KC; ++ks) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(xl + ks * 32);
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(wl + (ks * OB + ob) * FRAG);
          acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[ob], 0, 0, 0);
        }
      }
      wchunk_store(reinterpret_cast<int4*>(lds + ((c + 1) & 1) * WCHUNK), t, wv);
      if (more) store_x(c + 1, xv, lds + 2 * WCHUNK + ((c + 1) & 1) * XCHUNK);
      __syncthreads();
    }
    // ---- relu -> h1: the accumulators in register order are layer 2's B fragments
    bf16x8 h1[KS2];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      h1[2 * ob] = pack8(acc[ob], 0, true);
      h1[2 * ob + 1] = pack8(acc[ob], 1, true);
    }
    // ---- layer 2 (256 x 256, relu), one out block per chunk, fused with layer 3 (1 x 256)
    float v = 0.f;
#pragma unroll 1
    for (int ob = 0; ob < OB; ++ob) {
      const int c = nc1 + ob;
      const bool more = ob + 1 < OB;
      // b2 / w3 of this out block first, the weight prefetch after them: vector-memory loads return
      // in order, so the wait for b2 before the first MFMA leaves the prefetch in flight
      f32x16 a2;
      f32x16 w3v;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b = *reinterpret_cast<const float4*>(b2 + ob * 32 + 8 * g + 4 * h);
        const float4 w = *reinterpret_cast<const float4*>(w3 + ob * 32 + 8 * g + 4 * h);
        a2[4 * g + 0] = b.x; a2[4 * g + 1] = b.y; a2[4 * g + 2] = b.z; a2[4 * g + 3] = b.w;
        w3v[4 * g + 0] = w.x; w3v[4 * g + 1] = w.y; w3v[4 * g + 2] = w.z; w3v[4 * g + 3] = w.w;
      }
      __builtin_amdgcn_sched_barrier(0);
      // (after the last chunk: this one again, not stored)
      const WPiece wv = wchunk_load(wsrc + (size_t)(more ? c + 1 : c) * (WCHUNK / 16), t);
      __builtin_amdgcn_sched_barrier(0);
      const unsigned char* wl = lds + (c & 1) * WCHUNK + lane * 16;
#pragma unroll
      for (int ks = 0; ks < KS2; ++ks) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(wl + ks * FRAG);
        a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, h1[ks], a2, 0, 0, 0);
      }
      // register i holds hidden unit ob * 32 + (i & 3) + 8 (i >> 2) + 4 h of the lane's row
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float r = a2[i] > 0.f ? a2[i] : 0.f;
        v = v + w3v[i] * (float)(__bf16)r;
      }
      if (more) wchunk_store(reinterpret_cast<int4*>(lds + ((c + 1) & 1) * WCHUNK), t, wv);
      __syncthreads();
    }
    v = v + __shfl_xor(v, 32);
    const long long row = row0 + wave * 32 + n;
    if (h == 0 && row < A.rows) A.value[row] = v + b3;
  }
}

// ---------------------------------------------------------------- f32 kernel
constexpr int F32_ROWS = 32;   // rows per workgroup
constexpr int F32_KB = 64;     // terms per block sum
constexpr int F32_XS = 36;     // floats per staged column (32 rows + pad: 16-B aligned rows of 4)

// acc[r] += sum over kk < kn of w[kk * H] * xs[kk][r], the block summed on its own first
__device__ __forceinline__ void f32_block(const float* __restrict__ w, const float* __restrict__ xs, int xstride, int kn,
                                          float (&acc)[F32_ROWS]) {
  float p[F32_ROWS];
#pragma unroll
  for (int r = 0; r < F32_ROWS; ++r) p[r] = 0.f;
  for (int kk = 0; kk < kn; ++kk) {
    const float wk = w[(size_t)kk * H];
    const float4* x4 = reinterpret_cast<const float4*>(xs + kk * xstride);
#pragma unroll
    for (int q = 0; q < F32_ROWS / 4; ++q) {
      const float4 x = x4[q];
      p[4 * q + 0] = p[4 * q + 0] + wk * x.x;
      p[4 * q + 1] = p[4 * q + 1] + wk * x.y;
      p[4 * q + 2] = p[4 * q + 2] + wk * x.z;
      p[4 * q + 3] = p[4 * q + 3] + wk * x.w;
    }
  }
#pragma unroll
  for (int r = 0; r < F32_ROWS; ++r) acc[r] = acc[r] + p[r];
}

__global__ void __launch_bounds__(H) critic_mlp_f32(const CriticArgs A) {
  __shared__ __attribute__((aligned(16))) float xs[F32_KB * F32_XS];  // [k][row] of one layer-1 block
  __shared__ __attribute__((aligned(16))) float hs[H * F32_ROWS];     // [unit][row]
  const int t = threadIdx.x, in = A.in;
  const F32Layout L(in);
  const float* wf = static_cast<const float*>(A.w);
  const long long ntiles = (A.rows + F32_ROWS - 1) / F32_ROWS;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * F32_ROWS;
    float acc[F32_ROWS];
#pragma unroll
    for (int r = 0; r < F32_ROWS; ++r) acc[r] = 0.f;
    // ---- layer 1
    for (int k0 = 0; k0 < in; k0 += F32_KB) {
      const int kn = in - k0 < F32_KB ? in - k0 : F32_KB;
      {  // stage columns [k0, k0 + kn) of the 32 rows: thread t column t & 63 of rows (t >> 6) + 4 i
        const int col = t & 63, rs = t >> 6;
#pragma unroll
        for (int i = 0; i < F32_ROWS / 4; ++i) {
          const int r = rs + 4 * i;
          const long long row = row0 + r;
          float x = 0.f;
          if (col < kn && row < A.rows) x = A.gs[row * in + k0 + col];
          xs[col * F32_XS + r] = x;
        }
      }
      __syncthreads();
      f32_block(wf + (size_t)k0 * H + t, xs, F32_XS, kn, acc);
      __syncthreads();
    }
    {
      const float b = wf[L.b1 + t];
#pragma unroll
      for (int r = 0; r < F32_ROWS; ++r) {
        const float s = acc[r] + b;
        hs[t * F32_ROWS + r] = s > 0.f ? s : 0.f;
        acc[r] = 0.f;
      }
    }
    __syncthreads();
    // ---- layer 2
    for (int k0 = 0; k0 < H; k0 += F32_KB) f32_block(wf + L.w2 + (size_t)k0 * H + t, hs + k0 * F32_ROWS, F32_ROWS, F32_KB, acc);
    __syncthreads();  // every thread is done reading h1
    {
      const float b = wf[L.b2 + t], w = wf[L.w3 + t];
#pragma unroll
      for (int r = 0; r < F32_ROWS; ++r) {
        const float s = acc[r] + b;
        hs[t * F32_ROWS + r] = w * (s > 0.f ? s : 0.f);  // layer 3's products
      }
    }
    __syncthreads();
    // ---- layer 3: thread t sums units [32 (t & 7), +32) of row t >> 3, then the 8 parts (fixed order)
    {
      const int r = t >> 3, part = t & 7;
      float s = 0.f;
      for (int q = 0; q < 32; ++q) s = s + hs[(part * 32 + q) * F32_ROWS + r];
      s = s + __shfl_xor(s, 1);
      s = s + __shfl_xor(s, 2);
      s = s + __shfl_xor(s, 4);
      const long long row = row0 + r;
      if (part == 0 && row < A.rows) A.value[row] = s + wf[L.b3];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- log-prob
__global__ void __launch_bounds__(256) gaussian_logp_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ actions, long long rows, int adim,
                                                            float* __restrict__ logp) {
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
    const float* lg = logits + r * 2 * adim;
    const float* a = actions + r * adim;
    float s = 0.f;
    for (int k = 0; k < adim; ++k) {
      const float ls = lg[adim + k];
      const float z = (a[k] - lg[k]) * expf(-ls);
      s = s + (-0.5f * z * z - ls);
    }
    logp[r] = s - 0.5f * (float)adim * 1.8378770664093453f;  // log(2 pi)
  }
}

thread_local UnitError g_err;

}  // namespace

extern "C" {

const char* swarm_critic_last_error(void) { return g_err.msg; }

long long swarm_critic_packed_bytes(int in_dim, int precision) {
  if (in_dim < 1 || in_dim > SWARM_CRITIC_MAX_IN)
    return g_err.fail(SWARM_ELIMIT, "critic in_dim out of range [1, 1539]"), (long long)SWARM_ELIMIT;
  if (precision == SWARM_POLICY_BF16) return (long long)Bf16Layout(in_dim).total;
  if (precision == SWARM_POLICY_F32) return (long long)F32Layout(in_dim).total * 4;
  if (precision == SWARM_POLICY_F32X3)
    return g_err.fail(SWARM_ELIMIT, "the critic has no f32x3 path (bf16 or f32)"), (long long)SWARM_ELIMIT;
  return g_err.fail(SWARM_EINVAL, "unknown precision"), (long long)SWARM_EINVAL;
}

int swarm_critic_pack(int in_dim, int precision, const float* w1, const float* b1, const float* w2, const float* b2,
                      const float* w3, const float* b3, void* host_out) {
  const long long nb = swarm_critic_packed_bytes(in_dim, precision);
  if (nb < 0) return (int)nb;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !host_out) return g_err.fail(SWARM_ENULL, "null weight pointer");
  memset(host_out, 0, (size_t)nb);
  if (precision == SWARM_POLICY_BF16) {
    const Bf16Layout L(in_dim);
    unsigned char* base = static_cast<unsigned char*>(host_out);
    pack_w1f(base, w1, b1, in_dim, L.nc1 * KC, W1_KS_MAJOR, ToBf16());  // chunk c: k-steps KC c .. KC c + KC - 1
    pack_w2f(base + L.w2, w2, ToBf16());  // chunk ob: the actor's W2F blocks of out block ob
    memcpy(base + L.b2, b2, H * 4);
    pack_w3_row(reinterpret_cast<float*>(base + L.w3), w3);
    memcpy(base + L.b3, b3, 4);
  } else {
    const F32Layout L(in_dim);
    float* f = static_cast<float*>(host_out);
    for (int k = 0; k < in_dim; ++k)
      for (int m = 0; m < H; ++m) f[(size_t)k * H + m] = w1[(size_t)m * in_dim + k];
    memcpy(f + L.b1, b1, H * 4);
    for (int k = 0; k < H; ++k)
      for (int m = 0; m < H; ++m) f[L.w2 + (size_t)k * H + m] = w2[m * H + k];
    memcpy(f + L.b2, b2, H * 4);
    memcpy(f + L.w3, w3, H * 4);
    f[L.b3] = b3[0];
  }
  return SWARM_OK;
}

int swarm_critic_forward(const swarm_critic_t* c, const float* gs, long long rows, float* value, void* hip_stream) {
  if (!c || !c->weights) return g_err.fail(SWARM_ENULL, "critic/weights is NULL");
  const long long nb = swarm_critic_packed_bytes(c->in_dim, c->precision);
  if (nb < 0) return (int)nb;
  if (rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (rows == 0) return SWARM_OK;
  if (!gs || !value) return g_err.fail(SWARM_ENULL, "gs/value is NULL");
  if (((uintptr_t)c->weights) % 16) return g_err.fail(SWARM_EINVAL, "weights must be 16-B aligned");
  CriticArgs a;
  a.w = c->weights;
  a.gs = gs;
  a.value = value;
  a.rows = rows;
  a.in = c->in_dim;
  hipStream_t s = (hipStream_t)hip_stream;
  // the per-CU caps (16 and 32 tiles) are mirrored by tests/test_gpu_critic.py test_second_grid_pass
  if (c->precision == SWARM_POLICY_BF16)
    hipLaunchKernelGGL(critic_mlp_bf16, dim3(grid_for((rows + TILE - 1) / TILE, 16)), dim3(BF16_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(critic_mlp_f32, dim3(grid_for((rows + F32_ROWS - 1) / F32_ROWS, 32)), dim3(H), 0, s, a);
  return g_err.launch_status();
}

int swarm_gaussian_logp(const float* logits, const float* actions, long long rows, int adim, float* logp,
                        void* hip_stream) {
  if (rows < 0 || adim < 1) return g_err.fail(SWARM_EINVAL, "rows < 0 or adim < 1");
  if (rows == 0) return SWARM_OK;
  if (!logits || !actions || !logp) return g_err.fail(SWARM_ENULL, "logits/actions/logp is NULL");
  // the per-CU cap (32 blocks, here and in swarm_gae) is mirrored by tests/test_gpu_rollout.py
  hipLaunchKernelGGL(gaussian_logp_kernel, dim3(grid_for((rows + 255) / 256, 32)), dim3(256), 0, (hipStream_t)hip_stream,
                     logits, actions, rows, adim, logp);
  return g_err.launch_status();
}

int swarm_gae(const float* reward, const float* value, const uint8_t* terminated, const uint8_t* truncated,
              const uint8_t* env_done, const uint8_t* valid, int T, int E, int N, float gamma, float lam,
              float* advantage, float* value_target, void* hip_stream) {
  return gae_launch<false>(reward, value, terminated, truncated, env_done, valid, T, E, N, gamma, lam, advantage,
                           value_target, hip_stream, g_err);
}

}  // extern "C"
