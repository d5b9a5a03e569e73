// swarm_attn.hip — on-device attention actor (gfx950): the reference's
// CentralizedCriticModel(use_attention=True) actor (src/swarm_marl/training/models.py:104-137),
// eval mode.  The arithmetic, the two folds and the blob layout are written out in
// include/swarm_mi355x.h; the design notes are DESIGN.md §3.3.
//
// bf16 path: one fused launch.  A wave owns 64 observation rows per iteration.
//   front end (f32, VALU): lane l runs the whole front end of row l — o, t = A o + c0, the K
//     scores t . e_j, the softmax with the running row maximum subtracted, s = sum_j a_j e_j.  Every
//     weight it touches is wave-uniform, so the ~6 KB of front-end weights come through scalar
//     loads (constant address space) and ride in the SGPR operand of v_fma_f32: no LDS traffic, no
//     vector loads.  One pass over the neighbours: e_j is neither held (K <= 16) nor computed twice.
//   hand-over: the trunk is swarm_policy.hip's transposed MLP (C[out][row] = W . X^T, row on the
//     lane, 32 rows per tile, lane half h holding k = 16 ks + 8 h + j of k-step ks).  The layer-1
//     input is [s | own | obst | 1] on four k-steps, with s's columns ordered so that lane half h
//     needs s[16 h .. 16 h + 15]: lane l packs its row's s and tail to bf16 pairs and one
//     v_permlane32_swap per dword of (half-0 columns, half-1 columns) leaves the fragment of tile 0
//     (rows 0-31) in its first result and that of tile 1 (rows 32-63) in its second, on both halves.
//   trunk (bf16 MFMA, f32 accumulation), once per 32-row tile: the W2 and layer-1 fragments fill the
//     CU's 160 KB of LDS exactly; W3's fragments, b2 and b3 (7 KB) stream from L2, each requested one
//     out block of MFMAs ahead of its use.
// f32 path (parity, no speed claim): the unfolded formulas, f32 products and sums, 8 rows per
// 256-thread workgroup through LDS.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "swarm_mi355x.h"
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

typedef const __attribute__((address_space(4))) float* cfloat_p;  // constant address space: scalar loads

constexpr int EM = SWARM_ATTN_EMBED;    // 32
constexpr int KS1A = 4;                 // this trunk's layer-1 k-steps: [s 32 | own, obst, 1: <= 30, padded to 32]

// f32 front-end block of the bf16 blob (float offsets)
constexpr int FE_OWN_W = 0, FE_OWN_B = FE_OWN_W + EM * 9, FE_NB_W = FE_OWN_B + EM, FE_NB_B = FE_NB_W + EM * 4,
              FE_A = FE_NB_B + EM, FE_C0 = FE_A + EM * EM, FE_FLOATS = FE_C0 + EM;

// bf16 blob: [W2F 8x16 blocks][W3F 16 k-steps x 2*out lanes x 16 B][b2 256 f32][b3 32 f32][W1F 8x4
// blocks][front end FE_FLOATS f32]
struct Bf16Layout {
  size_t w2, w3, b2, b3, w1, fe, total;
  __host__ __device__ explicit Bf16Layout(int o) {
    w2 = 0;
    w3 = w2 + (size_t)OB * KS2 * FRAG;
    b2 = w3 + (size_t)KS2 * 2 * o * 16;
    b3 = b2 + H * 4;
    w1 = b3 + 32 * 4;
    fe = w1 + (size_t)OB * KS1A * FRAG;
    total = fe + (size_t)FE_FLOATS * 4;
  }
};
// f32 blob (float offsets): the unfolded parameters; W1 / W2 transposed ([k][unit]: a workgroup's
// 256 threads read one k-row coalesced)
struct F32Layout {
  int in1;
  size_t nbw, nbb, ownw, ownb, inw, inb, outw, outb, w1t, b1, w2t, b2, w3, b3, total;
  __host__ __device__ F32Layout(int ms, int o) {
    in1 = 9 + EM + 4 * ms;
    nbw = 0;
    nbb = nbw + EM * 4;
    ownw = nbb + EM;
    ownb = ownw + EM * 9;
    inw = ownb + EM;
    inb = inw + 3 * EM * EM;
    outw = inb + 3 * EM;
    outb = outw + EM * EM;
    w1t = outb + EM;
    b1 = w1t + (size_t)in1 * H;
    w2t = b1 + H;
    b2 = w2t + (size_t)H * H;
    w3 = b2 + H;
    b3 = w3 + (size_t)o * H;
    total = b3 + 16;
  }
};

// s component carried by layer-1 fragment column k < 32 (k-step k >> 4, lane half (k >> 3) & 1)
__host__ __device__ inline int s_of_col(int k) { return 16 * ((k >> 3) & 1) + 8 * (k >> 4) + (k & 7); }

__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }

__device__ __forceinline__ unsigned pack2(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}

struct FwdArgs {
  const void* w;        // packed blob (device)
  const float* obs;     // [rows, D]
  float* logits;        // [rows, out] or null
  float* actions;       // [rows, out/2] or null
  long long rows;
  int k, ms, out;
  uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

// ---------------------------------------------------------------- bf16 kernel
constexpr int LDS_W2 = 0;                    // LDS image: W2 fragments, then the layer-1 fragments
constexpr int LDS_W1 = OB * KS2 * FRAG;      // 131072
constexpr int LDS_BYTES = LDS_W1 + OB * KS1A * FRAG;  // 163840: the whole LDS of a CU

// The trunk over one 32-row tile: swarm_policy.hip's policy_mlp_bf16 (T = 1) with four layer-1
// k-steps.  W1 and W2 fragments come from LDS; what no longer fits there — W3's fragments, b2, b3,
// 7 KB of the blob `gw` — is requested from L2 at the top of the out block that uses it, a whole
// block of MFMAs (512 cycles) ahead of its use.  The biases are added after the products (the
// accumulators start at zero) so that their loads have that block to land in.
template <int MODE>
__device__ __forceinline__ void trunk_tile(const FwdArgs& A, const unsigned char* lds, const Bf16Layout& L,
                                           const unsigned char* gw, const bf16x8 (&xb)[KS1A], int lane, int out,
                                           long long row, bool valid) {
  const int n = lane & 31, h = (lane >> 5) & 1;
  const bool w3lane = n < out;
  const int w3idx = w3lane ? h * out + n : 0;
  const bf16x8* w1f = reinterpret_cast<const bf16x8*>(lds + LDS_W1 + 16u * (uint32_t)lane);
  const bf16x8* w2f = reinterpret_cast<const bf16x8*>(lds + LDS_W2 + 16u * (uint32_t)lane);
  const bf16x8* w3g = reinterpret_cast<const bf16x8*>(gw + L.w3);
  const float* b2 = reinterpret_cast<const float*>(gw + L.b2);
  const float* b3 = reinterpret_cast<const float*>(gw + L.b3);
  float b3v[8];  // this lane's logits biases (the blob holds 32 floats there: no index leaves it)
#pragma unroll
  for (int i = 0; i < 8; ++i) b3v[i] = b3[(i & 3) + 8 * (i >> 2) + 4 * h];
  // ---- layer 1: 256 x 64, relu -> h1 (16 k-step fragments)
  bf16x8 h1[KS2];
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    f32x16 acc = f32x16{};
#pragma unroll
    for (int ks = 0; ks < KS1A; ++ks)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[(ob * KS1A + ks) * 64], xb[ks], acc, 0, 0, 0);
    h1[2 * ob] = pack8(acc, 0, true);
    h1[2 * ob + 1] = pack8(acc, 1, true);
    __builtin_amdgcn_sched_barrier(0);  // keep each out block's fragment reads inside it
  }
  // ---- layer 2 (256 x 256, relu) fused with layer 3 (out x 256)
  f32x16 acc3 = f32x16{};
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    bf16x8 a0 = w3g[(2 * ob) * 2 * out + w3idx], a1 = w3g[(2 * ob + 1) * 2 * out + w3idx];
    float4 bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = *reinterpret_cast<const float4*>(b2 + ob * 32 + 8 * g + 4 * h);
    f32x16 acc = f32x16{};
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
      const bf16x8 w = w2f[(ob * KS2 + ks) * 64];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, h1[ks], acc, 0, 0, 0);
      if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // <= 8 fragments (32 VGPRs) in flight
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      acc[4 * g + 0] = acc[4 * g + 0] + bias[g].x; acc[4 * g + 1] = acc[4 * g + 1] + bias[g].y;
      acc[4 * g + 2] = acc[4 * g + 2] + bias[g].z; acc[4 * g + 3] = acc[4 * g + 3] + bias[g].w;
    }
    if (!w3lane) {
      a0 = bf16x8{};
      a1 = bf16x8{};
    }
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, pack8(acc, 0, true), acc3, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, pack8(acc, 1, true), acc3, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc3[i] = acc3[i] + b3v[i];
  // ---- outputs: lane holds logits m = (i&3) + 8(i>>2) + 4h of its row (out <= 12: i < 8)
  if (A.logits && valid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = (i & 3) + 8 * (i >> 2) + 4 * h;
      if (m < out) A.logits[row * out + m] = acc3[i];
    }
  }
  if (A.actions) {
    float lg[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lg[i] = acc3[i];
      lg[4 + i] = __shfl_xor(acc3[i], 32);
      lg[8 + i] = acc3[4 + i];
    }
    const int ad = out / 2;
    if (h == 0 && valid) {
      float z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (MODE == SWARM_POLICY_ACT_SAMPLE) normals(A, row, ad, z);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (k < ad) {
          float a = lg[k];
          if constexpr (MODE == SWARM_POLICY_ACT_SAMPLE) a = a + expf(lg[ad + k]) * z[k];
          A.actions[row * ad + k] = a;
        }
      }
    }
  }
}

// e_i = relu(b_nb[i] + W_nb[i] . nb) and the running score t . e, i over the 32 embed units
#define ATTN_EMBED_NB(i, e)                                     \
  float e = fej[FE_NB_B + (i)];                                 \
  e = __builtin_fmaf(fej[FE_NB_W + 4 * (i) + 0], nb0, e);       \
  e = __builtin_fmaf(fej[FE_NB_W + 4 * (i) + 1], nb1, e);       \
  e = __builtin_fmaf(fej[FE_NB_W + 4 * (i) + 2], nb2, e);       \
  e = __builtin_fmaf(fej[FE_NB_W + 4 * (i) + 3], nb3, e);       \
  e = relu(e);

template <int WAVES, int MODE>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WAVES / 4 > 0 ? WAVES / 4 : 1)))
attn_policy_bf16(const FwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const Bf16Layout L(A.out);
  {  // stage the LDS image (W2 and layer-1 fragments: 160 KB), once per workgroup
    const int4* src = reinterpret_cast<const int4*>(A.w);
    int4* dst = reinterpret_cast<int4*>(lds);
    constexpr int n16 = LDS_BYTES / 16, nw2 = LDS_W1 / 16;
    const int skip = (int)(L.w1 / 16) - nw2;  // the blob keeps W3, b2, b3 between the two
    constexpr int UNR = 8, STRIDE = 64 * WAVES;
    for (int base = threadIdx.x; base < n16; base += STRIDE * UNR) {
      int4 v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        int i = base + u * STRIDE;
        i = i < n16 ? i : n16 - 1;
        v[u] = src[i < nw2 ? i : i + skip];
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int i = base + u * STRIDE;
        if (i < n16) dst[i] = v[u];
      }
    }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const long long ngroups = (A.rows + 63) / 64;
  const cfloat_p fe = (cfloat_p)(uintptr_t)(reinterpret_cast<const unsigned char*>(A.w) + L.fe);
  for (long long grp = (long long)blockIdx.x * WAVES + wave; grp < ngroups; grp += (long long)gridDim.x * WAVES) {
    // opaque per group, as in policy_mlp_bf16: nothing derived from these is hoisted out of the loop
    int lane = threadIdx.x & 63, k_r = A.k, ms_r = A.ms, out = A.out;
    asm volatile("" : "+v"(lane), "+s"(k_r), "+s"(ms_r), "+s"(out));
    const int D = 9 + 4 * k_r + 4 * ms_r;
    // ================= front end: lane l, row 64 grp + l (clamped: a tail lane repeats the last row)
    const long long frow = grp * 64 + lane;
    const float* xr = A.obs + (frow < A.rows ? frow : A.rows - 1) * D;
    unsigned s_pk[16];   // bf16 pairs (s[2q], s[2q+1])
    unsigned tl_pk[16];  // bf16 pairs of the tail [own | obst | 1 | 0...]
    {
      float tl[32];
#pragma unroll
      for (int c = 0; c < 9; ++c) tl[c] = xr[c];
      const int no = 4 * ms_r;
#pragma unroll
      for (int c = 0; c < 4 * SWARM_ATTN_MAX_MS + 1; ++c) {
        const float v = xr[c < no ? 9 + 4 * k_r + c : 0];  // unconditional load from inside the row
        tl[9 + c] = c < no ? v : (c == no ? 1.f : 0.f);
      }
      tl[30] = 0.f;
      tl[31] = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) tl_pk[q] = pack2(tl[2 * q], tl[2 * q + 1]);
      // t = A o + c0,  o = relu(W_own own + b_own)
      float t[EM];
      {
        float o[EM];
#pragma unroll
        for (int m = 0; m < EM; ++m) {
          float acc = fe[FE_OWN_B + m];
#pragma unroll
          for (int c = 0; c < 9; ++c) acc = __builtin_fmaf(fe[FE_OWN_W + 9 * m + c], tl[c], acc);
          o[m] = relu(acc);
        }
#pragma unroll
        for (int i = 0; i < EM; ++i) {
          float acc = fe[FE_C0 + i];
#pragma unroll
          for (int m = 0; m < EM; ++m) acc = __builtin_fmaf(fe[FE_A + EM * i + m], o[m], acc);
          t[i] = acc;
        }
      }
      // One pass over the neighbours with the running row maximum subtracted (no exp argument is
      // ever positive): p_j = exp(score_j - max), s = sum_j p_j e_j / sum_j p_j; when the maximum
      // rises, what was accumulated under the old one is scaled by exp(old - new).  A second pass
      // under the final maximum would compute every e_j twice (160 of its ~350 FMAs per neighbour).
      float s[EM];
#pragma unroll
      for (int i = 0; i < EM; ++i) s[i] = 0.f;
      float den = 0.f, mx = -INFINITY;
#pragma unroll 1
      for (int j = 0; j < k_r; ++j) {
        cfloat_p fej = fe;  // opaque per neighbour: the 160 embed weights are reloaded, not held in SGPRs
        asm volatile("" : "+s"(fej));
        const float nb0 = xr[9 + 4 * j], nb1 = xr[10 + 4 * j], nb2 = xr[11 + 4 * j], nb3 = xr[12 + 4 * j];
        float ej[EM];
        float sc = 0.f;
#pragma unroll
        for (int i = 0; i < EM; ++i) {
          ATTN_EMBED_NB(i, e)
          ej[i] = e;
          sc = __builtin_fmaf(t[i], e, sc);
        }
        const float mn = fmaxf(mx, sc);
        const float corr = expf(mx - mn);  // exp(-inf) = 0 on the first neighbour
        const float p = expf(sc - mn);
        mx = mn;
        den = __builtin_fmaf(den, corr, p);
#pragma unroll
        for (int i = 0; i < EM; ++i) s[i] = __builtin_fmaf(p, ej[i], s[i] * corr);
      }
      const float inv = 1.f / den;
#pragma unroll
      for (int q = 0; q < 16; ++q) s_pk[q] = pack2(s[2 * q] * inv, s[2 * q + 1] * inv);
    }
    // ================= hand-over: lane l holds row l whole; tile u's lane (n, h) needs row 32 u + n's
    // half-h columns.  permlane32_swap(a, b) exchanges lanes 32-63 of a with lanes 0-31 of b: with
    // a = the half-0 dword and b = the half-1 dword, a becomes tile 0's fragment dword (lanes 0-31
    // their own half 0, lanes 32-63 row n's half 1) and b tile 1's.
    bf16x8 xb[2][KS1A];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 f0, f1, g0, g1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // s: half h of k-step ks is s[16 h + 8 ks ..+7] = pairs 8 h + 4 ks + q
        const auto r = __builtin_amdgcn_permlane32_swap(s_pk[4 * ks + q], s_pk[8 + 4 * ks + q], false, false);
        f0[q] = r[0];
        f1[q] = r[1];
        // tail: half h of k-step 2 + ks is tail[16 ks + 8 h ..+7] = pairs 8 ks + 4 h + q
        const auto r2 = __builtin_amdgcn_permlane32_swap(tl_pk[8 * ks + q], tl_pk[8 * ks + 4 + q], false, false);
        g0[q] = r2[0];
        g1[q] = r2[1];
      }
      xb[0][ks] = __builtin_bit_cast(bf16x8, f0);
      xb[1][ks] = __builtin_bit_cast(bf16x8, f1);
      xb[0][2 + ks] = __builtin_bit_cast(bf16x8, g0);
      xb[1][2 + ks] = __builtin_bit_cast(bf16x8, g1);
    }
    // ================= trunk, one 32-row tile at a time
    const unsigned char* gw = reinterpret_cast<const unsigned char*>(A.w);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long long base = grp * 64 + 32 * u;
      if (base < A.rows) {  // wave-uniform
        // opaque per tile: the two inlined trunks share no fragment address (held across a whole
        // trunk next to h1 they spill)
        int tl_lane = lane, tl_out = out;
        asm volatile("" : "+v"(tl_lane), "+s"(tl_out));
        const long long row = base + (tl_lane & 31);
        trunk_tile<MODE>(A, lds, L, gw, xb[u], tl_lane, tl_out, row, row < A.rows);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ---------------------------------------------------------------- f32 kernel (parity path)
constexpr int RB = 8;  // rows per workgroup iteration: thread (r, i) = (tid >> 5, tid & 31) in the front end

template <int MODE>
__global__ void __launch_bounds__(256) attn_policy_f32(const FwdArgs A) {
  __shared__ float s_e[RB * 16 * EM], s_k[RB * 16 * EM], s_v[RB * 16 * EM];
  __shared__ float s_o[RB * EM], s_q[RB * EM], s_ctx[RB * EM], s_sc[RB * 16], s_x[RB * 64], s_lg[RB * 16];
  float* const s_h1 = s_e;  // the trunk's activations reuse the front end's buffers
  float* const s_h2 = s_k;
  const F32Layout L(A.ms, A.out);
  const float* W = reinterpret_cast<const float*>(A.w);
  const int tid = threadIdx.x, r = tid >> 5, i = tid & 31;
  const int K = A.k, out = A.out, ad = A.out / 2, in1 = L.in1;
  const int D = 9 + 4 * K + 4 * A.ms;
  const long long nblk = (A.rows + RB - 1) / RB;
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long long row = blk * RB + r;
    const float* xr = A.obs + (row < A.rows ? row : A.rows - 1) * D;
    {  // embeds; the trunk input's own and obstacle columns
      float acc = W[L.ownb + i];
      for (int c = 0; c < 9; ++c) acc = acc + W[L.ownw + i * 9 + c] * xr[c];
      s_o[r * EM + i] = relu(acc);
      for (int j = 0; j < K; ++j) {
        float a = W[L.nbb + i];
        for (int c = 0; c < 4; ++c) a = a + W[L.nbw + i * 4 + c] * xr[9 + 4 * j + c];
        s_e[(r * 16 + j) * EM + i] = relu(a);
      }
      for (int c = i; c < 64; c += 32) {
        float v = 0.f;
        if (c < 9) v = xr[c];
        else if (c >= 9 + EM && c < in1) v = xr[9 + 4 * K + (c - 9 - EM)];
        s_x[r * 64 + c] = v;
      }
    }
    __syncthreads();
    {  // q, k_j, v_j
      float q = W[L.inb + i];
      for (int m = 0; m < EM; ++m) q = q + W[L.inw + i * EM + m] * s_o[r * EM + m];
      s_q[r * EM + i] = q;
      for (int j = 0; j < K; ++j) {
        float ak = W[L.inb + EM + i], av = W[L.inb + 2 * EM + i];
        for (int m = 0; m < EM; ++m) {
          const float em = s_e[(r * 16 + j) * EM + m];
          ak = ak + W[L.inw + (EM + i) * EM + m] * em;
          av = av + W[L.inw + (2 * EM + i) * EM + m] * em;
        }
        s_k[(r * 16 + j) * EM + i] = ak;
        s_v[(r * 16 + j) * EM + i] = av;
      }
    }
    __syncthreads();
    if (i < K) {  // scores
      float acc = 0.f;
      for (int m = 0; m < EM; ++m) acc = acc + s_q[r * EM + m] * s_k[(r * 16 + i) * EM + m];
      s_sc[r * 16 + i] = acc * 0.17677669529663687f;  // 1 / sqrt(32)
    }
    __syncthreads();
    {  // softmax (row maximum subtracted) and the context
      float mx = -INFINITY;
      for (int j = 0; j < K; ++j) mx = fmaxf(mx, s_sc[r * 16 + j]);
      float den = 0.f, c = 0.f;
      for (int j = 0; j < K; ++j) {
        const float p = expf(s_sc[r * 16 + j] - mx);
        den = den + p;
        c = c + p * s_v[(r * 16 + j) * EM + i];
      }
      s_ctx[r * EM + i] = c / den;
    }
    __syncthreads();
    {  // out projection -> the trunk input's context columns
      float acc = W[L.outb + i];
      for (int m = 0; m < EM; ++m) acc = acc + W[L.outw + i * EM + m] * s_ctx[r * EM + m];
      s_x[r * 64 + 9 + i] = acc;
    }
    __syncthreads();
    {  // layer 1: thread = hidden unit
      float acc[RB];
      const float b = W[L.b1 + tid];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) acc[rr] = b;
      for (int k = 0; k < in1; ++k) {
        const float w = W[L.w1t + (size_t)k * H + tid];
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) acc[rr] = acc[rr] + w * s_x[rr * 64 + k];
      }
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) s_h1[rr * H + tid] = relu(acc[rr]);
    }
    __syncthreads();
    {  // layer 2
      float acc[RB];
      const float b = W[L.b2 + tid];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) acc[rr] = b;
      for (int k = 0; k < H; ++k) {
        const float w = W[L.w2t + (size_t)k * H + tid];
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) acc[rr] = acc[rr] + w * s_h1[rr * H + k];
      }
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) s_h2[rr * H + tid] = relu(acc[rr]);
    }
    __syncthreads();
    if (tid < RB * out) {  // layer 3
      const int rr = tid / out, m = tid - rr * out;
      float acc = W[L.b3 + m];
      for (int k = 0; k < H; ++k) acc = acc + W[L.w3 + (size_t)m * H + k] * s_h2[rr * H + k];
      s_lg[rr * 16 + m] = acc;
      const long long orow = blk * RB + rr;
      if (A.logits && orow < A.rows) A.logits[orow * out + m] = acc;
    }
    __syncthreads();
    if (A.actions && tid < RB * ad) {
      const int rr = tid / ad, k = tid - rr * ad;
      const long long orow = blk * RB + rr;
      if (orow < A.rows) {
        float a = s_lg[rr * 16 + k];
        if constexpr (MODE == SWARM_POLICY_ACT_SAMPLE) {
          float z[6];
          normals(A, orow, ad, z);
          float zk = z[0];
#pragma unroll
          for (int q = 1; q < 6; ++q) zk = k == q ? z[q] : zk;
          a = a + expf(s_lg[rr * 16 + ad + k]) * zk;
        }
        A.actions[orow * ad + k] = a;
      }
    }
    __syncthreads();
  }
}

constexpr int BF16_WAVES = 8;  // one workgroup per CU (the LDS image), two waves per SIMD

thread_local UnitError g_err;

int check_dims(int k, int ms, int out_dim, int precision) {
  if (k < 1 || k > SWARM_ATTN_MAX_K)
    return g_err.fail(SWARM_ELIMIT, "neighbor_k out of range: the attention actor takes 1..16 neighbour slots (SWARM_ATTN_MAX_K)");
  if (ms < 0 || ms > SWARM_ATTN_MAX_MS)
    return g_err.fail(SWARM_ELIMIT, "sensed_obstacles out of range: the attention actor takes 0..5 (SWARM_ATTN_MAX_MS)");
  if (out_dim < 2 || out_dim > SWARM_POLICY_MAX_OUT || (out_dim & 1))
    return g_err.fail(SWARM_ELIMIT, "out_dim must be even, 2..12 (SWARM_POLICY_MAX_OUT)");
  if (precision == SWARM_POLICY_F32X3)
    return g_err.fail(SWARM_ELIMIT, "the attention actor has no f32x3 path: SWARM_POLICY_BF16 or SWARM_POLICY_F32");
  if (precision != SWARM_POLICY_BF16 && precision != SWARM_POLICY_F32) return g_err.fail(SWARM_EINVAL, "unknown precision");
  return SWARM_OK;
}

}  // namespace

extern "C" {

const char* swarm_attn_policy_last_error(void) { return g_err.msg; }

long long swarm_attn_policy_packed_bytes(int neighbor_k, int sensed_obstacles, int out_dim, int precision) {
  const int rc = check_dims(neighbor_k, sensed_obstacles, out_dim, precision);
  if (rc != SWARM_OK) return rc;
  if (precision == SWARM_POLICY_BF16) return (long long)Bf16Layout(out_dim).total;
  return (long long)F32Layout(sensed_obstacles, out_dim).total * 4;
}

int swarm_attn_policy_pack(int neighbor_k, int sensed_obstacles, int out_dim, int precision,
                           const swarm_attn_weights_t* w, void* host_out) {
  const long long nb = swarm_attn_policy_packed_bytes(neighbor_k, sensed_obstacles, out_dim, precision);
  if (nb < 0) return (int)nb;
  if (!w || !host_out) return g_err.fail(SWARM_ENULL, "null weights / output pointer");
  if (!w->neighbor_w || !w->neighbor_b || !w->own_w || !w->own_b || !w->in_proj_w || !w->in_proj_b ||
      !w->out_proj_w || !w->out_proj_b || !w->w1 || !w->b1 || !w->w2 || !w->b2 || !w->w3 || !w->b3)
    return g_err.fail(SWARM_ENULL, "null weight pointer");
  memset(host_out, 0, (size_t)nb);
  const int ms = sensed_obstacles, in1 = 9 + EM + 4 * ms;
  if (precision == SWARM_POLICY_F32) {
    const F32Layout L(ms, out_dim);
    float* f = static_cast<float*>(host_out);
    memcpy(f + L.nbw, w->neighbor_w, EM * 4 * 4);
    memcpy(f + L.nbb, w->neighbor_b, EM * 4);
    memcpy(f + L.ownw, w->own_w, EM * 9 * 4);
    memcpy(f + L.ownb, w->own_b, EM * 4);
    memcpy(f + L.inw, w->in_proj_w, 3 * EM * EM * 4);
    memcpy(f + L.inb, w->in_proj_b, 3 * EM * 4);
    memcpy(f + L.outw, w->out_proj_w, EM * EM * 4);
    memcpy(f + L.outb, w->out_proj_b, EM * 4);
    for (int k = 0; k < in1; ++k)
      for (int m = 0; m < H; ++m) f[L.w1t + (size_t)k * H + m] = w->w1[(size_t)m * in1 + k];
    memcpy(f + L.b1, w->b1, H * 4);
    for (int k = 0; k < H; ++k)
      for (int m = 0; m < H; ++m) f[L.w2t + (size_t)k * H + m] = w->w2[(size_t)m * H + k];
    memcpy(f + L.b2, w->b2, H * 4);
    memcpy(f + L.w3, w->w3, (size_t)out_dim * H * 4);
    memcpy(f + L.b3, w->b3, (size_t)out_dim * 4);
    return SWARM_OK;
  }
  const Bf16Layout L(out_dim);
  unsigned char* base = static_cast<unsigned char*>(host_out);
  // ---- the folds, in double
  const float *wq = w->in_proj_w, *wk = w->in_proj_w + EM * EM, *wv = w->in_proj_w + 2 * EM * EM;
  const float *bq = w->in_proj_b, *bv = w->in_proj_b + 2 * EM;
  const double scale = 1.0 / sqrt((double)EM);
  float* fe = reinterpret_cast<float*>(base + L.fe);
  memcpy(fe + FE_OWN_W, w->own_w, EM * 9 * 4);
  memcpy(fe + FE_OWN_B, w->own_b, EM * 4);
  memcpy(fe + FE_NB_W, w->neighbor_w, EM * 4 * 4);
  memcpy(fe + FE_NB_B, w->neighbor_b, EM * 4);
  for (int i = 0; i < EM; ++i) {  // A = Wk^T Wq / sqrt(32), c0 = Wk^T bq / sqrt(32)
    for (int m = 0; m < EM; ++m) {
      double a = 0.0;
      for (int r = 0; r < EM; ++r) a += (double)wk[r * EM + i] * (double)wq[r * EM + m];
      fe[FE_A + i * EM + m] = (float)(a * scale);
    }
    double c = 0.0;
    for (int r = 0; r < EM; ++r) c += (double)wk[r * EM + i] * (double)bq[r];
    fe[FE_C0 + i] = (float)(c * scale);
  }
  double mv[EM][EM], uv[EM];  // Wout Wv, Wout bv + bout
  for (int a = 0; a < EM; ++a) {
    for (int b = 0; b < EM; ++b) {
      double x = 0.0;
      for (int r = 0; r < EM; ++r) x += (double)w->out_proj_w[a * EM + r] * (double)wv[r * EM + b];
      mv[a][b] = x;
    }
    double x = (double)w->out_proj_b[a];
    for (int r = 0; r < EM; ++r) x += (double)w->out_proj_w[a * EM + r] * (double)bv[r];
    uv[a] = x;
  }
  // ---- layer 1: row m of [F | W1 own | W1 obst | b1 + d | 0], F's columns in fragment order
  uint16_t* w1f = reinterpret_cast<uint16_t*>(base + L.w1);
  for (int m = 0; m < H; ++m) {
    const float* w1r = w->w1 + (size_t)m * in1;
    float rowv[64];
    for (int k = 0; k < 32; ++k) {
      const int b = s_of_col(k);
      double x = 0.0;
      for (int a = 0; a < EM; ++a) x += (double)w1r[9 + a] * mv[a][b];
      rowv[k] = (float)x;
    }
    for (int t = 0; t < 32; ++t) {
      float v = 0.f;
      if (t < 9) v = w1r[t];
      else if (t < 9 + 4 * ms) v = w1r[9 + EM + (t - 9)];
      else if (t == 9 + 4 * ms) {
        double x = (double)w->b1[m];
        for (int a = 0; a < EM; ++a) x += (double)w1r[9 + a] * uv[a];
        v = (float)x;
      }
      rowv[32 + t] = v;
    }
    for (int k = 0; k < 64; ++k)  // natural k: k-step k >> 4, lane half (k >> 3) & 1, element k & 7
      w1f[(size_t)frag_slot((m >> 5) * KS1A + (k >> 4), m & 31, (k >> 3) & 1) * 8 + (k & 7)] = bf16_rne(rowv[k]);
  }
  pack_w2f(base + L.w2, w->w2, ToBf16());  // the trunk's tail: the actor's W2F and W3F
  pack_w3f(base + L.w3, w->w3, out_dim, ToBf16());
  memcpy(base + L.b2, w->b2, H * 4);
  memcpy(base + L.b3, w->b3, (size_t)out_dim * 4);
  return SWARM_OK;
}

int swarm_attn_policy_forward(const swarm_attn_policy_t* p, const float* obs, long long rows, float* logits,
                              float* actions, int action_mode, unsigned long long seed, unsigned long long counter,
                              void* hip_stream) {
  if (!p || !p->weights) return g_err.fail(SWARM_ENULL, "policy/weights is NULL");
  const int rc = check_dims(p->neighbor_k, p->sensed_obstacles, p->out_dim, p->precision);
  if (rc != SWARM_OK) return rc;
  if (rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (rows == 0) return SWARM_OK;
  if (!obs) return g_err.fail(SWARM_ENULL, "obs is NULL");
  if (!logits && !actions) return g_err.fail(SWARM_ENULL, "need logits and/or actions");
  if (action_mode != SWARM_POLICY_ACT_MEAN && action_mode != SWARM_POLICY_ACT_SAMPLE)
    return g_err.fail(SWARM_EINVAL, "unknown action_mode");
  if (((uintptr_t)p->weights) % 16) return g_err.fail(SWARM_EINVAL, "weights must be 16-B aligned");
  FwdArgs a;
  a.w = p->weights;
  a.obs = obs;
  a.logits = logits;
  a.actions = actions;
  a.rows = rows;
  a.k = p->neighbor_k;
  a.ms = p->sensed_obstacles;
  a.out = p->out_dim;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.ctr_lo = (uint32_t)counter;
  a.ctr_hi = (uint32_t)(counter >> 32);
  hipStream_t s = (hipStream_t)hip_stream;
  const bool sample = action_mode == SWARM_POLICY_ACT_SAMPLE;
  if (p->precision == SWARM_POLICY_BF16) {
    const int lds = LDS_BYTES;
    auto fn = sample ? attn_policy_bf16<BF16_WAVES, SWARM_POLICY_ACT_SAMPLE>
                     : attn_policy_bf16<BF16_WAVES, SWARM_POLICY_ACT_MEAN>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
        hipSuccess)
      return g_err.fail(SWARM_EHIP, "hipFuncSetAttribute failed");
    const int grid = grid_for(((rows + 63) / 64 + BF16_WAVES - 1) / BF16_WAVES, 1);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * BF16_WAVES), lds, s, a);
  } else {
    auto fn = sample ? attn_policy_f32<SWARM_POLICY_ACT_SAMPLE> : attn_policy_f32<SWARM_POLICY_ACT_MEAN>;
    const int grid = grid_for((rows + RB - 1) / RB, 4);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, s, a);
  }
  return g_err.launch_status();
}

}  // extern "C"
