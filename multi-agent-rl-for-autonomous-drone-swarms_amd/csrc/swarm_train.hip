// swarm_train.hip — training the bf16 actor on the device (gfx950, MFMA): the backward of
// swarm_policy.hip's bf16 MLP, its weight gradients, and a device packer that turns the float32
// master weights back into the inference blob.  The arithmetic is written out in
// include/swarm_mi355x.h; this file says how it is laid out.  The blob's layout (ActorLayout) and
// the rules for its fragment elements are swarm_nn.h's, the ones swarm_policy_pack loops over: the
// packer here only maps a thread to a slot.  The transposed W2^T / W3^T fragments of the workspace
// have no other user and are defined here.
//
// Five simple launches per swarm_policy_backward, all async on one stream, no atomics, no grid that
// depends on the device:
//
//  (a) train_fwd_dz2   one wave per 32-row tile, W1 / W2 fragments and b2 staged in LDS exactly as
//      policy_mlp_bf16 stages them.  It recomputes h1 and h2 with that kernel's instruction sequence
//      (the same fragments, the same MFMA order, pack8's relu after the rounding), so the relu masks
//      are those of the logits the loss saw.  dz2 = (W3^T bf16(g)) [h2 > 0] is one MFMA per out
//      block: the eight W3^T fragments (K = 16 >= 2A, natural k order) sit in 32 VGPRs.
//  (b) train_dz1       one wave per tile, W1 and W2^T fragments in LDS: layer 1 again for the h1
//      mask (3 MFMAs per out block, bit for bit the h1 of (a)), then dz1 = (W2^T dz2) [h1 > 0],
//      16 MFMAs per block with dz2 read row-major as natural-k B fragments.
//  (c) train_wgrad x3  the sums over rows.  Every tensor a weight gradient reads (bf16 x with the 1
//      in column D, bf16 g, h1, h2, dz2, dz1) is also stored UNIT-MAJOR [unit][row] by (a) and (b),
//      so both operands of C[m][n] = sum_r A[m][r] B[n][r] are 16 contiguous bytes per lane in the
//      same k order: no LDS, no transpose read, no barrier.  One
//      workgroup per slab of TRAIN_SLAB rows, one wave per block of output tiles, f32 partials per
//      slab in the workspace.  The bias gradients are one more MFMA per k-step against an all-ones
//      B fragment (db2, db3) or the 1 in column D of x (db1).
//  (d) train_finalise  one thread per gradient element adds the slabs' partials in index order.
//
// Rows past `rows` (the row count is padded to a multiple of 32) are computed from a clamped obs
// row with g = 0, so every dz of theirs is exactly 0 and they add exactly 0 to every sum.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "swarm_mi355x.h"
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

constexpr int XU = 64;         // unit-major rows of x (two 32-blocks: columns 0..D-1, the 1, zeros)
constexpr int GU = 32;         // unit-major rows of g (one 32-block: 2A columns, zeros)
constexpr int TRAIN_WAVES = 8;       // waves per workgroup of (a) and (b): one workgroup per CU (the LDS blob)
constexpr int TRAIN_MAX_BLOCKS = SWARM_TRAIN_MAX_BLOCKS;  // grid cap of (a) and (b): a constant, not the CU count
constexpr int SLAB = SWARM_TRAIN_SLAB;                    // rows per weight-gradient slab
constexpr size_t W1F_BYTES = (size_t)OB * KS1 * FRAG;     // 24,576
constexpr size_t W2F_BYTES = (size_t)OB * KS2 * FRAG;     // 131,072
constexpr size_t W3T_BYTES = (size_t)OB * FRAG;           // 8,192
constexpr int PART_FLOATS = H * H + H + GU * H + GU + H * XU;  // one slab's partials: P2, PB2, P3, PB3, P1

// the training workspace (bytes): the transposed fragment blobs the packer writes, the per-row
// stage tensors of one backward (ld = rows rounded up to 32), the slabs' partial sums
struct TrainLayout {
  size_t ld, nslabs;
  size_t w2t, w3t, xT, gT, h1T, h2T, dz2T, dz1T, dz2, part, total;
  __host__ __device__ explicit TrainLayout(long long rows) {
    ld = ((size_t)rows + 31) / 32 * 32;
    nslabs = (ld + SLAB - 1) / SLAB;
    w2t = 0;
    w3t = w2t + W2F_BYTES;
    xT = w3t + W3T_BYTES;
    gT = xT + (size_t)XU * ld * 2;
    h1T = gT + (size_t)GU * ld * 2;
    h2T = h1T + (size_t)H * ld * 2;
    dz2T = h2T + (size_t)H * ld * 2;
    dz1T = dz2T + (size_t)H * ld * 2;
    dz2 = dz1T + (size_t)H * ld * 2;
    part = dz2 + (size_t)H * ld * 2;
    total = part + nslabs * (size_t)PART_FLOATS * 4;
  }
};

// ---------------------------------------------------------------- device packer
struct PackArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  unsigned char* blob;
  unsigned char* ws;
  int in, out;
};

// one thread per 16-byte slot (8 bf16 or 4 f32) of the blob, then of W2^T and W3^T
__global__ void __launch_bounds__(256) train_pack(const PackArgs A) {
  const ActorLayout L(A.out);
  const TrainLayout T(0);
  const int nblob = (int)(L.total / 16);
  const int nw2t = (int)(W2F_BYTES / 16), nw3t = (int)(W3T_BYTES / 16);
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nblob + nw2t + nw3t) return;
  uint16_t e[8];
  uint4 v;
  unsigned char* dst;
  if (slot < nblob) {
    dst = A.blob + (size_t)slot * 16;
    const size_t off = (size_t)slot * 16;
    if (off >= L.b2) {  // b2 [256] f32, then b3 [32] f32 with zeros past `out`
      const int f0 = (int)((off - L.b2) / 4);
      float f[4];
      for (int i = 0; i < 4; ++i) {
        const int k = f0 + i;
        f[i] = k < H ? A.b2[k] : (k - H < A.out ? A.b3[k - H] : 0.f);
      }
      v = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
      *reinterpret_cast<uint4*>(dst) = v;
      return;
    }
    // the blob's fragments: swarm_nn.h's slots and element rules, as the host packers
    if (off >= L.w3) {
      const W3Slot f = w3f_slot_of(A.out, (int)((off - L.w3) / 16));
      chained_slot(e, A.w3, f.m, f.ks, f.h, ToBf16());
    } else if (off >= L.w2) {  // W2F: block ob KS2 + ks
      const FragSlot f = frag_slot_of((int)((off - L.w2) / 16));
      chained_slot(e, A.w2, f.blk / KS2 * 32 + f.n, f.blk % KS2, f.h, ToBf16());
    } else {  // W1F: block ob KS1 + ks
      const FragSlot f = frag_slot_of(slot);
      l1_slot(e, A.w1, A.b1, A.in, f.blk / KS1 * 32 + f.n, f.blk % KS1, f.h, ToBf16());
    }
  } else if (slot < nblob + nw2t) {  // W2^T fragments: block (ib, ks), lane l: W2[16 ks + 8 h + j][32 ib + (l & 31)]
    const FragSlot f = frag_slot_of(slot - nblob);
    dst = A.ws + T.w2t + (size_t)(slot - nblob) * 16;
    const int i = f.blk / KS2 * 32 + f.n, ks = f.blk % KS2;
    for (int j = 0; j < 8; ++j) e[j] = bf16_rne(A.w2[(16 * ks + 8 * f.h + j) * H + i]);
  } else {  // W3^T fragments: block ob, lane l: W3[8 h + j][32 ob + (l & 31)], zero past `out`
    const FragSlot f = frag_slot_of(slot - nblob - nw2t);
    dst = A.ws + T.w3t + (size_t)(slot - nblob - nw2t) * 16;
    const int u = f.blk * 32 + f.n;
    for (int j = 0; j < 8; ++j) {
      const int m = 8 * f.h + j;
      e[j] = m < A.out ? bf16_rne(A.w3[m * H + u]) : (uint16_t)0;
    }
  }
  v = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16),
                 e[6] | ((uint32_t)e[7] << 16));
  *reinterpret_cast<uint4*>(dst) = v;
}

// ---------------------------------------------------------------- stages (a) and (b)
struct BwdArgs {
  const unsigned char* blob;  // the inference blob
  const float* obs;           // [rows, in]
  const float* g;             // [rows, out]
  unsigned char* ws;
  uint16_t *h1, *h2, *dz2, *dz1;  // optional [rows, 256] row-major stage outputs
  long long rows;
  int in, out;
};

// the 16-bit halves of `d` whose half of `hb` (a relu'd bf16 pair: never negative) is > 0
__device__ __forceinline__ uint32_t mask_pair(uint32_t d, uint32_t hb) {
  const uint32_t lo = (hb & 0xffffu) ? 0xffffu : 0u;
  const uint32_t hi = (hb >> 16) ? 0xffff0000u : 0u;
  return d & (lo | hi);
}

// Where a lane of the tile at rows [t32, t32 + 32) stores: every address is a wave-uniform base
// (SGPRs: the tensor, the unit's row, the tile) plus one of two 32-bit lane offsets plus a constant,
// so the ~600 distinct addresses of a tile cost scalar arithmetic and no vector registers.
struct LanePos {
  size_t ld, t32;     // uniform
  uint32_t um_off;    // 4 h ld + n: elements into [unit][pos] from (unit without its 4 h term, t32)
  uint32_t rm_off;    // n 256 + 4 h: elements into [row][unit] from (t32, unit without its 4 h term)
};

// sub-block s of out block ob (accumulator registers 8s .. 8s+7, packed): unit-major [unit][pos]
// always; row-major [row][unit] into `rm` (uniform, may be NULL) for the lanes with `rm_ok`
__device__ __forceinline__ void store_sub(uint16_t* um, uint16_t* rm, bool rm_ok, const LanePos& P, int ob, int s,
                                          const u32x4& w) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int unit = 32 * ob + 16 * s + 8 * (j >> 2) + (j & 3);  // + 4 h: in um_off
    (um + ((size_t)unit * P.ld + P.t32))[P.um_off] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
  }
  if (rm && rm_ok) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      *reinterpret_cast<uint2*>(rm + (P.t32 * H + 32 * ob + 16 * s + 8 * q) + P.rm_off) = make_uint2(w[2 * q], w[2 * q + 1]);
  }
}

// obs fragments (B of layer 1) of lane (n, h): policy_mlp_bf16's loads and selects
__device__ __forceinline__ void load_obs(const float* xr, int in, int h, bf16x8 (&xb)[KS1]) {
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

// copy n16 16-byte words into LDS, the whole workgroup
__device__ __forceinline__ void stage(int4* dst, const int4* src, int n16) {
  for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
}

__global__ void __launch_bounds__(64 * TRAIN_WAVES) __attribute__((amdgpu_waves_per_eu(2)))
train_fwd_dz2(const BwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const ActorLayout L(A.out);
  const TrainLayout T(A.rows);
  stage(reinterpret_cast<int4*>(lds), reinterpret_cast<const int4*>(A.blob), (int)((W1F_BYTES + W2F_BYTES) / 16));
  stage(reinterpret_cast<int4*>(lds + W1F_BYTES + W2F_BYTES), reinterpret_cast<const int4*>(A.blob + L.b2), H * 4 / 16);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int n = lane & 31, h = lane >> 5;
  const int in = A.in, out = A.out;
  const long long ntiles = (long long)(T.ld / 32);
  const bf16x8* w1f = reinterpret_cast<const bf16x8*>(lds + 16 * lane);
  const bf16x8* w2f = reinterpret_cast<const bf16x8*>(lds + W1F_BYTES + 16 * lane);
  const float* b2 = reinterpret_cast<const float*>(lds + W1F_BYTES + W2F_BYTES);
  uint16_t* xT = reinterpret_cast<uint16_t*>(A.ws + T.xT);
  uint16_t* gT = reinterpret_cast<uint16_t*>(A.ws + T.gT);
  uint16_t* h1T = reinterpret_cast<uint16_t*>(A.ws + T.h1T);
  uint16_t* h2T = reinterpret_cast<uint16_t*>(A.ws + T.h2T);
  uint16_t* dz2T = reinterpret_cast<uint16_t*>(A.ws + T.dz2T);
  uint16_t* dz2W = reinterpret_cast<uint16_t*>(A.ws + T.dz2);
  bf16x8 w3t[OB];
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) w3t[ob] = reinterpret_cast<const bf16x8*>(A.ws + T.w3t)[ob * 64 + lane];
  for (long long tile = (long long)blockIdx.x * TRAIN_WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * TRAIN_WAVES) {
    // opaque per tile: the row stride, so that the unit rows' addresses are scalar arithmetic redone
    // per tile instead of ~600 values hoisted out of the loop and kept live
    size_t ld = T.ld;
    asm volatile("" : "+s"(ld));
    LanePos P;
    P.ld = ld;
    P.t32 = (size_t)tile * 32;
    P.um_off = (uint32_t)(4 * h * ld + n);
    P.rm_off = (uint32_t)(n * H + 4 * h);
    const long long row = tile * 32 + n;  // < ld
    const bool valid = row < A.rows;
    const long long rc = valid ? row : A.rows - 1;
    bf16x8 xb[KS1];
    load_obs(A.obs + rc * in, in, h, xb);
    // g fragment (B of the W3^T product): bf16(g[row][8h + j]), zero past `out` and on rows past the end
    bf16x8 gb;
    {
      float gv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = 8 * h + j;
        gv[j] = A.g[rc * out + (m < out ? m : out - 1)];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) gb[j] = (__bf16)((valid && 8 * h + j < out) ? gv[j] : 0.f);
    }
    // unit-major bf16 x (with the 1 in column `in`) and g for the weight gradients
    const uint32_t xoff = (uint32_t)(8 * h * ld + n);  // rows 8 h + .. of a 16-row group, this lane's position
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
      // element j is half j & 1 of word j >> 1 (a bit_cast of the single __bf16 element xb[ks][j] to
      // uint16_t stored element 0 for every j: the exact-integer test)
      const u32x4 xw = __builtin_bit_cast(u32x4, xb[ks]);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        (xT + ((size_t)(16 * ks + j) * ld + P.t32))[xoff] = (uint16_t)(xw[j >> 1] >> (16 * (j & 1)));
    }
    const u32x4 gw = __builtin_bit_cast(u32x4, gb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      (xT + ((size_t)(KP1 + j) * ld + P.t32))[xoff] = 0;
      (gT + ((size_t)j * ld + P.t32))[xoff] = (uint16_t)(gw[j >> 1] >> (16 * (j & 1)));
      (gT + ((size_t)(16 + j) * ld + P.t32))[xoff] = 0;
    }
    // ---- layer 1 (policy_mlp_bf16's sequence)
    bf16x8 h1[KS2];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      f32x16 acc = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[(ob * KS1 + ks) * 64], xb[ks], acc, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32x4 w = pack8_u32(acc, s, true);
        h1[2 * ob + s] = __builtin_bit_cast(bf16x8, w);
        store_sub(h1T, A.h1, valid, P, ob, s, w);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- layer 2 and dz2, out block by out block
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) {
      f32x16 acc;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 b = *reinterpret_cast<const float4*>(b2 + ob * 32 + 8 * g4 + 4 * h);
        acc[4 * g4 + 0] = b.x; acc[4 * g4 + 1] = b.y; acc[4 * g4 + 2] = b.z; acc[4 * g4 + 3] = b.w;
      }
#pragma unroll
      for (int ks = 0; ks < KS2; ++ks) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[(ob * KS2 + ks) * 64], h1[ks], acc, 0, 0, 0);
        if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
      const f32x16 dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3t[ob], gb, f32x16{}, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32x4 hw = pack8_u32(acc, s, true);
        u32x4 dw = pack8_u32(dacc, s, false);
#pragma unroll
        for (int q = 0; q < 4; ++q) dw[q] = mask_pair(dw[q], hw[q]);
        store_sub(h2T, A.h2, valid, P, ob, s, hw);
        store_sub(dz2T, dz2W, true, P, ob, s, dw);  // row-major for stage (b): every padded row too
        if (A.dz2 && valid) {
#pragma unroll
          for (int q = 0; q < 2; ++q)
            *reinterpret_cast<uint2*>(A.dz2 + (P.t32 * H + 32 * ob + 16 * s + 8 * q) + P.rm_off) =
                make_uint2(dw[2 * q], dw[2 * q + 1]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

__global__ void __launch_bounds__(64 * TRAIN_WAVES) __attribute__((amdgpu_waves_per_eu(2)))
train_dz1(const BwdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const TrainLayout T(A.rows);
  stage(reinterpret_cast<int4*>(lds), reinterpret_cast<const int4*>(A.blob), (int)(W1F_BYTES / 16));
  stage(reinterpret_cast<int4*>(lds + W1F_BYTES), reinterpret_cast<const int4*>(A.ws + T.w2t), (int)(W2F_BYTES / 16));
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int n = lane & 31, h = lane >> 5;
  const int in = A.in;
  const long long ntiles = (long long)(T.ld / 32);
  const bf16x8* w1f = reinterpret_cast<const bf16x8*>(lds + 16 * lane);
  const bf16x8* w2t = reinterpret_cast<const bf16x8*>(lds + W1F_BYTES + 16 * lane);
  const uint16_t* dz2W = reinterpret_cast<const uint16_t*>(A.ws + T.dz2);
  uint16_t* dz1T = reinterpret_cast<uint16_t*>(A.ws + T.dz1T);
  for (long long tile = (long long)blockIdx.x * TRAIN_WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * TRAIN_WAVES) {
    size_t ld = T.ld;
    asm volatile("" : "+s"(ld));  // as in train_fwd_dz2
    LanePos P;
    P.ld = ld;
    P.t32 = (size_t)tile * 32;
    P.um_off = (uint32_t)(4 * h * ld + n);
    P.rm_off = (uint32_t)(n * H + 4 * h);
    const long long row = tile * 32 + n;
    const bool valid = row < A.rows;
    bf16x8 xb[KS1];
    load_obs(A.obs + (valid ? row : A.rows - 1) * in, in, h, xb);
    // dz2 of this row as natural-k B fragments: units 16 ks + 8 h + j
    bf16x8 dz[KS2];
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) dz[ks] = *reinterpret_cast<const bf16x8*>(dz2W + (P.t32 * H + 16 * ks) + (uint32_t)(n * H + 8 * h));
#pragma unroll
    for (int ib = 0; ib < OB; ++ib) {
      f32x16 a1 = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[(ib * KS1 + ks) * 64], xb[ks], a1, 0, 0, 0);
      f32x16 acc = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS2; ++ks) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2t[(ib * KS2 + ks) * 64], dz[ks], acc, 0, 0, 0);
        if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const u32x4 hw = pack8_u32(a1, s, true);
        u32x4 dw = pack8_u32(acc, s, false);
#pragma unroll
        for (int q = 0; q < 4; ++q) dw[q] = mask_pair(dw[q], hw[q]);
        store_sub(dz1T, A.dz1, valid, P, ib, s, dw);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ---------------------------------------------------------------- stage (c): weight gradients
// C[m][n] = sum over rows r of AT[m][r] BT[n][r] for one slab of rows (blockIdx.x).  Wave w of the
// workgroup owns MT x NT tiles of 32 x 32: m blocks MT jm .., n blocks NT jn .. (jm = w / (NB / NT),
// jn = w % (NB / NT)).  A k-chunk is 32 rows: lane (m, h) reads rows 32 c + 16 h + 8 s + j of k-step
// s = 0, 1 (32 contiguous bytes) from either operand — the same k order in both, whatever it is.
// BIAS: the waves with jn = 0 also sum A over the rows (an all-ones B fragment).
template <int MT, int NT, int WAVES, bool BIAS>
__global__ void __launch_bounds__(64 * WAVES) train_wgrad(const uint16_t* __restrict__ AT, const uint16_t* __restrict__ BT,
                                                          size_t ld, int NB, float* __restrict__ P, float* __restrict__ PB,
                                                          size_t slab_stride) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = lane & 31, h = lane >> 5;
  const int jn = wave % (NB / NT), jm = wave / (NB / NT);
  const size_t slab = blockIdx.x;
  const size_t r0 = slab * SLAB;
  const size_t r1 = r0 + SLAB < ld ? r0 + SLAB : ld;
  f32x16 acc[MT][NT], accb[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    accb[i] = f32x16{};
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};
  }
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.f;
  const bool bias_wave = BIAS && jn == 0;
  const uint16_t* ap = AT + (size_t)(jm * MT * 32 + n) * ld + 16 * h;
  const uint16_t* bp = BT + (size_t)(jn * NT * 32 + n) * ld + 16 * h;
  for (size_t r = r0; r < r1; r += 32) {
    bf16x8 a[MT][2], b[NT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s) a[i][s] = *reinterpret_cast<const bf16x8*>(ap + (size_t)i * 32 * ld + r + 8 * s);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) b[j][s] = *reinterpret_cast<const bf16x8*>(bp + (size_t)j * 32 * ld + r + 8 * s);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
        if (bias_wave) accb[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][s], ones, accb[i], 0, 0, 0);
      }
  }
  // this slab's partials: C row (i & 3) + 8 (i >> 2) + 4 h of the tile in register i, column n on the lane
  const int N = NB * 32;
  float* p = P + slab * slab_stride;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = (jm * MT + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        p[(size_t)m * N + (jn * NT + j) * 32 + n] = acc[i][j][q];
      }
  if (bias_wave && n == 0) {
    float* pb = PB + slab * slab_stride;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int q = 0; q < 16; ++q) pb[(jm * MT + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h] = accb[i][q];
  }
}

// ---------------------------------------------------------------- stage (d)
struct FinArgs {
  const float* part;  // [nslabs][PART_FLOATS]: P2 [256][256], PB2 [256], P3 [32][256], PB3 [32], P1 [256][64]
  float *dw1, *db1, *dw2, *db2, *dw3, *db3;
  int nslabs, in, out;
};
constexpr int P2_OFF = 0, PB2_OFF = H * H, P3_OFF = PB2_OFF + H, PB3_OFF = P3_OFF + GU * H, P1_OFF = PB3_OFF + GU;

// one thread per gradient element: partial 0, then + partial 1, + partial 2, ... in f32
__global__ void __launch_bounds__(256) train_finalise(const FinArgs A) {
  const int n1 = H * A.in, n3 = A.out * H;
  const int total = n1 + H + H * H + H + n3 + A.out;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int src;
  float* dst;
  if (i < n1) {
    src = P1_OFF + (i / A.in) * XU + i % A.in; dst = A.dw1 + i;
  } else if ((i -= n1) < H) {
    src = P1_OFF + i * XU + A.in; dst = A.db1 + i;  // the 1 in column `in` of x
  } else if ((i -= H) < H * H) {
    src = P2_OFF + i; dst = A.dw2 + i;
  } else if ((i -= H * H) < H) {
    src = PB2_OFF + i; dst = A.db2 + i;
  } else if ((i -= H) < n3) {
    src = P3_OFF + i; dst = A.dw3 + i;
  } else {
    i -= n3;
    src = PB3_OFF + i; dst = A.db3 + i;
  }
  float s = A.part[src];
  for (int k = 1; k < A.nslabs; ++k) s = s + A.part[(size_t)k * PART_FLOATS + src];
  *dst = s;
}

thread_local UnitError g_err;

int check_dims(int in_dim, int out_dim) {
  return actor_dims_ok(in_dim, out_dim) ? SWARM_OK : g_err.fail(SWARM_ELIMIT, "policy dims out of range");
}

}  // namespace

extern "C" {

const char* swarm_policy_train_last_error(void) { return g_err.msg; }

long long swarm_policy_train_workspace_bytes(int in_dim, int out_dim, long long rows) {
  if (check_dims(in_dim, out_dim) != SWARM_OK) return (long long)SWARM_ELIMIT;
  if (rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0"), (long long)SWARM_EINVAL;
  if (rows > SWARM_TRAIN_MAX_ROWS) return g_err.fail(SWARM_ELIMIT, "rows above SWARM_TRAIN_MAX_ROWS"), (long long)SWARM_ELIMIT;
  return (long long)TrainLayout(rows).total;
}

int swarm_policy_pack_device(int in_dim, int out_dim, const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* w3, const float* b3, void* weights, void* workspace, void* hip_stream) {
  if (check_dims(in_dim, out_dim) != SWARM_OK) return SWARM_ELIMIT;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !weights || !workspace) return g_err.fail(SWARM_ENULL, "null weight pointer");
  if (((uintptr_t)weights) % 16 || ((uintptr_t)workspace) % 16)
    return g_err.fail(SWARM_EINVAL, "weights and workspace must be 16-B aligned");
  const PackArgs a{w1, b1, w2, b2, w3, b3, static_cast<unsigned char*>(weights), static_cast<unsigned char*>(workspace),
                   in_dim, out_dim};
  const int slots = (int)((ActorLayout(out_dim).total + W2F_BYTES + W3T_BYTES) / 16);
  hipLaunchKernelGGL(train_pack, dim3((slots + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, a);
  return g_err.launch_status();
}

int swarm_policy_backward(const swarm_policy_backward_args_t* args, void* hip_stream) {
  if (!args) return g_err.fail(SWARM_ENULL, "args is NULL");
  if (check_dims(args->in_dim, args->out_dim) != SWARM_OK) return SWARM_ELIMIT;
  if (args->rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (args->rows > SWARM_TRAIN_MAX_ROWS) return g_err.fail(SWARM_ELIMIT, "rows above SWARM_TRAIN_MAX_ROWS");
  if (args->rows == 0) return SWARM_OK;
  if (!args->weights || !args->obs || !args->grad_logits || !args->workspace)
    return g_err.fail(SWARM_ENULL, "weights, obs, grad_logits or workspace is NULL");
  if (!args->dw1 || !args->db1 || !args->dw2 || !args->db2 || !args->dw3 || !args->db3)
    return g_err.fail(SWARM_ENULL, "a gradient output is NULL");
  if (((uintptr_t)args->weights) % 16 || ((uintptr_t)args->workspace) % 16)
    return g_err.fail(SWARM_EINVAL, "weights and workspace must be 16-B aligned");
  for (const uint16_t* p : {args->h1, args->h2, args->dz2, args->dz1})
    if (((uintptr_t)p) % 8) return g_err.fail(SWARM_EINVAL, "stage outputs must be 8-B aligned");
  hipStream_t s = (hipStream_t)hip_stream;
  const TrainLayout T(args->rows);
  unsigned char* ws = static_cast<unsigned char*>(args->workspace);
  const BwdArgs a{static_cast<const unsigned char*>(args->weights), args->obs, args->grad_logits, ws,
                  args->h1, args->h2, args->dz2, args->dz1, args->rows, args->in_dim, args->out_dim};
  // (a), (b): one wave per 32-row tile, TRAIN_WAVES per workgroup, at most TRAIN_MAX_BLOCKS workgroups
  const long long need = ((long long)(T.ld / 32) + TRAIN_WAVES - 1) / TRAIN_WAVES;
  const int grid = (int)(need < TRAIN_MAX_BLOCKS ? need : TRAIN_MAX_BLOCKS);
  const int lds_a = (int)(W1F_BYTES + W2F_BYTES + H * 4), lds_b = (int)(W1F_BYTES + W2F_BYTES);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(train_fwd_dz2), hipFuncAttributeMaxDynamicSharedMemorySize, lds_a) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(train_dz1), hipFuncAttributeMaxDynamicSharedMemorySize, lds_b) != hipSuccess)
    return g_err.fail(SWARM_EHIP, "hipFuncSetAttribute failed");
  hipLaunchKernelGGL(train_fwd_dz2, dim3(grid), dim3(64 * TRAIN_WAVES), lds_a, s, a);
  hipLaunchKernelGGL(train_dz1, dim3(grid), dim3(64 * TRAIN_WAVES), lds_b, s, a);
  // (c): one workgroup per slab
  const int nslabs = (int)T.nslabs;
  auto u16 = [&](size_t off) { return reinterpret_cast<const uint16_t*>(ws + off); };
  float* part = reinterpret_cast<float*>(ws + T.part);
  hipLaunchKernelGGL((train_wgrad<2, 4, 8, true>), dim3(nslabs), dim3(512), 0, s, u16(T.dz2T), u16(T.h1T), T.ld, OB,
                     part + P2_OFF, part + PB2_OFF, (size_t)PART_FLOATS);
  hipLaunchKernelGGL((train_wgrad<1, 4, 2, true>), dim3(nslabs), dim3(128), 0, s, u16(T.gT), u16(T.h2T), T.ld, OB,
                     part + P3_OFF, part + PB3_OFF, (size_t)PART_FLOATS);
  hipLaunchKernelGGL((train_wgrad<2, 2, 4, false>), dim3(nslabs), dim3(256), 0, s, u16(T.dz1T), u16(T.xT), T.ld, XU / 32,
                     part + P1_OFF, static_cast<float*>(nullptr), (size_t)PART_FLOATS);
  // (d)
  const FinArgs f{part, args->dw1, args->db1, args->dw2, args->db2, args->dw3, args->db3, nslabs, args->in_dim, args->out_dim};
  const int total = H * args->in_dim + H + H * H + H + args->out_dim * H + args->out_dim;
  hipLaunchKernelGGL(train_finalise, dim3((total + 255) / 256), dim3(256), 0, s, f);
  return g_err.launch_status();
}

}  // extern "C"
