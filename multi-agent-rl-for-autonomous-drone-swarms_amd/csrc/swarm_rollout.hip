// swarm_rollout.hip — what a rollout fragment needs besides the networks and the env step so that
// the whole fragment can be one replayed graph (gfx950; the arithmetic is written
// out in include/swarm_mi355x.h):
//
//   swarm_rollout_sample   one lane per row: actions = mean + expf(log_std) * z from logits, the
//                          Philox counter read from device memory (*counter_dev + counter_add), so a
//                          captured launch draws new noise on every replay
//   swarm_rollout_record   up to 8 (src, dst, bytes) segments copied by one launch: the per-step
//                          rows of a fragment (reward, flags, the next obs / global_state / valid)
//
// Neither changes an actor kernel: the sample kernel draws through swarm_nn.h's normals() and forms
// the action in the actors' expression, so equal logits give the actors' actions bit for bit.  No
// LDS, no atomics, no host synchronisation, no allocation; every launch repeats bit for bit.
#include "swarm_nn.h"

#pragma clang fp contract(off)

namespace {

thread_local UnitError g_err;

constexpr int THREADS = 256;

// ---------------------------------------------------------------- sampling
struct SampleArgs {
  const float* logits;
  float* actions;
  const unsigned long long* counter_dev;
  unsigned long long counter_add;
  long long rows;
  uint32_t seed_lo, seed_hi;
  int ad;
};

// what normals() reads of a forward kernel's argument block
struct NoiseKey {
  uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

__global__ void __launch_bounds__(THREADS) sample_kernel(const SampleArgs A) {
  // one uniform 8-byte read; the 64-bit sum carries into the high word
  const unsigned long long ctr = (A.counter_dev ? *A.counter_dev : 0ull) + A.counter_add;
  const NoiseKey key{A.seed_lo, A.seed_hi, (uint32_t)ctr, (uint32_t)(ctr >> 32)};
  const int ad = A.ad;
  for (long long row = (long long)blockIdx.x * THREADS + threadIdx.x; row < A.rows; row += (long long)gridDim.x * THREADS) {
    const float* lg = A.logits + row * (2 * ad);
    float z[6];
    normals(key, row, ad, z);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (k < ad) {
        float a = lg[k];
        a = a + expf(lg[ad + k]) * z[k];  // policy_mlp_bf16's expression and order
        A.actions[row * ad + k] = a;
      }
    }
  }
}

// ---------------------------------------------------------------- record
// A tile is TILE_BYTES consecutive bytes of one segment (the segment's last one may be shorter); the
// tiles of all segments are numbered in segment order and dealt to the workgroups round robin, so
// a 77 MB segment is spread over the whole grid and an 8-byte one costs one short tile.  A tile is
// copied by one workgroup with consecutive lanes on consecutive elements: 16-byte elements where
// the segment's src and dst are both 16-byte aligned, 4-byte ones where both are 4-byte aligned,
// bytes otherwise; the bytes behind the last whole element (only in a segment's last tile) go one
// per lane.  TILE_BYTES is a multiple of 16, so every tile of a segment starts at its alignment.
constexpr int TILE_BYTES = 16384;  // 256 lanes x 4 x 16 B
constexpr int CHUNKS = TILE_BYTES / 16;

struct RecordArgs {
  const unsigned char* src[SWARM_ROLLOUT_MAX_SEGMENTS];
  unsigned char* dst[SWARM_ROLLOUT_MAX_SEGMENTS];
  unsigned long long bytes[SWARM_ROLLOUT_MAX_SEGMENTS];
  unsigned long long tile_end[SWARM_ROLLOUT_MAX_SEGMENTS];  // running tile count up to and including the segment
  unsigned long long tiles;
};

template <class T>
__device__ __forceinline__ void copy_elems(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, uint32_t n) {
  const T* sp = reinterpret_cast<const T*>(s);
  T* dp = reinterpret_cast<T*>(d);
  for (uint32_t i = threadIdx.x; i < n; i += THREADS) dp[i] = sp[i];
}

__global__ void __launch_bounds__(THREADS) record_kernel(const RecordArgs A) {
  for (unsigned long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
    // the tile's segment: uniform over the workgroup (scalar compares on the kernel arguments)
    int g = 0;
#pragma unroll
    for (int i = 0; i < SWARM_ROLLOUT_MAX_SEGMENTS - 1; ++i) g += tile >= A.tile_end[i] ? 1 : 0;
    const unsigned char* sb = A.src[0];
    unsigned char* db = A.dst[0];
    unsigned long long nb = A.bytes[0], first = 0;
#pragma unroll
    for (int i = 1; i < SWARM_ROLLOUT_MAX_SEGMENTS; ++i)
      if (g == i) {
        sb = A.src[i];
        db = A.dst[i];
        nb = A.bytes[i];
        first = A.tile_end[i - 1];
      }
    const unsigned long long off = (tile - first) * TILE_BYTES;
    const unsigned long long left = nb - off;  // > 0: the segment has a tile here
    const uint32_t len = left < (unsigned long long)TILE_BYTES ? (uint32_t)left : (uint32_t)TILE_BYTES;
    const unsigned char* s = sb + off;
    unsigned char* d = db + off;
    const uintptr_t both = (uintptr_t)sb | (uintptr_t)db;
    uint32_t done;
    if ((both & 15) == 0) {
      if (len == TILE_BYTES) {  // a whole tile: four independent 16-byte loads in flight per lane
        const u32x4* sp = reinterpret_cast<const u32x4*>(s);
        u32x4* dp = reinterpret_cast<u32x4*>(d);
        u32x4 v[CHUNKS / THREADS];
#pragma unroll
        for (int j = 0; j < CHUNKS / THREADS; ++j) v[j] = sp[j * THREADS + threadIdx.x];
#pragma unroll
        for (int j = 0; j < CHUNKS / THREADS; ++j) dp[j * THREADS + threadIdx.x] = v[j];
        continue;
      }
      copy_elems<u32x4>(s, d, len >> 4);
      done = len & ~15u;
    } else if ((both & 3) == 0) {
      copy_elems<uint32_t>(s, d, len >> 2);
      done = len & ~3u;
    } else {
      copy_elems<unsigned char>(s, d, len);
      done = len;
    }
    if (threadIdx.x < len - done) d[done + threadIdx.x] = s[done + threadIdx.x];  // < 16 bytes
  }
}

}  // namespace

extern "C" {

const char* swarm_rollout_last_error(void) { return g_err.msg; }

int swarm_rollout_sample(const float* logits, long long rows, int act_dim, unsigned long long seed,
                         const unsigned long long* counter_dev, unsigned long long counter_add, float* actions,
                         void* hip_stream) {
  if (act_dim < 1 || act_dim > SWARM_ROLLOUT_MAX_ACT) return g_err.fail(SWARM_ELIMIT, "act_dim out of range [1, SWARM_ROLLOUT_MAX_ACT]");
  if (rows < 0) return g_err.fail(SWARM_EINVAL, "rows < 0");
  if (rows == 0) return SWARM_OK;
  if (!logits || !actions) return g_err.fail(SWARM_ENULL, "logits/actions is NULL");
  if (((uintptr_t)counter_dev) % 8) return g_err.fail(SWARM_EINVAL, "counter_dev must be 8-byte aligned");
  SampleArgs a;
  a.logits = logits;
  a.actions = actions;
  a.counter_dev = counter_dev;
  a.counter_add = counter_add;
  a.rows = rows;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.ad = act_dim;
  hipLaunchKernelGGL(sample_kernel, dim3(grid_for((rows + THREADS - 1) / THREADS, 8)), dim3(THREADS), 0, (hipStream_t)hip_stream, a);
  return g_err.launch_status();
}

int swarm_rollout_record(const swarm_rollout_record_t* r, void* hip_stream) {
  if (!r) return g_err.fail(SWARM_ENULL, "record is NULL");
  if (r->count < 0) return g_err.fail(SWARM_EINVAL, "count < 0");
  if (r->count > SWARM_ROLLOUT_MAX_SEGMENTS) return g_err.fail(SWARM_ELIMIT, "more than SWARM_ROLLOUT_MAX_SEGMENTS segments");
  RecordArgs a;
  unsigned long long tiles = 0;
  int used = 0;
  for (int i = 0; i < r->count; ++i) {
    const swarm_rollout_segment_t& g = r->segments[i];
    if (!g.dst || g.bytes == 0) continue;
    if (!g.src) return g_err.fail(SWARM_ENULL, "a segment's src is NULL");
    if (g.bytes > (1ull << 46)) return g_err.fail(SWARM_ELIMIT, "a segment is larger than 2^46 bytes");
    tiles += ((g.bytes + 15) / 16 + CHUNKS - 1) / CHUNKS;
    a.src[used] = static_cast<const unsigned char*>(g.src);
    a.dst[used] = static_cast<unsigned char*>(g.dst);
    a.bytes[used] = g.bytes;
    a.tile_end[used] = tiles;
    ++used;
  }
  if (used == 0) return SWARM_OK;
  for (int i = used; i < SWARM_ROLLOUT_MAX_SEGMENTS; ++i) {  // never selected: tile < tiles == tile_end[i]
    a.src[i] = nullptr;
    a.dst[i] = nullptr;
    a.bytes[i] = 0;
    a.tile_end[i] = tiles;
  }
  a.tiles = tiles;
  // the grid from the 16-byte chunk counts: a workgroup per tile (the segments' chunks in CHUNKS-sized
  // pieces), at most 8 per CU; the rest of the tiles are walked grid-stride
  hipLaunchKernelGGL(record_kernel, dim3(grid_for((long long)tiles, 8)), dim3(THREADS), 0, (hipStream_t)hip_stream, a);
  return g_err.launch_status();
}

}  // extern "C"
