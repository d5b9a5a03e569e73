// swarm_env_cfg.h — what the units that write swarm_env_cfg_t records on the device must agree on
// (swarm_kernel.hip: swarm_env_cfg_set; swarm_dr.hip: swarm_env_cfg_randomize), written once.
// Internal: not installed, not part of the C-ABI; included as "swarm_env_cfg.h", next to the sources.
// Internal linkage: each unit compiles its own copy.
#pragma once

#include <hip/hip_runtime.h>

namespace {

// s_threshold on the device: the same search with IEEE sqrt (llvm.sqrt) and one-ulp steps on
// the bit pattern (every argument here is finite and >= 0, so the patterns are ordered).
__device__ float s_threshold_dev(float T) {
  if (!(T >= 0.0f)) return -1.0f;
  if (__builtin_isinf(T)) return __builtin_inff();
  float s = T * T;
  while (s > 0.0f && __builtin_sqrtf(s) > T) s = __uint_as_float(__float_as_uint(s) - 1u);
  for (;;) {
    const float nx = __uint_as_float(__float_as_uint(s) + 1u);
    if (__builtin_isinf(nx) || __builtin_sqrtf(nx) > T) break;
    s = nx;
  }
  return s;
}

}  // namespace
