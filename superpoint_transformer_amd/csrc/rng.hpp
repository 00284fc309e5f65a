// Counter-based random numbers shared by the sampling and the augmentation kernels.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace spt {

// splitmix64 finaliser over (seed, counter): counter-based, no state, reproducible
__host__ __device__ __forceinline__ uint32_t rand32(uint64_t seed, uint64_t i) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 32);
}

// decision uniform in [0, 1): the top 24 bits, exact in f32 (compare `u < p` like torch.rand)
__host__ __device__ __forceinline__ float rand_unit(uint64_t seed, uint64_t i) {
  return (float)(rand32(seed, i) >> 8) * 0x1p-24f;
}

}  // namespace spt
