// What mvr_ransac (procrustes.hip) and mvr_ransac_checked (ransac_checked.hip) share: the counter-stream draw.
#pragma once
#include "common.hpp"

namespace mvr {

// draw j of iteration i for pair p: ransac_draw(seed, (p << 40) | (i << 8) | j) % n (oracle/ransac.py:draws)
__device__ __forceinline__ uint64_t ransac_draw(uint64_t seed, uint64_t ctr) {
  uint64_t z = seed + ctr * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace mvr
