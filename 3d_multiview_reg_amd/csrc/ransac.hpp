// What the sampling registrations share (ransac.hip: mvr_ransac, mvr_ransac_checked; fgr.hip: the tuple filter and the
// final score): the counter-stream draws, the edge-length test and the row distance of the evaluation.  The
// comparisons and the evaluation are rounded fp64 operations in a fixed order (no fma), the host restatements'
// (oracle/ransac.py, tests/ransac_checked_oracle.py) bit for bit.
#pragma once
#include "common.hpp"

namespace mvr {

// splitmix64 of seed + ctr * golden; ransac_draws packs (pair, iteration, draw) into ctr (oracle/ransac.py:draws)
__device__ __forceinline__ uint64_t ransac_draw(uint64_t seed, uint64_t ctr) {
  uint64_t z = seed + ctr * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the k <= M draws of iteration `it` of pair p out of n rows; c[k ..] = 0
template <int M>
__device__ __forceinline__ void ransac_draws(uint64_t seed, int p, uint64_t it, int n, int k, int64_t (&c)[M]) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const uint64_t ctr = ((uint64_t)p << 40) | (it << 8) | (uint64_t)j;
    c[j] = j < k ? (int64_t)(ransac_draw(seed, ctr) % (uint64_t)n) : 0;
  }
}

// the edge-length test on two correspondences (source points sa, sb, target points da, db): each of the two squared
// lengths at least sim2 times the other
__device__ __forceinline__ bool ransac_edge_ok(const double* sa, const double* sb, const double* da, const double* db,
                                               double sim2) {
#pragma clang fp contract(off)
  const double s0 = sa[0] - sb[0], s1 = sa[1] - sb[1], s2 = sa[2] - sb[2];
  const double t0 = da[0] - db[0], t1 = da[1] - db[1], t2 = da[2] - db[2];
  const double ls2 = (s0 * s0 + s1 * s1) + s2 * s2;
  const double lt2 = (t0 * t0 + t1 * t1) + t2 * t2;
  return ls2 >= sim2 * lt2 && lt2 >= sim2 * ls2;
}

// |R x + t - y|^2 in the evaluation's operation order (oracle/ransac.py evaluate).  Row e of R at R + RS e, t[e] at
// t + TS e: <3, 1> over R[3][3], t[3]; <4, 4> over the rows of a 3 x 4 [R | t] (t = its column 3)
template <int RS, int TS>
__device__ __forceinline__ double ransac_row_d2(const double* R, const double* t, const double* x, const double* y) {
#pragma clang fp contract(off)
  const double a = x[0], b = x[1], c = x[2];
  double dd = 0.0;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double v = ((R[RS * e] * a + R[RS * e + 1] * b) + R[RS * e + 2] * c) + t[TS * e];
    const double df = v - y[e];
    dd = dd + df * df;
  }
  return dd;
}

}  // namespace mvr
