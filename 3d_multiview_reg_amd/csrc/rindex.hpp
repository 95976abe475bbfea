// The per-fragment radius index (built by overlap.hip mvr_radius_index_build): points sorted by (fragment, cell of
// size r) and an open-addressing hash of the occupied cells.  The layout is ABI (mvr_radius_index_bytes).  Its users:
// the overlap gate (overlap.hip) and the scene fusion (fuse.hip); through icp_core.hpp the nearest-neighbour kernels
// (icp.hip, icp_plane.hip, icp_gicp.hip, icp_robust.hip, icp_colored.hip, info.hip); and the per-point kernels, one
// thread per point in the index's sorted order over the ball around it (normals.hip, iss.hip, color_grad.hip,
// outlier.hip, fpfh.hip, knn_self.hip), which take from here their prologue (point_at), the cell of a
// point (cell_of), the walk of the ball (ball_walk), a fragment's rows (frag_rows) and, on the host, the checks of an
// entry and the launch (ball_values_ok, index_pointers_ok, launch_per_point).
#pragma once
#include "common.hpp"
#include "mvreg.h"

namespace mvr {

constexpr uint64_t OV_EMPTY = ~0ull;
constexpr int OV_BITS = 16;                 // bits per cell / voxel coordinate
constexpr int64_t OV_BIAS = 1 << 15;        // signed cell coordinates are biased by 2^15

__device__ __forceinline__ uint64_t pack_key(int b, int64_t x, int64_t y, int64_t z) {
  const uint64_t m = (1ull << OV_BITS) - 1;
  return ((uint64_t)b << (3 * OV_BITS)) | (((uint64_t)x & m) << (2 * OV_BITS)) | (((uint64_t)y & m) << OV_BITS) |
         ((uint64_t)z & m);
}
__device__ __forceinline__ uint64_t hash64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

struct RIndex {
  int32_t* sidx;      // [M] point ids in (fragment, cell) order
  uint64_t* skey;     // [M]
  uint64_t* hkeys;    // [cap]
  int2* hval;         // [cap] (start, end) of the cell in the sorted order
  uint64_t cap;
};

// the probe ends at an empty slot: cap >= 2 M and at most M cells are occupied
__device__ __forceinline__ int2 cell_find(const RIndex& ix, uint64_t k) {
  uint64_t h = hash64(k) & (ix.cap - 1);
  while (true) {
    const uint64_t s = ix.hkeys[h];
    if (s == k) return ix.hval[h];
    if (s == OV_EMPTY) return make_int2(0, 0);
    h = (h + 1) & (ix.cap - 1);
  }
}

// The point at position s < M of the index's sorted order: its row i of xyz, its fragment b and its coordinates p.
// Thread s of a per-point kernel takes it, so a wave's threads sit in a few neighbouring cells and read the same rows.
__device__ __forceinline__ void point_at(const RIndex& ix, const double* __restrict__ xyz, int64_t s, int64_t& i, int& b,
                                         double (&p)[3]) {
  i = ix.sidx[s];
  b = (int)(ix.skey[s] >> (3 * OV_BITS));
  for (int e = 0; e < 3; ++e) p[e] = xyz[3 * i + e];
}

// The cell of size r that holds p, biased as pack_key takes it, and lo, p's distance to the lower neighbour cell
// along each axis (r - lo to the upper one)
__device__ __forceinline__ void cell_of(const double (&p)[3], double r, int64_t (&c)[3], double (&lo)[3]) {
  for (int e = 0; e < 3; ++e) {
    const double cf = floor(p[e] / r);
    c[e] = (int64_t)cf + OV_BIAS;
    lo[e] = p[e] - cf * r;
  }
}

// the rows [t0, t1) of fragment b, clamped into [0, M]
__device__ __forceinline__ void frag_rows(const int64_t* __restrict__ off, int b, int64_t M, int64_t& t0, int64_t& t1) {
  t0 = off[b];
  t1 = off[b + 1];
  t0 = t0 < 0 ? 0 : (t0 > M ? M : t0);
  t1 = t1 < t0 ? t0 : (t1 > M ? M : t1);
}

// The walk of the ball of `radius` <= r around p over fragment b's points: the 27 cells around floor(p / r) through
// the cell hash, without those whose box lies outside the ball (a lower bound of the distance to the box, shrunk by
// slack = 1e-9 r, far above the rounding of p / r).  in_ball(t, j, ex, ey, ez) is called for every row t of the
// fragment, at position j of the sorted order, with sqrt(ex*ex + ey*ey + ez*ez) < radius (strict), e = x_t - p, in the
// order of the cells and of a cell's rows, which follows the index alone.  Bounded: 27 cells, a cell's rows, the hash
// probe.
template <class F>
__device__ __forceinline__ void ball_walk(const RIndex& ix, const double* __restrict__ xyz, int b, const double (&p)[3],
                                          double r, double radius, F&& in_ball) {
  const double slack = 1e-9 * r, rad2 = radius * radius * (1.0 + 1e-9);
  int64_t c[3];
  double lo[3];
  cell_of(p, r, c, lo);
  for (int cell = 0; cell < 27; ++cell) {
    const int dx = cell % 3 - 1, dy = (cell / 3) % 3 - 1, dz = cell / 9 - 1;
    const double gx = dx == 0 ? 0.0 : fmax((dx < 0 ? lo[0] : r - lo[0]) - slack, 0.0);
    const double gy = dy == 0 ? 0.0 : fmax((dy < 0 ? lo[1] : r - lo[1]) - slack, 0.0);
    const double gz = dz == 0 ? 0.0 : fmax((dz < 0 ? lo[2] : r - lo[2]) - slack, 0.0);
    if (gx * gx + gy * gy + gz * gz > rad2) continue;   // no point of that cell lies in the ball
    const int2 se = cell_find(ix, pack_key(b, c[0] + dx, c[1] + dy, c[2] + dz));
    for (int j = se.x; j < se.y; ++j) {
      const int64_t t = ix.sidx[j];
      const double ex = xyz[3 * t] - p[0], ey = xyz[3 * t + 1] - p[1], ez = xyz[3 * t + 2] - p[2];
      if (sqrt(ex * ex + ey * ey + ez * ez) < radius) in_ball(t, j, ex, ey, ez);
    }
  }
}

inline char* take(char*& p, size_t b) {
  p = reinterpret_cast<char*>(((uintptr_t)p + 255) & ~(uintptr_t)255);
  char* r = p;
  p += b;
  return r;
}
inline uint64_t cap_for(int64_t M) {
  uint64_t c = 1024;
  while (c < (uint64_t)(2 * (M > 0 ? M : 1))) c <<= 1;
  return c;
}
inline RIndex index_view(void* base, int64_t M) {
  char* p = reinterpret_cast<char*>(base);
  RIndex ix{};
  ix.cap = cap_for(M);
  ix.sidx = reinterpret_cast<int32_t*>(take(p, (size_t)(M > 0 ? M : 1) * 4));
  ix.skey = reinterpret_cast<uint64_t*>(take(p, (size_t)(M > 0 ? M : 1) * 8));
  ix.hkeys = reinterpret_cast<uint64_t*>(take(p, ix.cap * 8));
  ix.hval = reinterpret_cast<int2*>(take(p, ix.cap * 8));
  return ix;
}

// ---------------------------------------------------------------------------------- entry points on the index (host)
// The scalar rules of an entry that walks a ball of `radius` on the index: M in [0, 2^31), B in (0, 2^15), r_index
// and radius positive, the ball inside a cell (a NaN fails).  An entry makes them first, then returns MVR_OK at
// M == 0, then looks at its pointers
inline bool ball_values_ok(int B, int64_t M, double r_index, double radius) {
  return M >= 0 && M <= 0x7fffffff && B > 0 && B < (1 << 15) && radius > 0.0 && r_index > 0.0 && !(radius > r_index);
}
// the pointers every entry on the index takes, and the index's size; nothing is looked at without points
inline bool index_pointers_ok(const void* index, size_t index_bytes, const double* xyz, const int64_t* off,
                              int64_t M) {
  return M == 0 || (index && xyz && off && index_bytes >= mvr_radius_index_bytes(M));
}
// kernel(index's view, args...), one thread per point: ceil(M / kThreads) workgroups of kThreads, lds dynamic bytes
template <int kThreads, class... P, class... A>
inline int launch_per_point(void (*kernel)(RIndex, P...), const void* index, int64_t M, size_t lds, hipStream_t stream,
                            A... args) {
  const unsigned blocks = (unsigned)((M + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), lds, stream, index_view(const_cast<void*>(index), M),
                     args...);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}

}  // namespace mvr
