// The per-fragment radius index (built by overlap.hip mvr_radius_index_build): points sorted by (fragment, cell of
// size r) and an open-addressing hash of the occupied cells.  Shared by the overlap gate (overlap.hip), the normals
// (normals.hip), the FPFH descriptors (fpfh.hip) and, through icp_core.hpp, the ICP refinements (icp.hip,
// icp_plane.hip, icp_gicp.hip) and the information matrices (info.hip).  The layout is ABI (mvr_radius_index_bytes).
#pragma once
#include "common.hpp"

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

}  // namespace mvr
