// Exact k nearest neighbours of every point among the points of its own fragment, on the radius index of overlap.hip
// (mvreg.h mvr_knn_self): the counterpart of Open3D's KDTreeFlann.search_knn_vector_3d on the cloud
// it was built on, restated from the maths.
//
// Two kernels.  knn_self_kernel: one thread per point, thread s the point at position s of the index's sorted order
// (a wave's threads sit in a few neighbouring cells and read the same rows, as in normals.hip).  The thread keeps its
// best min(k, n_b) candidates, ordered by (d2, row), in LDS laid out [slot][thread] (a wave's accesses to one slot are
// consecutive words), the worst of them in registers: only a candidate below it enters the insertion.  It walks the
// cells ring by ring (Chebyshev ring 1: the 27 cells, ring 2: the 98 around them), skips a cell whose box lies farther
// than the worst kept, and is resolved after ring rho when the list is full and its worst lies within
// rho r + (the distance to the nearest face of the point's own cell) less the slack: every point of a cell not walked
// is then strictly farther.  A full list of all n_b points is resolved too.  What is left after ring kKnnRhoMax goes
// into a list in the workspace, and knn_fallback_kernel (a fixed grid, the count read from device memory) scans the
// rows of such a point's fragment directly, one wave per point: every lane keeps the best of every 64th row in the
// same LDS lists and the wave merges the 64 sorted lists by shuffles.  n_b distance evaluations bound the work of an
// isolated point, and the result is exact for any input.  The order of that list varies from run to run; nothing that is computed depends on
// it.  The result is the set of the min(k, n_b) smallest (d2, row), a function of the fragment alone, whatever path
// and whatever order of the cells found it.
// Every loop is bounded: kKnnRhoMax, a ring's cells, a cell's rows, the insertion (k), the hash probe (cap >= 2 M),
// n_b.  One atomic: the list's counter.
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// One wave per workgroup: nothing is shared between waves, and the LDS of a workgroup is k * 12 bytes per thread
// (48 KB at k = 64), so the smallest workgroup leaves the finest grain for the occupancy the LDS allows.
#ifndef MVR_KNN_THREADS
#define MVR_KNN_THREADS 64
#endif
// the last ring the first kernel walks (DESIGN.md 4.21a has 2 against 3)
#ifndef MVR_KNN_RHO_MAX
#define MVR_KNN_RHO_MAX 2
#endif
constexpr int kKnnThreads = MVR_KNN_THREADS;
constexpr int kKnnRhoMax = MVR_KNN_RHO_MAX;
constexpr int kKnnMaxK = 64;
constexpr int kKnnFallbackBlocks = 2048;   // waves of the direct scan, each taking the list's entries b, b + 2048, ...

extern __shared__ double knn_lds[];   // keys [k][kKnnThreads] fp64, then ids [k][kKnnThreads] int32

// A thread's candidates: slots [0, cnt) ascending by (d2, row); full at cnt == kk, then (kd, kid) is the last slot
struct KnnList {
  double* key;
  int32_t* id;
  int kk, cnt;
  double kd;
  int32_t kid;

  __device__ __forceinline__ void init(int k, int kk_) {
    key = knn_lds + threadIdx.x;
    id = reinterpret_cast<int32_t*>(knn_lds + (size_t)k * kKnnThreads) + threadIdx.x;
    kk = kk_;
    cnt = 0;
    kd = INFINITY;
    kid = 0x7fffffff;
  }
  __device__ __forceinline__ void offer(double d, int32_t t) {
    if (!(d < kd || (d == kd && t < kid))) return;   // a NaN distance never enters
    int j = cnt < kk ? cnt : kk - 1;
    while (j > 0) {
      const double pk = key[(j - 1) * kKnnThreads];
      const int32_t pi = id[(j - 1) * kKnnThreads];
      if (!(pk > d || (pk == d && pi > t))) break;
      key[j * kKnnThreads] = pk;
      id[j * kKnnThreads] = pi;
      --j;
    }
    key[j * kKnnThreads] = d;
    id[j * kKnnThreads] = t;
    if (cnt < kk) ++cnt;
    if (cnt == kk) {
      kd = key[(kk - 1) * kKnnThreads];
      kid = id[(kk - 1) * kKnnThreads];
    }
  }
  // row i of the outputs: the found entries, then -1 / +inf up to k
  __device__ __forceinline__ void store(int64_t i, int k, int32_t* __restrict__ idx, double* __restrict__ dist2) const {
    int32_t* oi = idx + i * k;
    double* od = dist2 + i * k;
    for (int s = 0; s < k; ++s) {
      const bool found = s < cnt;
      oi[s] = found ? id[s * kKnnThreads] : -1;
      od[s] = found ? key[s * kKnnThreads] : (double)INFINITY;
    }
  }
};

// (ex*ex + ey*ey) + ez*ez, every product and sum rounded on its own
__device__ __forceinline__ double knn_d2(const double* __restrict__ xyz, int64_t t, const double (&p)[3]) {
#pragma clang fp contract(off)
  const double ex = xyz[3 * t] - p[0], ey = xyz[3 * t + 1] - p[1], ez = xyz[3 * t + 2] - p[2];
  return (ex * ex + ey * ey) + ez * ez;
}

// a lower bound of the distance along one axis to the cells d cells away, shrunk by the slack
__device__ __forceinline__ double axis_gap(int d, double lo, double r, double slack) {
  if (d == 0) return 0.0;
  return fmax((d < 0 ? lo : r - lo) + (double)((d < 0 ? -d : d) - 1) * r - slack, 0.0);
}

__global__ __launch_bounds__(kKnnThreads) void knn_self_kernel(RIndex ix, const double* __restrict__ xyz,
                                                               const int64_t* __restrict__ off, int64_t M, double r,
                                                               int k, int32_t* __restrict__ idx,
                                                               double* __restrict__ dist2, int32_t* n_left,
                                                               int32_t* __restrict__ left) {
  const int64_t s = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
  if (s >= M) return;   // no barrier below
  int64_t i, t0, t1, c[3];
  int b;
  double p[3], lo[3], face = r;   // face: the distance to the nearest face of the point's own cell
  point_at(ix, xyz, s, i, b, p);
  frag_rows(off, b, M, t0, t1);
  const int64_t n_b = t1 - t0;
  const double slack = 1e-9 * r;
  cell_of(p, r, c, lo);
  for (int e = 0; e < 3; ++e) face = fmin(face, fmin(lo[e], r - lo[e]));
  KnnList L;
  L.init(k, (int)(n_b < k ? (n_b > 0 ? n_b : 1) : k));
  bool resolved = false;
  for (int rho = 1; rho <= kKnnRhoMax && !resolved; ++rho) {
    const int w = 2 * rho + 1, n = w * w * w;
    for (int q = 0; q < n; ++q) {
      const int cell = (q + n / 2) % n;   // ring 1: the point's own cell first
      const int dx = cell % w - rho, dy = (cell / w) % w - rho, dz = cell / (w * w) - rho;
      if (rho > 1 && abs(dx) < rho && abs(dy) < rho && abs(dz) < rho) continue;   // walked by an earlier ring
      const double gx = axis_gap(dx, lo[0], r, slack), gy = axis_gap(dy, lo[1], r, slack),
                   gz = axis_gap(dz, lo[2], r, slack);
      if (gx * gx + gy * gy + gz * gz > L.kd) continue;   // no point of that cell can enter (kd = inf until full)
      const int2 se = cell_find(ix, pack_key(b, c[0] + dx, c[1] + dy, c[2] + dz));
      for (int j = se.x; j < se.y; ++j) {
        const int32_t t = ix.sidx[j];
        L.offer(knn_d2(xyz, t, p), t);
      }
    }
    // a point of a cell not walked yet lies farther than rho r + face along some axis
    const double reach = fmax((double)rho * r + face - slack, 0.0);
    resolved = L.cnt == L.kk && (L.kk == n_b || L.kd <= reach * reach);
  }
  if (resolved)
    L.store(i, k, idx, dist2);
  else
    left[atomicAdd(n_left, 1)] = (int32_t)s;   // at most M entries
}

__global__ __launch_bounds__(kKnnThreads) void knn_fallback_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                   const int64_t* __restrict__ off, int64_t M, int k,
                                                                   int32_t* __restrict__ idx,
                                                                   double* __restrict__ dist2, const int32_t* n_left,
                                                                   const int32_t* __restrict__ left) {
  static_assert(kKnnThreads == kWave, "the direct scan is one wave per query");
  const int lane = threadIdx.x;
  int64_t n = *n_left;
  n = n < 0 ? 0 : (n > M ? M : n);
  for (int64_t q = blockIdx.x; q < n; q += gridDim.x) {   // uniform over the wave, as everything but the scan
    const int64_t s = left[q];
    if (s < 0 || s >= M) continue;
    int64_t i, t0, t1;
    int b;
    double p[3];
    point_at(ix, xyz, s, i, b, p);
    frag_rows(off, b, M, t0, t1);
    const int64_t n_b = t1 - t0;
    const int kk = (int)(n_b < k ? (n_b > 0 ? n_b : 1) : k);
    // every lane keeps the best kk of its rows t0 + lane, t0 + lane + 64, ...: the best kk of all are among them
    KnnList L;
    L.init(k, kk);
    for (int64_t t = t0 + lane; t < t1; t += kWave) L.offer(knn_d2(xyz, t, p), (int32_t)t);
    // merge: kk times the smallest head (d2, row) of the 64 sorted lists; rows are distinct, so one lane owns it
    int32_t* oi = idx + i * k;
    double* od = dist2 + i * k;
    int at = 0;
    for (int o = 0; o < kk; ++o) {
      const bool has = at < L.cnt;
      double hd = has ? L.key[at * kKnnThreads] : (double)INFINITY;
      int32_t hi = has ? L.id[at * kKnnThreads] : 0x7fffffff;
      const int32_t mine = hi;
#pragma unroll
      for (int x = 32; x > 0; x >>= 1) {
        const double od2 = __shfl_xor(hd, x, kWave);
        const int32_t oi2 = __shfl_xor(hi, x, kWave);
        if (od2 < hd || (od2 == hd && oi2 < hi)) { hd = od2; hi = oi2; }
      }
      if (has && mine == hi) ++at;
      if (lane == 0) {   // no head left (rows with a NaN distance never enter): the padding
        oi[o] = hi == 0x7fffffff ? -1 : hi;
        od[o] = hi == 0x7fffffff ? (double)INFINITY : hd;
      }
    }
    for (int o = kk + lane; o < k; o += kWave) {
      oi[o] = -1;
      od[o] = (double)INFINITY;
    }
  }
}

inline size_t knn_ws_bytes(int64_t M) { return 256 + (((size_t)(M > 0 ? M : 1) * 4 + 255) & ~(size_t)255); }

}  // namespace mvr

extern "C" size_t mvr_knn_self_workspace_bytes(int64_t M) { return mvr::knn_ws_bytes(M); }

extern "C" int mvr_knn_self(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                            int64_t M, double r_index, int k, int32_t* idx, double* dist2, void* workspace,
                            size_t workspace_bytes, hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, r_index) || k < 1 || k > mvr::kKnnMaxK) return MVR_EINVAL;   // no radius
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !idx || !dist2 || !workspace ||
      workspace_bytes < mvr::knn_ws_bytes(M))
    return MVR_EINVAL;
  int32_t* n_left = reinterpret_cast<int32_t*>(workspace);          // workspace: the counter, then at 256 the list
  int32_t* left = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + 256);
  if (hipMemsetAsync(n_left, 0, 256, stream) != hipSuccess) return MVR_ELAUNCH;
  const size_t lds = (size_t)k * mvr::kKnnThreads * 12;
  const int rc = mvr::launch_per_point<mvr::kKnnThreads>(mvr::knn_self_kernel, index, M, lds, stream, xyz, off, M,
                                                         r_index, k, idx, dist2, n_left, left);
  if (rc != MVR_OK) return rc;
  const unsigned fb = M < mvr::kKnnFallbackBlocks ? (unsigned)M : (unsigned)mvr::kKnnFallbackBlocks;
  hipLaunchKernelGGL(mvr::knn_fallback_kernel, dim3(fb), dim3(mvr::kKnnThreads), lds, stream,
                     mvr::index_view(const_cast<void*>(index), M), xyz, off, M, k, idx, dist2, n_left, left);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
