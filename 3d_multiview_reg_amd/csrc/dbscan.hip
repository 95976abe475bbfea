// DBSCAN clustering of every fragment's own points on the radius index (mvreg.h mvr_cluster_dbscan):
// what Open3D's cluster_dbscan(eps, min_points) returns when it is called per fragment, restated from the definition
// (core points, the connected components of the eps-graph on them, border points to the lowest-numbered cluster among
// their core neighbours), which is what the sequential loop computes.  tests/dbscan_oracle.py restates that loop.
//
// Five launches and one scan, each per-point launch one thread per point in the index's sorted order on the core of
// rindex.hpp (4.33), rows of xyz (global) everywhere:
//   core     count the ball; parent[i] = i for a core row, -1 for any other.
//   link     a core row i walks its ball and unites its set with that of every core row t < i of it (each edge of the
//            graph is taken once, from its larger end) by lock-free hooking: find both roots, hook the larger under
//            the smaller with a compare-and-swap that succeeds only while the larger still is a root.
//   flatten  root[i] = the root of i's tree (-1 for a row that is not core), flag[i] = i is a root; flag[M] = 0.
//   scan     rank = the exclusive sum of flag over [0, M]: rows of a fragment are contiguous, so a root's number within
//            its fragment is rank[root] - rank[off[b]] and the fragment has rank[off[b + 1]] - rank[off[b]] clusters.
//   label    a core row takes its root's number; any other row walks its ball for the smallest root among the core
//            rows of it (roots are numbered in ascending order, so the smallest root is the lowest number), -1 with
//            none.  Sizes are integer adds (order-independent), one per wave and distinct cluster, not one per point:
//            in a fragment that is one cluster every point would otherwise add to one address.
//   counts   n_clusters[b], one thread per fragment.
//
// Termination without waiting.  Every write to parent[x] (the hook, and the shortening of a path in find_root) puts a
// smaller row of x's own set there, and only rows whose parent is themselves are hooked: parent[x] <= x at all times,
// with equality exactly at the roots, and a row that has stopped being a root never becomes one again.  So every find
// is a strictly decreasing walk, a failed compare-and-swap returns a strictly smaller parent, the larger of the two
// roots of a retry strictly decreases, and no cycle can form.  No thread waits for another: there is no lock and no
// flag to spin on.  Sets only merge; when the launch has ended every edge has been united, so a tree is a component,
// and since every ancestor is smaller, its root is the component's smallest core row whatever the interleaving was:
// root, flag, rank and everything after them are a pure function of the points.
//
// Visibility across workgroups.  A compute unit's L1 is not refreshed by the stores of another (and the L2s of the
// XCDs are not coherent with each other), so a plain re-read after a failed compare-and-swap could return the same
// stale value for ever.  In the link kernel every read of parent is therefore a relaxed agent-scope atomic load
// (served past the L1), every write is an agent-scope compare-and-swap, and a retry continues from the value the
// compare-and-swap itself returned.  The launches' boundaries order the phases: after them plain loads do.
#include "common.hpp"
#include "radix.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

constexpr int kDbscanThreads = 64;   // as radius_count_kernel: nothing is shared between a workgroup's waves
constexpr int kRowThreads = 256;     // the launches over rows that walk no ball

__device__ __forceinline__ int32_t parent_load(const int32_t* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x]: want -> put, only while it still is `want`; -> what was there
__device__ __forceinline__ int32_t parent_cas(int32_t* parent, int x, int32_t want, int32_t put) {
  __hip_atomic_compare_exchange_strong(parent + x, &want, put, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return want;
}

// The root of core row x's tree, p = parent[x] as just read.  On the way a row whose parent is no root gets its
// grandparent for a parent (only while the parent still is the one read: the entry can only decrease).  x strictly
// decreases, at most x steps (the loop's condition is p != x under 0 <= p <= x, and says so).
__device__ __forceinline__ int find_root(int32_t* parent, int x, int32_t p) {
  while ((uint32_t)p < (uint32_t)x) {
    const int32_t gp = parent_load(parent, p);
    if (gp != p) parent_cas(parent, x, p, gp);
    x = p;
    p = gp;
  }
  return x;
}
__device__ __forceinline__ int find_root(int32_t* parent, int x) { return find_root(parent, x, parent_load(parent, x)); }

// Unite the sets of the roots-to-be a and b -> a row of the united set, its root when last seen.  A failed hook means
// hi has been hooked by another thread meanwhile: the walk goes on from the parent it was given, and max(a, b)
// strictly decreases from one round to the next.
__device__ __forceinline__ int unite(int32_t* parent, int a, int b) {
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t was = parent_cas(parent, hi, hi, lo);
    if (was == hi) return lo;
    a = find_root(parent, was);
    b = find_root(parent, lo);
  }
  return a;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_core_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                     int64_t M, double r, double eps, int min_points,
                                                                     int32_t* __restrict__ parent,
                                                                     uint8_t* __restrict__ core) {
  const int64_t s = (int64_t)blockIdx.x * kDbscanThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b, n = 0;
  double p[3];
  point_at(ix, xyz, s, i, b, p);
  ball_walk(ix, xyz, b, p, r, eps, [&](int64_t, int, double, double, double) { ++n; });
  const bool is_core = n >= min_points;
  parent[i] = is_core ? (int32_t)i : -1;
  if (core) core[i] = is_core ? 1 : 0;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_link_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                     int64_t M, double r, double eps,
                                                                     int32_t* parent) {
  const int64_t s = (int64_t)blockIdx.x * kDbscanThreads + threadIdx.x;
  if (s >= M) return;   // no barrier and no wave operation below
  int64_t i;
  int b;
  double p[3];
  point_at(ix, xyz, s, i, b, p);
  if (parent_load(parent, (int)i) < 0) return;   // not core: nothing to unite
  int mine = (int)i;                             // a row of i's set, its root when last seen
  ball_walk(ix, xyz, b, p, r, eps, [&](int64_t t, int, double, double, double) {
    if (t >= i) return;                          // the edge belongs to its larger end
    const int32_t pt = parent_load(parent, (int)t);
    if (pt < 0) return;                          // not core (that never changes)
    const int rt = find_root(parent, (int)t, pt);
    mine = find_root(parent, mine);
    if (mine != rt) mine = unite(parent, mine, rt);   // after the first few edges most neighbours are joined already
  });
}

// one thread per row: no write to parent here, plain loads
__global__ __launch_bounds__(kRowThreads) void dbscan_flatten_kernel(const int32_t* __restrict__ parent, int64_t M,
                                                                     int32_t* __restrict__ root,
                                                                     int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (i > M) return;
  if (i == M) {   // the scan runs over M + 1 entries so that rank[M] is the number of all clusters
    flag[M] = 0;
    return;
  }
  int32_t x = (int32_t)i, q = parent[i];
  if (q < 0) {
    root[i] = -1;
    flag[i] = 0;
    return;
  }
  while ((uint32_t)q < (uint32_t)x) {   // q != x under 0 <= q <= x: strictly decreasing
    x = q;
    q = parent[x];
  }
  root[i] = x;
  flag[i] = x == (int32_t)i ? 1 : 0;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_label_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                      const int64_t* __restrict__ off, int64_t M,
                                                                      double r, double eps,
                                                                      const int32_t* __restrict__ root,
                                                                      const int32_t* __restrict__ rank,
                                                                      int32_t* __restrict__ labels, int32_t* sizes) {
  static_assert(kDbscanThreads == kWave, "the size adds are gathered per wave");
  const int64_t s = (int64_t)blockIdx.x * kDbscanThreads + threadIdx.x;
  int64_t slot = -1;   // where this row's cluster is counted; every lane stays for the ballots below
  if (s < M) {
    int64_t i, t0, t1;
    int b;
    double p[3];
    point_at(ix, xyz, s, i, b, p);
    frag_rows(off, b, M, t0, t1);
    int32_t rt = root[i];
    if (rt < 0) {
      int32_t best = 0x7fffffff;
      ball_walk(ix, xyz, b, p, r, eps, [&](int64_t t, int, double, double, double) {
        const int32_t q = root[t];
        if (q >= 0 && q < best) best = q;
      });
      rt = best == 0x7fffffff ? -1 : best;
    }
    const int32_t lab = rt < 0 ? -1 : rank[rt] - rank[t0];
    labels[i] = lab;
    if (lab >= 0 && t0 + lab < M) slot = t0 + lab;   // lab < n_clusters[b] <= n_b: inside the fragment's rows
  }
  if (!sizes) return;   // uniform
  unsigned long long left = __ballot(slot >= 0);
  while (left) {        // uniform; one round per distinct cluster among the wave's rows
    const int leader = __ffsll(left) - 1;
    const int64_t there = __shfl(slot, leader, kWave);
    const unsigned long long same = __ballot(slot == there);
    if (lane_id() == leader) atomicAdd(sizes + there, (int32_t)__popcll(same));
    left &= ~same;
  }
}

__global__ __launch_bounds__(kRowThreads) void dbscan_counts_kernel(const int64_t* __restrict__ off, int B, int64_t M,
                                                                    const int32_t* __restrict__ rank,
                                                                    int32_t* __restrict__ n_clusters) {
  const int b = blockIdx.x * kRowThreads + threadIdx.x;
  if (b >= B) return;
  int64_t t0, t1;
  frag_rows(off, b, M, t0, t1);
  n_clusters[b] = rank[t1] - rank[t0];
}

// parent, root, flag, rank: M + 1 int32 each, every one on a 256-byte boundary; then the scan's workspace
inline size_t dbscan_rows_bytes(int64_t M) { return (((size_t)(M > 0 ? M : 0) + 1) * 4 + 255) & ~(size_t)255; }
inline size_t dbscan_ws_bytes(int64_t M) {
  return 256 + 4 * dbscan_rows_bytes(M) + 256 + scan_ws_bytes((M > 0 ? M : 0) + 1);
}

}  // namespace mvr

extern "C" size_t mvr_dbscan_workspace_bytes(int64_t M) { return mvr::dbscan_ws_bytes(M); }

extern "C" int mvr_cluster_dbscan(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                                  int64_t M, double r_index, double eps, int min_points, int32_t* labels,
                                  int32_t* n_clusters, int32_t* sizes, uint8_t* core, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  using namespace mvr;
  if (!ball_values_ok(B, M, r_index, eps) || min_points < 1) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed, nothing is written
  if (!index_pointers_ok(index, index_bytes, xyz, off, M) || !labels || !n_clusters || !workspace ||
      workspace_bytes < dbscan_ws_bytes(M))
    return MVR_EINVAL;
  char* p = reinterpret_cast<char*>(workspace);
  const size_t rows = dbscan_rows_bytes(M), sc = scan_ws_bytes(M + 1);
  int32_t* parent = reinterpret_cast<int32_t*>(take(p, rows));
  int32_t* root = reinterpret_cast<int32_t*>(take(p, rows));
  int32_t* flag = reinterpret_cast<int32_t*>(take(p, rows));
  int32_t* rank = reinterpret_cast<int32_t*>(take(p, rows));
  void* tscan = take(p, sc);
  if (sizes && hipMemsetAsync(sizes, 0, (size_t)M * 4, stream) != hipSuccess) return MVR_ELAUNCH;
  int rc = launch_per_point<kDbscanThreads>(dbscan_core_kernel, index, M, 0, stream, xyz, M, r_index, eps, min_points,
                                            parent, core);
  if (rc != MVR_OK) return rc;
  rc = launch_per_point<kDbscanThreads>(dbscan_link_kernel, index, M, 0, stream, xyz, M, r_index, eps, parent);
  if (rc != MVR_OK) return rc;
  hipLaunchKernelGGL(dbscan_flatten_kernel, dim3((unsigned)((M + 1 + kRowThreads - 1) / kRowThreads)),
                     dim3(kRowThreads), 0, stream, parent, M, root, flag);
  MVR_CHECK_LAUNCH();
  if ((rc = excl_scan_i32(flag, rank, M + 1, tscan, sc, stream)) != MVR_OK) return rc;
  rc = launch_per_point<kDbscanThreads>(dbscan_label_kernel, index, M, 0, stream, xyz, off, M, r_index, eps,
                                        (const int32_t*)root, (const int32_t*)rank, labels, sizes);
  if (rc != MVR_OK) return rc;
  hipLaunchKernelGGL(dbscan_counts_kernel, dim3((unsigned)((B + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0,
                     stream, off, B, M, (const int32_t*)rank, n_clusters);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
