// Per-point normals on the radius index of overlap.hip (mvreg.h mvr_estimate_normals): Open3D's
// estimate_normals(KDTreeSearchParamRadius(radius)) restated from the maths.  The neighbours of a point are the
// points of its own fragment closer than `radius` (the point itself among them); the normal is the unit eigenvector
// of the smallest eigenvalue of their covariance, (0, 0, 1) below three neighbours.
//
// One thread per point, fp64 throughout, no atomics and no workspace.  Thread s takes the point at position s of the
// index's sorted order, so a wave's threads sit in a few neighbouring cells and read the same rows; the walk over the
// 27 cells and over a cell's rows follows the index alone, so a point's bits depend on its fragment only.
// Coordinates are taken relative to the point: the covariance cancels at the size of the ball, not of the scene.
// Every loop is bounded: 27 cells, a cell's rows, the Jacobi sweep cap, and the hash probe (cap >= 2 M).
#include "common.hpp"
#include "cov3.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// 64, 128 and 256 threads measure the same (0.64 ms for 611,804 points): nothing is shared between
// a workgroup's waves, so the smallest.  94 VGPRs, no scratch, no LDS
#ifndef MVR_NORMALS_THREADS
#define MVR_NORMALS_THREADS 64
#endif
constexpr int kNormalsThreads = MVR_NORMALS_THREADS;

__global__ __launch_bounds__(kNormalsThreads) void normals_kernel(RIndex ix, const double* __restrict__ xyz, int64_t M,
                                                                  double r, double radius,
                                                                  const double* __restrict__ viewpoints,
                                                                  double* __restrict__ normals,
                                                                  int32_t* __restrict__ n_nbr) {
  const int64_t s = (int64_t)blockIdx.x * kNormalsThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b, n;
  double p[3];
  point_at(ix, xyz, s, i, b, p);
  double m[3], S[6];   // sum e; sum e e^T: xx xy xz yy yz zz
  ball_sums(ix, xyz, b, p, r, radius, n, m, S);
  double nv[3] = {0.0, 0.0, 1.0};
  if (n >= 3) {
    double a[3][3], V[3][3];
    ball_covariance(n, m, S, a);
    jacobi_eig3(a, V);
    // the column of the smallest eigenvalue; on equal values the last axis, as (0, 0, 1) is the default
    double v[3] = {V[0][2], V[1][2], V[2][2]}, lam = a[2][2];
    if (a[1][1] < lam) { lam = a[1][1]; v[0] = V[0][1]; v[1] = V[1][1]; v[2] = V[2][1]; }
    if (a[0][0] < lam) { lam = a[0][0]; v[0] = V[0][0]; v[1] = V[1][0]; v[2] = V[2][0]; }
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (len > 0.0)
      for (int e = 0; e < 3; ++e) nv[e] = v[e] / len;
  }
  if (viewpoints) {
    const double* vp = viewpoints + 3 * (int64_t)b;
    if (nv[0] * (vp[0] - p[0]) + nv[1] * (vp[1] - p[1]) + nv[2] * (vp[2] - p[2]) < 0.0)
      for (int e = 0; e < 3; ++e) nv[e] = -nv[e];
  }
  for (int e = 0; e < 3; ++e) normals[3 * i + e] = nv[e];
  if (n_nbr) n_nbr[i] = n;
}

}  // namespace mvr

extern "C" int mvr_estimate_normals(const void* index, size_t index_bytes, const double* xyz, const int64_t* off,
                                    int B, int64_t M, double r_index, double radius, const double* viewpoints,
                                    double* normals, int32_t* n_nbr, hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, radius)) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !normals) return MVR_EINVAL;
  return mvr::launch_per_point<mvr::kNormalsThreads>(mvr::normals_kernel, index, M, 0, stream, xyz, M, r_index, radius,
                                                     viewpoints, normals, n_nbr);
}
