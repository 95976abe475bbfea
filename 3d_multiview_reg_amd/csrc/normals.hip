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

// One Jacobi rotation of the symmetric a that zeroes a[P][Q]; R is the third index.  V <- V J.
template <int P, int Q, int R>
__device__ __forceinline__ void sym_rotate(double (&a)[3][3], double (&V)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0 || fabs(apq) <= 1e-17 * (fabs(a[P][P]) + fabs(a[Q][Q]))) return;
  const double th = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vp = V[i][P], vq = V[i][Q];
    V[i][P] = c * vp - s * vq;
    V[i][Q] = s * vp + c * vq;
  }
}

// The symmetric (two-sided) form of svd3.hpp's cyclic Jacobi: eigenvalues on the diagonal of a, eigenvectors in the
// columns of V.  Zero off-diagonals are left alone, so a zero row and column keep their axis exactly.
__device__ __forceinline__ void jacobi_eig3(double (&a)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (!(off > 1e-17 * (fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2])))) break;
    sym_rotate<0, 1, 2>(a, V);
    sym_rotate<0, 2, 1>(a, V);
    sym_rotate<1, 2, 0>(a, V);
  }
}

__global__ __launch_bounds__(kNormalsThreads) void normals_kernel(RIndex ix, const double* __restrict__ xyz, int64_t M,
                                                                  double r, double radius,
                                                                  const double* __restrict__ viewpoints,
                                                                  double* __restrict__ normals,
                                                                  int32_t* __restrict__ n_nbr) {
  const int64_t s = (int64_t)blockIdx.x * kNormalsThreads + threadIdx.x;
  if (s >= M) return;
  const int64_t i = ix.sidx[s];
  const int b = (int)(ix.skey[s] >> (3 * OV_BITS));
  const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  int n = 0;
  double m[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sum e; sum e e^T: xx xy xz yy yz zz
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t, double ex, double ey, double ez) {
    ++n;
    m[0] += ex; m[1] += ey; m[2] += ez;
    S[0] += ex * ex; S[1] += ex * ey; S[2] += ex * ez;
    S[3] += ey * ey; S[4] += ey * ez; S[5] += ez * ez;
  });
  double nv[3] = {0.0, 0.0, 1.0};
  if (n >= 3) {
    const double inv = 1.0 / (double)n;
    for (int e = 0; e < 3; ++e) m[e] *= inv;
    double a[3][3], V[3][3];
    a[0][0] = S[0] * inv - m[0] * m[0];
    a[0][1] = a[1][0] = S[1] * inv - m[0] * m[1];
    a[0][2] = a[2][0] = S[2] * inv - m[0] * m[2];
    a[1][1] = S[3] * inv - m[1] * m[1];
    a[1][2] = a[2][1] = S[4] * inv - m[1] * m[2];
    a[2][2] = S[5] * inv - m[2] * m[2];
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
  if (M < 0 || M > 0x7fffffff || B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (!(radius > 0.0) || !(r_index > 0.0) || radius > r_index) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!index || !xyz || !off || !normals || index_bytes < mvr_radius_index_bytes(M)) return MVR_EINVAL;
  const mvr::RIndex ix = mvr::index_view(const_cast<void*>(index), M);
  const unsigned blocks = (unsigned)((M + mvr::kNormalsThreads - 1) / mvr::kNormalsThreads);
  hipLaunchKernelGGL(mvr::normals_kernel, dim3(blocks), dim3(mvr::kNormalsThreads), 0, stream, ix, xyz, M, r_index,
                     radius, viewpoints, normals, n_nbr);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
