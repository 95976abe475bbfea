// Per-point intensity and its gradient in the tangent plane, on the radius index of overlap.hip (mvreg.h
// mvr_color_gradient): what Open3D's coloured ICP prepares on its target
// (InitializePointCloudForColoredICP), restated from the maths.  The intensity is the mean of the three colour
// channels.  Over the neighbours x_j of x_i (its fragment's points closer than `radius`, itself among them) the
// gradient d solves, in the least-squares sense, u_j . d = I_j - I_i with u_j the part of x_j - x_i in the tangent
// plane of the normal n, plus the row (n_nbr - 1) n . d = 0 that keeps d in that plane: written as the 3 x 3 normal
// equations A d = h and solved by Cholesky.  Fewer than 4 neighbours or a failed pivot: gradient 0.
//
// One thread per point in the index's sorted order, as normals.hip: fp64 throughout, no atomics, no LDS and no
// workspace; the sums run in the order of the index's walk, so a point's bits depend on its fragment only.  Every
// loop is bounded: 27 cells, a cell's rows, the hash probe (cap >= 2 M).
#include "common.hpp"
#include "cov3.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// nothing is shared between a workgroup's waves, so the smallest, as normals.hip (DESIGN.md 4.32 has the A/B)
#ifndef MVR_COLOR_GRAD_THREADS
#define MVR_COLOR_GRAD_THREADS 64
#endif
constexpr int kColorGradThreads = MVR_COLOR_GRAD_THREADS;

__device__ __forceinline__ double intensity_of(const double* __restrict__ colors, int64_t i) {
  return (colors[3 * i] + colors[3 * i + 1] + colors[3 * i + 2]) / 3.0;
}

// d <- A^-1 h by Cholesky, A by its upper triangle xx xy xz yy yz zz.  false: a pivot is not above 1e-12 of the
// largest diagonal entry (a NaN fails the test too)
__device__ __forceinline__ bool solve3(const double (&A)[6], const double (&h)[3], double (&d)[3]) {
  const double floor_ = 1e-12 * fmax(fmax(A[0], A[3]), A[5]);
  if (!(A[0] > floor_)) return false;
  const double l00 = sqrt(A[0]), l10 = A[1] / l00, l20 = A[2] / l00;
  const double p1 = A[3] - l10 * l10;
  if (!(p1 > floor_)) return false;
  const double l11 = sqrt(p1), l21 = (A[4] - l20 * l10) / l11;
  const double p2 = A[5] - l20 * l20 - l21 * l21;
  if (!(p2 > floor_)) return false;
  const double l22 = sqrt(p2);
  const double y0 = h[0] / l00, y1 = (h[1] - l10 * y0) / l11, y2 = (h[2] - l20 * y0 - l21 * y1) / l22;
  d[2] = y2 / l22;
  d[1] = (y1 - l21 * d[2]) / l11;
  d[0] = (y0 - l10 * d[1] - l20 * d[2]) / l00;
  return true;
}

__global__ __launch_bounds__(kColorGradThreads) void color_grad_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                       const double* __restrict__ normals,
                                                                       const double* __restrict__ colors, int64_t M,
                                                                       double r, double radius,
                                                                       double* __restrict__ intensity,
                                                                       double* __restrict__ grad,
                                                                       int32_t* __restrict__ n_nbr) {
  const int64_t s = (int64_t)blockIdx.x * kColorGradThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b, n;
  double p[3], A[6], h[3];
  point_at(ix, xyz, s, i, b, p);
  const double nv[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  const double f0 = intensity_of(colors, i);
  ball_tangent_sums(ix, xyz, b, p, nv, f0, r, radius, [&](int64_t t) { return intensity_of(colors, t); }, n, A, h);
  double d[3] = {0.0, 0.0, 0.0};
  if (n >= 4) {
    const double k2 = (double)(n - 1) * (double)(n - 1);   // the row (n_nbr - 1) n . d = 0
    A[0] += k2 * nv[0] * nv[0]; A[1] += k2 * nv[0] * nv[1]; A[2] += k2 * nv[0] * nv[2];
    A[3] += k2 * nv[1] * nv[1]; A[4] += k2 * nv[1] * nv[2]; A[5] += k2 * nv[2] * nv[2];
    double sol[3];
    if (solve3(A, h, sol) && isfinite(sol[0]) && isfinite(sol[1]) && isfinite(sol[2]))
      for (int e = 0; e < 3; ++e) d[e] = sol[e];
  }
  intensity[i] = f0;
  for (int e = 0; e < 3; ++e) grad[3 * i + e] = d[e];
  if (n_nbr) n_nbr[i] = n;
}

}  // namespace mvr

extern "C" int mvr_color_gradient(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                                  const double* colors, const int64_t* off, int B, int64_t M, double r_index,
                                  double radius, double* intensity, double* grad, int32_t* n_nbr,
                                  hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, radius)) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !normals || !colors || !intensity || !grad)
    return MVR_EINVAL;
  return mvr::launch_per_point<mvr::kColorGradThreads>(mvr::color_grad_kernel, index, M, 0, stream, xyz, normals, colors,
                                                       M, r_index, radius, intensity, grad, n_nbr);
}
