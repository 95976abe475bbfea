// ISS keypoints on the radius index of overlap.hip (mvreg.h mvr_iss_saliency, mvr_radius_nms):
// Open3D's ComputeISSKeypoints (Intrinsic Shape Signatures, Zhong 2009) restated from the maths, in two launches.
// iss_saliency_kernel: the eigenvalues l1 >= l2 >= l3 of the covariance of a point's ball and the ISS rule on them,
// by products instead of Open3D's quotients; the saliency of a candidate is l3, of every other point exactly -1.
// radius_nms_kernel: non-maximum suppression of any per-point score over a ball, ties to the lower row.
//
// Both: one thread per point, fp64 throughout, no atomics, no workspace and no LDS.  Thread s takes the point at
// position s of the index's sorted order, so a wave's threads sit in a few neighbouring cells and read the same
// rows; the walk follows the index alone, so a point's bits depend on its fragment only.  Every loop is bounded: 27
// cells, a cell's rows, the Jacobi sweep cap, and the hash probe (cap >= 2 M).
#include "common.hpp"
#include "cov3.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// Threads per workgroup: 64, 128 and 256 measure the same (611,804 points, radius 0.075 / 0.05, medians of 7 in one
// process each: saliency 0.561 / 0.557 / 0.564 ms, NMS 0.552 / 0.558 / 0.567 ms, a second run at 64: 0.569 / 0.554;
// DESIGN.md 4.29).  Nothing is shared between a workgroup's waves, so the smallest, as normals.hip.
// 72 and 48 VGPRs, no scratch, no LDS
#ifndef MVR_ISS_THREADS
#define MVR_ISS_THREADS 64
#endif
#ifndef MVR_NMS_THREADS
#define MVR_NMS_THREADS 64
#endif
constexpr int kIssThreads = MVR_ISS_THREADS;
constexpr int kNmsThreads = MVR_NMS_THREADS;

__global__ __launch_bounds__(kIssThreads) void iss_saliency_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                   int64_t M, double r, double radius, double gamma_21,
                                                                   double gamma_32, double min_ratio,
                                                                   int min_neighbors, double* __restrict__ saliency,
                                                                   int32_t* __restrict__ n_nbr) {
  const int64_t s = (int64_t)blockIdx.x * kIssThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b, n;
  double p[3], m[3], S[6];
  point_at(ix, xyz, s, i, b, p);
  ball_sums(ix, xyz, b, p, r, radius, n, m, S);
  double sal = -1.0;
  if (n >= min_neighbors) {   // min_neighbors >= 1, and the point is in its own ball
    double a[3][3];
    ball_covariance(n, m, S, a);
    jacobi_eigvals3(a);   // the eigenvectors are not needed: 9 accumulators fewer than the normals carry
    double l1 = a[0][0], l2 = a[1][1], l3 = a[2][2], t;
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    if (l2 < l3) { t = l2; l2 = l3; l3 = t; }
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    // a NaN eigenvalue fails every comparison: not a candidate
    if (l3 > min_ratio * l1 && l2 < gamma_21 * l1 && l3 < gamma_32 * l2) sal = l3;
  }
  saliency[i] = sal;
  if (n_nbr) n_nbr[i] = n;
}

__global__ __launch_bounds__(kNmsThreads) void radius_nms_kernel(RIndex ix, const double* __restrict__ xyz, int64_t M,
                                                                 double r, double radius, int min_neighbors,
                                                                 const double* __restrict__ score,
                                                                 uint8_t* __restrict__ keep) {
  const int64_t s = (int64_t)blockIdx.x * kNmsThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b, n = 0;
  double p[3];
  point_at(ix, xyz, s, i, b, p);
  const double si = score[i];
  bool beaten = false;
  // every row t is a row of xyz below M (the index holds nothing else), so score[t] is in bounds
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t t, int, double, double, double) {
    ++n;
    const double sj = score[t];
    if (t != i && (sj > si || (sj == si && t < i))) beaten = true;   // a NaN on either side: false
  });
  keep[i] = (si > 0.0 && n >= min_neighbors && !beaten) ? 1 : 0;
}

}  // namespace mvr

extern "C" int mvr_iss_saliency(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                                int64_t M, double r_index, double salient_radius, double gamma_21, double gamma_32,
                                double min_ratio, int min_neighbors, double* saliency, int32_t* n_nbr,
                                hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, salient_radius) || min_neighbors < 1) return MVR_EINVAL;
  if (!(gamma_21 > 0.0) || gamma_21 > 1.0 || !(gamma_32 > 0.0) || gamma_32 > 1.0) return MVR_EINVAL;
  if (!(min_ratio >= 0.0) || !(min_ratio < 1.0)) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !saliency) return MVR_EINVAL;
  return mvr::launch_per_point<mvr::kIssThreads>(mvr::iss_saliency_kernel, index, M, 0, stream, xyz, M, r_index,
                                                 salient_radius, gamma_21, gamma_32, min_ratio, min_neighbors, saliency,
                                                 n_nbr);
}

extern "C" int mvr_radius_nms(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                              int64_t M, double r_index, double radius, int min_neighbors, const double* score,
                              uint8_t* keep, hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, radius) || min_neighbors < 1) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !score || !keep) return MVR_EINVAL;
  return mvr::launch_per_point<mvr::kNmsThreads>(mvr::radius_nms_kernel, index, M, 0, stream, xyz, M, r_index, radius,
                                                 min_neighbors, score, keep);
}
