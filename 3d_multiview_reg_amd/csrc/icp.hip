// Batched point-to-point ICP refinement on the radius index of overlap.hip (mvreg.h mvr_icp_refine).
// The reference stops at the coarse estimate (weighted Procrustes / RANSAC over 5000 correspondences); this is the
// fine registration on the fragments' own points that Open3D's registration_icp does after it, restated from the
// maths: nearest target point per transformed source point, unweighted Kabsch on the pairs closer than max_dist.
//
// One 1024-thread workgroup per pair, every iteration inside the one launch, fp64 throughout.  The search, the loop
// and the reduction are icp_core.hpp's; this file's own is:
//   sums     count, sum d^2, sum x, sum y, sum x y^T per thread in registers, relative to a per-pair origin (the
//            source fragment's first point and its image under T0), so that sum x y^T - n mx my^T cancels little
//   solve    lane 0: centred covariance from the sums, jacobi_svd3, det-corrected R, t; broadcast through LDS
// Every loop is bounded: max_iters, the Jacobi sweep cap, and the hash probe (cap >= 2 M ends it at an empty slot).
#include "icp_core.hpp"
#include "svd3.hpp"

namespace mvr {

// 16 waves = 4 per SIMD: a query is a chain of dependent loads (hash slot -> cell range -> row -> point), and the
// other waves are what hides it.  128 VGPRs at this size, 13 of them spilled (once per query, outside the cell and
// candidate loops); 512 and 256 threads need no spill and measure 1.5 and 1.8 times slower
#ifndef MVR_ICP_THREADS
#define MVR_ICP_THREADS 1024
#endif
constexpr int kIcpThreads = MVR_ICP_THREADS;

struct PointToPoint {
  static constexpr int kSums = 17;   // n, sum d^2, sum x [3], sum y [3], sum x y^T [9]
  static constexpr int kMinCorr = 3, kOrigin = 6;   // the origins of the sums: source side, target side
  static constexpr bool kCanFail = false;

  __device__ __forceinline__ static void origin(const IcpArgs& a, const PairRange& g, const double* T0, double* sO) {
    double o[3] = {0.0, 0.0, 0.0};
    if (g.s0 < g.s1)
      for (int e = 0; e < 3; ++e) o[e] = a.xyz[3 * g.s0 + e];
    for (int e = 0; e < 3; ++e) {
      sO[e] = o[e];
      sO[3 + e] = T0[4 * e] * o[0] + T0[4 * e + 1] * o[1] + T0[4 * e + 2] * o[2] + T0[4 * e + 3];
    }
  }

  __device__ __forceinline__ static void accumulate(const IcpArgs& a, const double* sT, const double* sO,
                                                    double (&v)[kSums], int64_t i, int64_t bt, const double (&q)[3]) {
    // x is read again (moved_point had it): the same values, and no register held across the search for it
    const double xr[3] = {a.xyz[3 * i] - sO[0], a.xyz[3 * i + 1] - sO[1], a.xyz[3 * i + 2] - sO[2]};
    const double yr[3] = {a.xyz[3 * bt] - sO[3], a.xyz[3 * bt + 1] - sO[4], a.xyz[3 * bt + 2] - sO[5]};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      v[2 + e] += xr[e];
      v[5 + e] += yr[e];
#pragma unroll
      for (int f = 0; f < 3; ++f) v[8 + 3 * e + f] += xr[e] * yr[f];
    }
  }

  // argmin |R x + t - y|^2 over the valid pairs, on the original source points
  __device__ __forceinline__ static bool solve(const double (&v)[kSums], double* sT, const double* sO) {
    double mx[3], my[3], H[3][3], U[3][3], S[3], V[3][3];
    for (int e = 0; e < 3; ++e) { mx[e] = v[2 + e] / v[0]; my[e] = v[5 + e] / v[0]; }
    for (int e = 0; e < 3; ++e)
      for (int f = 0; f < 3; ++f) H[e][f] = v[8 + 3 * e + f] - v[0] * mx[e] * my[f];
    jacobi_svd3(H, U, S, V);
    const double d = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int e = 0; e < 3; ++e) {
      double R[3];
      for (int f = 0; f < 3; ++f) R[f] = V[e][0] * U[f][0] + V[e][1] * U[f][1] + d * V[e][2] * U[f][2];
      for (int f = 0; f < 3; ++f) sT[4 * e + f] = R[f];
      sT[4 * e + 3] = (my[e] + sO[3 + e]) - (R[0] * (mx[0] + sO[0]) + R[1] * (mx[1] + sO[1]) + R[2] * (mx[2] + sO[2]));
    }
    return true;
  }
};

__global__ __launch_bounds__(kIcpThreads) void icp_kernel(IcpArgs a) { icp_loop<PointToPoint, kIcpThreads>(a); }

}  // namespace mvr

extern "C" int mvr_icp_refine(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                              int64_t M, double r_index, const int64_t* pairs, const double* T0, int P,
                              double max_dist, int max_iters, double tol_fitness, double tol_rmse, double* T,
                              double* fitness, double* rmse, int32_t* n_corr, int32_t* iters, int32_t* status,
                              double* trace, hipStream_t stream) {
  mvr::IcpArgs a;
  const int rc = mvr::icp_args(a, index, index_bytes, xyz, off, B, M, r_index, pairs, T0, P, max_dist, max_iters,
                               tol_fitness, tol_rmse, T, fitness, rmse, n_corr, iters, status, trace);
  if (rc != MVR_OK || P == 0) return rc;
  hipLaunchKernelGGL(mvr::icp_kernel, dim3(P), dim3(mvr::kIcpThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
