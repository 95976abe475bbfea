// Batched point-to-point ICP refinement on the radius index of overlap.hip (mvreg.h mvr_icp_refine).
// The reference stops at the coarse estimate (weighted Procrustes / RANSAC over 5000 correspondences); this is the
// fine registration on the fragments' own points that Open3D's registration_icp does after it, restated from the
// maths: nearest target point per transformed source point, unweighted Kabsch on the pairs closer than max_dist.
//
// One 1024-thread workgroup per pair, every iteration inside the one launch, fp64 throughout.  The search, the loop
// and the reduction are icp_core.hpp's, and so is the model, PointToPointT, shared with icp_robust.hip:
//   sums     count, sum d^2, sum x, sum y, sum x y^T per thread in registers, relative to a per-pair origin (the
//            source fragment's first point and its image under T0), so that sum x y^T - n mx my^T cancels little
//   solve    lane 0: centred covariance from the sums, jacobi_svd3, det-corrected R, t; broadcast through LDS
// Every loop is bounded: max_iters, the Jacobi sweep cap, and the hash probe (cap >= 2 M ends it at an empty slot).
#include "icp_core.hpp"

namespace mvr {

// 16 waves = 4 per SIMD: a query is a chain of dependent loads (hash slot -> cell range -> row -> point), and the
// other waves are what hides it.  128 VGPRs at this size, 13 of them spilled (once per query, outside the cell and
// candidate loops); 512 and 256 threads need no spill and measure 1.5 and 1.8 times slower
#ifndef MVR_ICP_THREADS
#define MVR_ICP_THREADS 1024
#endif
constexpr int kIcpThreads = MVR_ICP_THREADS;

using PointToPoint = PointToPointT<UnitWeight>;   // icp_core.hpp

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
