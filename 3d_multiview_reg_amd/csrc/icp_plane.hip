// Batched point-to-plane ICP refinement on the radius index (mvreg.h mvr_icp_refine_plane): the
// loop of Open3D's registration_icp with TransformationEstimationPointToPlane, restated from the maths, beside the
// point-to-point form of icp.hip.  The search, the loop with its stopping rule, the 6 x 6 solve and the update of T
// are icp_core.hpp's (the nearest target point, strict < max_dist, the lowest row on a tie, fitness and rmse on
// Euclidean distances); what an evaluation sums is icp_core.hpp's PointToPlaneT, shared with icp_robust.hip.
//
// Per match, in registers: of a = [(q - c) x n, n], b = (q - y) . n (n the normal of the match y, c the target
// fragment's first point) the upper triangle of sum a a^T (21) and sum a b (6).  Lane 0 solves xi = -H^-1 g from
// them; a pivot that fails pivot > 1e-12 max H_ii ends the loop with status bit 8 and T kept.
#include "icp_core.hpp"

namespace mvr {

// 16 waves, as icp.hip: the search is a chain of dependent loads that only other waves hide.  128 VGPRs at this size
// with 38 spilled (108 B scratch per lane, touched per query around the search, not per candidate);
// 512 and 256 threads (179 VGPRs, no spill, 2 waves per SIMD) measure 1.5 and 1.7 times slower
#ifndef MVR_ICP_PLANE_THREADS
#define MVR_ICP_PLANE_THREADS 1024
#endif
constexpr int kPlaneThreads = MVR_ICP_PLANE_THREADS;

using PointToPlane = PointToPlaneT<UnitWeight>;   // icp_core.hpp

__global__ __launch_bounds__(kPlaneThreads) void icp_plane_kernel(IcpArgs a) {
  icp_loop<PointToPlane, kPlaneThreads>(a);
}

}  // namespace mvr

extern "C" int mvr_icp_refine_plane(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                                    const int64_t* off, int B, int64_t M, double r_index, const int64_t* pairs,
                                    const double* T0, int P, double max_dist, int max_iters, double tol_fitness,
                                    double tol_rmse, double* T, double* fitness, double* rmse, int32_t* n_corr,
                                    int32_t* iters, int32_t* status, double* trace, hipStream_t stream) {
  mvr::IcpArgs a;
  const int rc = mvr::icp_args(a, index, index_bytes, xyz, off, B, M, r_index, pairs, T0, P, max_dist, max_iters,
                               tol_fitness, tol_rmse, T, fitness, rmse, n_corr, iters, status, trace);
  if (rc != MVR_OK || P == 0) return rc;
  if (M > 0 && !normals) return MVR_EINVAL;
  a.normals = normals;
  hipLaunchKernelGGL(mvr::icp_plane_kernel, dim3(P), dim3(mvr::kPlaneThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
