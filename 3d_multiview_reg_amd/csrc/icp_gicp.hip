// Batched generalized (plane-to-plane) ICP refinement on the radius index (mvreg.h mvr_icp_refine_generalized;
// DESIGN.md 4.23): the loop of Segal et al.'s GICP, Open3D's registration_generalized_icp, restated from the maths,
// beside the point-to-plane form of icp_plane.hip.  The search, the loop with its stopping rule, the trace, the status
// bits, the origin c, the 6 x 6 solve and the update of T are icp_core.hpp's, shared with that file.  What differs is
// what a match adds to the sums: icp_core.hpp's GeneralizedT, shared with icp_robust.hip.
//
// A point with unit normal n has covariance I - (1 - eps) n n^T: 1 in the surface, eps along the normal.  For a source
// point x matched with y (q = T x, R the rotation of T, n the normal of y, m = R n_s with n_s the normal of x):
//   M = 2 I - (1 - eps)(n n^T + m m^T)    A = M^-1 (symmetric; by cofactors)
//   G = [-[q - c]x | I]                   d = q - y
//   H = sum G^T A G                       g = sum G^T A d                xi = -H^-1 g
// With S = [q - c]x: G^T A G = [[S A S^T, S A], [(S A)^T, A]] and G^T A d = [S (A d), A d].
//
// Per match, in registers: the two normals are loaded, n_s rotated, M inverted and the products formed only once a
// match is found, so nothing of it is live across the search.  A non-finite A, from normals that are not unit, ends the
// loop at the solve's pivot test with status bit 8 and T kept.
#include "icp_core.hpp"

namespace mvr {

// 16 waves, as icp.hip and icp_plane.hip: the search is a chain of dependent loads that only other waves hide, and
// the search is the same code (DESIGN.md 4.23 has the compiler's register, scratch and LDS figures)
#ifndef MVR_ICP_GICP_THREADS
#define MVR_ICP_GICP_THREADS 1024
#endif
constexpr int kGicpThreads = MVR_ICP_GICP_THREADS;

using Generalized = GeneralizedT<UnitWeight>;   // icp_core.hpp

__global__ __launch_bounds__(kGicpThreads) void icp_gicp_kernel(IcpArgs a) { icp_loop<Generalized, kGicpThreads>(a); }

}  // namespace mvr

extern "C" int mvr_icp_refine_generalized(const void* index, size_t index_bytes, const double* xyz,
                                          const double* normals, const int64_t* off, int B, int64_t M, double r_index,
                                          const int64_t* pairs, const double* T0, int P, double max_dist,
                                          double epsilon, int max_iters, double tol_fitness, double tol_rmse, double* T,
                                          double* fitness, double* rmse, int32_t* n_corr, int32_t* iters,
                                          int32_t* status, double* trace, hipStream_t stream) {
  if (!(epsilon > 0.0) || !(epsilon <= 1.0)) return MVR_EINVAL;
  mvr::IcpArgs a;
  const int rc = mvr::icp_args(a, index, index_bytes, xyz, off, B, M, r_index, pairs, T0, P, max_dist, max_iters,
                               tol_fitness, tol_rmse, T, fitness, rmse, n_corr, iters, status, trace);
  if (rc != MVR_OK || P == 0) return rc;
  if (M > 0 && !normals) return MVR_EINVAL;
  a.normals = normals;
  a.epsilon = epsilon;
  hipLaunchKernelGGL(mvr::icp_gicp_kernel, dim3(P), dim3(mvr::kGicpThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
