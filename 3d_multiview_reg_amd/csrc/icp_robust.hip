// Robust kernels on the three batched ICP variants (mvreg.h mvr_icp_refine_robust): what Open3D's
// RobustKernel does to registration_icp and registration_generalized_icp, restated from the maths.  Every valid
// correspondence gets the weight w(r) of its residual at the T its solve starts from, one IRLS step per iteration.
//
// The search, the loop with its stopping rule, trace and status bits, the models and their solves are icp_core.hpp's,
// shared with icp.hip, icp_plane.hip and icp_gicp.hip: this file instantiates the three models with KernelWeight
// instead of UnitWeight.  A model then multiplies what a match adds to its sums with w, keeps sum w as one more sum,
// and the loop writes it to w_sum.  The weight is computed per match after the search, from values the model has
// anyway (d^2, b, A d): nothing of it is live across the search's loops.
//
// One kernel per method, the robust kernel a uniform run-time switch in KernelWeight::weight (three kernels, not
// fifteen): the switch is a few scalar branches per match beside a search of dozens of dependent loads, and L2 through
// this entry runs the very code the other four kernels run, with w == 1.0, which is what pins it bit for bit to the
// plain entries (x * 1.0 == x; every product keeps its shape, (w a_f) a_g into the same FMA).
#include "icp_core.hpp"

namespace mvr {

// 16 waves, as the three plain kernels: the search is the same chain of dependent loads (DESIGN.md 4.30 has the
// compiler's register, scratch and LDS figures beside theirs)
#ifndef MVR_ICP_ROBUST_THREADS
#define MVR_ICP_ROBUST_THREADS 1024
#endif
constexpr int kRobustThreads = MVR_ICP_ROBUST_THREADS;

template <class Model>
__global__ __launch_bounds__(kRobustThreads) void icp_robust_kernel(RobustArgs a) {
  icp_loop<Model, kRobustThreads>(a);
}

}  // namespace mvr

extern "C" int mvr_icp_refine_robust(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                                     const int64_t* off, int B, int64_t M, double r_index, const int64_t* pairs,
                                     const double* T0, int P, int method, double max_dist, double epsilon, int kernel,
                                     double kernel_k, int max_iters, double tol_fitness, double tol_rmse, double* T,
                                     double* fitness, double* rmse, int32_t* n_corr, int32_t* iters, int32_t* status,
                                     double* trace, double* w_sum, hipStream_t stream) {
  if (method < MVR_ICP_POINT_TO_POINT || method > MVR_ICP_GENERALIZED) return MVR_EINVAL;
  if (kernel < MVR_KERNEL_L2 || kernel > MVR_KERNEL_TUKEY) return MVR_EINVAL;
  if (kernel != MVR_KERNEL_L2 && !(kernel_k > 0.0)) return MVR_EINVAL;
  if (method == MVR_ICP_GENERALIZED && (!(epsilon > 0.0) || !(epsilon <= 1.0))) return MVR_EINVAL;
  mvr::RobustArgs a;
  const int rc = mvr::icp_args(a, index, index_bytes, xyz, off, B, M, r_index, pairs, T0, P, max_dist, max_iters,
                               tol_fitness, tol_rmse, T, fitness, rmse, n_corr, iters, status, trace);
  if (rc != MVR_OK || P == 0) return rc;
  if (method != MVR_ICP_POINT_TO_POINT && M > 0 && !normals) return MVR_EINVAL;
  a.normals = normals;
  a.epsilon = epsilon;
  a.kernel = kernel;
  a.kernel_k = kernel_k;
  a.w_sum = w_sum;
  const dim3 grid(P), block(mvr::kRobustThreads);
  if (method == MVR_ICP_POINT_TO_POINT)
    hipLaunchKernelGGL(mvr::icp_robust_kernel<mvr::PointToPointT<mvr::KernelWeight>>, grid, block, 0, stream, a);
  else if (method == MVR_ICP_POINT_TO_PLANE)
    hipLaunchKernelGGL(mvr::icp_robust_kernel<mvr::PointToPlaneT<mvr::KernelWeight>>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(mvr::icp_robust_kernel<mvr::GeneralizedT<mvr::KernelWeight>>, grid, block, 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
