// Batched coloured ICP refinement on the radius index (mvreg.h mvr_icp_refine_colored): the loop of
// Open3D's registration_colored_icp (Park, Zhou, Koltun 2017), restated from the maths.  The search, the loop with its
// stopping rule, trace and status bits, the 6 x 6 solve and the update of T are icp_core.hpp's (the nearest target
// point, strict < max_dist, the lowest row on a tie, fitness and rmse on Euclidean distances); what an evaluation sums
// is icp_core.hpp's ColoredT: per match the point-to-plane term with the share lambda and a photometric term, the
// source's intensity against the target's first-order model of it in its tangent plane (color_grad.hip), with the
// share 1 - lambda.  On a plane the geometric term leaves the in-plane motion free and the photometric term fixes it.
//
// Two kernels: MVR_KERNEL_L2 runs the UnitWeight instantiation, where the weights are a type and nothing is generated
// for them; the four robust kernels share the KernelWeight one, the kernel a uniform run-time switch per term.
#include "icp_core.hpp"

namespace mvr {

// 16 waves, as the other ICP kernels: the search is the same chain of dependent loads (DESIGN.md 4.32 has the
// compiler's register, scratch and LDS figures)
#ifndef MVR_ICP_COLORED_THREADS
#define MVR_ICP_COLORED_THREADS 1024
#endif
constexpr int kColoredThreads = MVR_ICP_COLORED_THREADS;

template <class Model>
__global__ __launch_bounds__(kColoredThreads) void icp_colored_kernel(ColoredArgs a) {
  icp_loop<Model, kColoredThreads>(a);
}

}  // namespace mvr

extern "C" int mvr_icp_refine_colored(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                                      const double* intensity, const double* grad, const int64_t* off, int B,
                                      int64_t M, double r_index, const int64_t* pairs, const double* T0, int P,
                                      double max_dist, double lambda_geometric, int kernel, double kernel_k,
                                      int max_iters, double tol_fitness, double tol_rmse, double* T, double* fitness,
                                      double* rmse, int32_t* n_corr, int32_t* iters, int32_t* status, double* trace,
                                      double* w_sum, hipStream_t stream) {
  if (!(lambda_geometric >= 0.0) || !(lambda_geometric <= 1.0)) return MVR_EINVAL;
  if (kernel < MVR_KERNEL_L2 || kernel > MVR_KERNEL_TUKEY) return MVR_EINVAL;
  if (kernel != MVR_KERNEL_L2 && !(kernel_k > 0.0)) return MVR_EINVAL;
  mvr::ColoredArgs a;
  const int rc = mvr::icp_args(a, index, index_bytes, xyz, off, B, M, r_index, pairs, T0, P, max_dist, max_iters,
                               tol_fitness, tol_rmse, T, fitness, rmse, n_corr, iters, status, trace);
  if (rc != MVR_OK || P == 0) return rc;
  if (M > 0 && (!normals || !intensity || !grad)) return MVR_EINVAL;
  a.normals = normals;
  a.kernel = kernel;
  a.kernel_k = kernel_k;
  a.w_sum = w_sum;
  a.intensity = intensity;
  a.grad = grad;
  a.lambda = lambda_geometric;
  const dim3 grid(P), block(mvr::kColoredThreads);
  if (kernel == MVR_KERNEL_L2)
    hipLaunchKernelGGL(mvr::icp_colored_kernel<mvr::ColoredT<mvr::UnitWeight>>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(mvr::icp_colored_kernel<mvr::ColoredT<mvr::KernelWeight>>, grid, block, 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
