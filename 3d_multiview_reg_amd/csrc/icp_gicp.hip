// Batched generalized (plane-to-plane) ICP refinement on the radius index (mvreg.h mvr_icp_refine_generalized;
// DESIGN.md 4.23): the loop of Segal et al.'s GICP, Open3D's registration_generalized_icp, restated from the maths,
// beside the point-to-plane form of icp_plane.hip.  The search, the loop with its stopping rule, the trace, the status
// bits, the origin c, the 6 x 6 solve and the update of T are icp_core.hpp's, shared with that file.  What differs is
// what a match adds to the sums.
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

struct Generalized : SixDofModel {   // the sums: n, sum d^2, upper triangle of sum G^T A G [21], sum G^T A d [6]
  __device__ __forceinline__ static void accumulate(const IcpArgs& a, const double* sT, const double* sC,
                                                    double (&v)[kSums], int64_t i, int64_t bt, const double (&q)[3]) {
    const double ome = 1.0 - a.epsilon;
    const double n[3] = {a.normals[3 * bt], a.normals[3 * bt + 1], a.normals[3 * bt + 2]};
    const double sx = a.normals[3 * i], sy = a.normals[3 * i + 1], sz = a.normals[3 * i + 2];
    const double m[3] = {sT[0] * sx + sT[1] * sy + sT[2] * sz, sT[4] * sx + sT[5] * sy + sT[6] * sz,
                         sT[8] * sx + sT[9] * sy + sT[10] * sz};
    // M = 2 I - (1 - eps)(n n^T + m m^T) by its upper triangle (00 01 02 11 12 22), A = adj(M) / det(M)
    const double m00 = 2.0 - ome * (n[0] * n[0] + m[0] * m[0]), m01 = -ome * (n[0] * n[1] + m[0] * m[1]),
                 m02 = -ome * (n[0] * n[2] + m[0] * m[2]), m11 = 2.0 - ome * (n[1] * n[1] + m[1] * m[1]),
                 m12 = -ome * (n[1] * n[2] + m[1] * m[2]), m22 = 2.0 - ome * (n[2] * n[2] + m[2] * m[2]);
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double inv = 1.0 / (m00 * c00 + m01 * c01 + m02 * c02);
    const double A[3][3] = {{c00 * inv, c01 * inv, c02 * inv},
                            {c01 * inv, (m00 * m22 - m02 * m02) * inv, (m01 * m02 - m00 * m12) * inv},
                            {c02 * inv, (m01 * m02 - m00 * m12) * inv, (m00 * m11 - m01 * m01) * inv}};
    const double e[3] = {q[0] - a.xyz[3 * bt], q[1] - a.xyz[3 * bt + 1], q[2] - a.xyz[3 * bt + 2]};
    const double w[3] = {q[0] - sC[0], q[1] - sC[1], q[2] - sC[2]};
    // Bm = S A: column j is w x A[:, j];  Cm = S A S^T: row f is w x Bm[f, :];  gd = [w x (A d), A d]
    double Bm[3][3], Cm[3][3], gd[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Bm[0][j] = w[1] * A[2][j] - w[2] * A[1][j];
      Bm[1][j] = w[2] * A[0][j] - w[0] * A[2][j];
      Bm[2][j] = w[0] * A[1][j] - w[1] * A[0][j];
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      Cm[f][0] = w[1] * Bm[f][2] - w[2] * Bm[f][1];
      Cm[f][1] = w[2] * Bm[f][0] - w[0] * Bm[f][2];
      Cm[f][2] = w[0] * Bm[f][1] - w[1] * Bm[f][0];
      gd[3 + f] = A[f][0] * e[0] + A[f][1] * e[1] + A[f][2] * e[2];
    }
    gd[0] = w[1] * gd[5] - w[2] * gd[4];
    gd[1] = w[2] * gd[3] - w[0] * gd[5];
    gd[2] = w[0] * gd[4] - w[1] * gd[3];
    int h = 2;
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
      for (int g = f; g < 6; ++g) v[h++] += g < 3 ? Cm[f][g] : f < 3 ? Bm[f][g - 3] : A[f - 3][g - 3];
#pragma unroll
    for (int f = 0; f < 6; ++f) v[23 + f] += gd[f];
  }
};

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
