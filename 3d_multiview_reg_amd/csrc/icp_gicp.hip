// Batched generalized (plane-to-plane) ICP refinement on the radius index (mvreg.h mvr_icp_refine_generalized;
// DESIGN.md 4.23): the loop of Segal et al.'s GICP, Open3D's registration_generalized_icp, restated from the maths,
// beside the point-to-plane form of icp_plane.hip.  eval(T), the stopping rule, the trace, the status bits, the origin
// c, the update of T and solve6 are that file's, statement for statement; icp.hip and icp_plane.hip are not touched,
// so their entry points keep their object code.  What differs is what a solve sums.
//
// A point with unit normal n has covariance I - (1 - eps) n n^T: 1 in the surface, eps along the normal.  For a source
// point x matched with y (q = T x, R the rotation of T, n the normal of y, m = R n_s with n_s the normal of x):
//   M = 2 I - (1 - eps)(n n^T + m m^T)    A = M^-1 (symmetric; by cofactors)
//   G = [-[q - c]x | I]                   d = q - y
//   H = sum G^T A G                       g = sum G^T A d                xi = -H^-1 g
// With S = [q - c]x: G^T A G = [[S A S^T, S A], [(S A)^T, A]] and G^T A d = [S (A d), A d].
//
// One workgroup per pair, every iteration inside the one launch, fp64 throughout.  Per evaluation:
//   search   as icp.hip: 27 cells around floor(q / r_index), the query's own first, boxes that cannot win skipped
//   sums     count, sum d^2, the upper triangle of H (21) and g (6), per thread in registers.  The two normals are
//            loaded, n_s rotated, M inverted and the products formed only once a match is found: nothing of it is live
//            across the search
//   reduce   block_sum in a fixed order: no atomics, no workspace, a pair's bits do not depend on the batch
//   solve    lane 0: Cholesky of the 6 x 6 system; a pivot that fails pivot > 1e-12 max H_ii ends the loop with status
//            bit 8 and T kept (a non-finite A, from normals that are not unit, ends there too).
//            T <- [R_inc | xi[3:6] + c - R_inc c] T, R_inc = Rz Ry Rx
// Every loop is bounded: max_iters, 27 cells, a cell's rows, and the hash probe (cap >= 2 M).
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// 16 waves, as icp.hip and icp_plane.hip: the search is a chain of dependent loads that only other waves hide, and
// the search is the same code (DESIGN.md 4.23 has the compiler's register, scratch and LDS figures)
#ifndef MVR_ICP_GICP_THREADS
#define MVR_ICP_GICP_THREADS 1024
#endif
constexpr int kGicpThreads = MVR_ICP_GICP_THREADS;
constexpr int kGicpSums = 29;   // n, sum d^2, upper triangle of sum G^T A G [21], sum G^T A d [6]

struct IcpGicpArgs {
  RIndex ix;
  const double* xyz; const double* normals; const int64_t* off; int B; int64_t M; double r;
  const int64_t* pairs; const double* T0;
  double max_dist, epsilon; int max_iters; double tol_fitness, tol_rmse;
  double* T; double* fitness; double* rmse; int32_t* n_corr; int32_t* iters; int32_t* status; double* trace;
};

// icp_plane.hip's solve6, statement for statement.  lane 0: xi <- -H^-1 g by Cholesky, H given by its upper triangle
// in row order.  false: a pivot is not above 1e-12 of the largest diagonal entry (a NaN fails the test too), xi is
// then not meaningful
__device__ static bool solve6(const double* h, const double* g, double (&xi)[6]) {
  double L[6][6];
  double top = 0.0;
  for (int i = 0, q = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++q) {
      L[j][i] = h[q];
      if (i == j) top = fmax(top, h[q]);
    }
  const double floor_ = 1e-12 * top;
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > floor_)) return false;
    const double ljj = sqrt(d);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {   // L y = -g
    double s = -g[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {   // L^T xi = y
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
  return true;
}

__global__ __launch_bounds__(kGicpThreads) void icp_gicp_kernel(IcpGicpArgs a) {
  __shared__ double red[kGicpSums * (kGicpThreads / 64)];
  __shared__ double sT[12], sC[3];   // the current T; the origin of the cross products
  __shared__ int sBad;               // the solve's verdict, from lane 0 to everyone
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t sf = a.pairs[2 * (int64_t)p], tf = a.pairs[2 * (int64_t)p + 1];
  const int64_t rows = (int64_t)a.max_iters + 1;
  double* trace = a.trace ? a.trace + (int64_t)p * rows * 2 : nullptr;
  double* To = a.T + 12 * (int64_t)p;

  const double* T0 = a.T0 + 12 * (int64_t)p;
  bool ok = sf >= 0 && sf < a.B && tf >= 0 && tf < a.B;
  for (int q = 0; q < 12; ++q) ok = ok && isfinite(T0[q]);
  int64_t s0 = 0, s1 = 0, t0 = 0, t1 = 0;
  if (ok && a.off) {
    s0 = a.off[sf];
    s1 = a.off[sf + 1];
    t0 = a.off[tf];
    t1 = a.off[tf + 1];
    ok = s0 >= 0 && s0 <= s1 && s1 <= a.M && t0 >= 0 && t1 <= a.M;
  }
  if (!ok) {   // uniform: T = T0 bit for bit, nothing evaluated
    if (tid == 0) {
      for (int q = 0; q < 12; ++q) To[q] = T0[q];
      a.fitness[p] = 0.0;
      a.rmse[p] = 0.0;
      if (a.n_corr) a.n_corr[p] = 0;
      if (a.iters) a.iters[p] = 0;
      a.status[p] = 4;
    }
    if (trace)
      for (int64_t e = tid; e < 2 * rows; e += kGicpThreads) trace[e] = -1.0;
    return;
  }
  const int64_t n_src = s1 - s0;
  if (tid == 0) {
    for (int q = 0; q < 12; ++q) sT[q] = T0[q];
    for (int e = 0; e < 3; ++e) sC[e] = t0 < t1 ? a.xyz[3 * t0 + e] : 0.0;
    sBad = 0;
  }
  __syncthreads();
  const double r = a.r, slack = 1e-9 * a.r, md2 = a.max_dist * a.max_dist * (1.0 + 1e-9);
  const double ome = 1.0 - a.epsilon;

  // v <- the sums of eval(sT), in every thread.  T and the origin are read from LDS (broadcasts) where they are used
  auto eval = [&](double (&v)[kGicpSums]) {
#pragma unroll
    for (int q = 0; q < kGicpSums; ++q) v[q] = 0.0;
    for (int64_t i = s0 + tid; i < s1; i += kGicpThreads) {
      const double x = a.xyz[3 * i], y = a.xyz[3 * i + 1], z = a.xyz[3 * i + 2];
      const double q[3] = {sT[0] * x + sT[1] * y + sT[2] * z + sT[3], sT[4] * x + sT[5] * y + sT[6] * z + sT[7],
                           sT[8] * x + sT[9] * y + sT[10] * z + sT[11]};
      int64_t c[3];
      double lo[3];   // distance to the lower neighbour cell along each axis; r - lo to the upper one
      for (int e = 0; e < 3; ++e) {
        const double cf = floor(q[e] / r);
        c[e] = (int64_t)cf + OV_BIAS;
        lo[e] = q[e] - cf * r;
      }
      double best = md2;
      int64_t bt = -1;
      for (int k = 0; k < 27; ++k) {
        const int cell = (k + 13) % 27;   // the query's own cell first
        const int dx = cell % 3 - 1, dy = (cell / 3) % 3 - 1, dz = cell / 9 - 1;
        // a lower bound of the distance to that cell's box: shrunk by a slack far above the rounding of q / r
        const double gx = dx == 0 ? 0.0 : fmax((dx < 0 ? lo[0] : r - lo[0]) - slack, 0.0);
        const double gy = dy == 0 ? 0.0 : fmax((dy < 0 ? lo[1] : r - lo[1]) - slack, 0.0);
        const double gz = dz == 0 ? 0.0 : fmax((dz < 0 ? lo[2] : r - lo[2]) - slack, 0.0);
        if (gx * gx + gy * gy + gz * gz > best) continue;   // no point of that cell can win
        const int2 se = cell_find(a.ix, pack_key((int)tf, c[0] + dx, c[1] + dy, c[2] + dz));
        for (int j = se.x; j < se.y; ++j) {
          const int64_t t = a.ix.sidx[j];
          const double ex = q[0] - a.xyz[3 * t], ey = q[1] - a.xyz[3 * t + 1], ez = q[2] - a.xyz[3 * t + 2];
          const double d2 = ex * ex + ey * ey + ez * ez;
          if (sqrt(d2) < a.max_dist && (bt < 0 || d2 < best || (d2 == best && t < bt))) {
            best = d2;
            bt = t;
          }
        }
      }
      if (bt >= 0) {
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
        v[0] += 1.0;
        v[1] += best;
        int h = 2;
#pragma unroll
        for (int f = 0; f < 6; ++f)
#pragma unroll
          for (int g = f; g < 6; ++g) v[h++] += g < 3 ? Cm[f][g] : f < 3 ? Bm[f][g - 3] : A[f - 3][g - 3];
#pragma unroll
        for (int f = 0; f < 6; ++f) v[23 + f] += gd[f];
      }
    }
    block_sum<kGicpSums>(v, red);
  };

  double v[kGicpSums];
  int k = 0, n = 0, status = 0;
  double fit = 0.0, rm = 0.0;
  bool converged = false;
  while (true) {
    eval(v);
    n = (int)v[0];
    const double nfit = n_src > 0 ? v[0] / (double)n_src : 0.0, nrm = n > 0 ? sqrt(v[1] / v[0]) : 0.0;
    converged = k > 0 && fabs(nfit - fit) < a.tol_fitness && fabs(nrm - rm) < a.tol_rmse;
    fit = nfit;
    rm = nrm;
    if (trace && tid == 0) { trace[2 * k] = fit; trace[2 * k + 1] = rm; }
    if (converged || k == a.max_iters) break;
    if (n < 6) { status |= 1; break; }
    if (tid == 0) {
      double xi[6];
      if (!solve6(v + 2, v + 23, xi)) {
        sBad = 1;
      } else {   // T <- D T, D = [R_inc | xi[3:6] + c - R_inc c], R_inc = Rz(xi2) Ry(xi1) Rx(xi0)
        const double cx = cos(xi[0]), sx = sin(xi[0]), cy = cos(xi[1]), sy = sin(xi[1]), cz = cos(xi[2]),
                     sz = sin(xi[2]);
        const double R[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                                {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                                {-sy, cy * sx, cy * cx}};
        double Tn[12];
        for (int e = 0; e < 3; ++e) {
          for (int f = 0; f < 4; ++f) Tn[4 * e + f] = R[e][0] * sT[f] + R[e][1] * sT[4 + f] + R[e][2] * sT[8 + f];
          Tn[4 * e + 3] += xi[3 + e] + sC[e] - (R[e][0] * sC[0] + R[e][1] * sC[1] + R[e][2] * sC[2]);
        }
        for (int q = 0; q < 12; ++q) sT[q] = Tn[q];
      }
    }
    __syncthreads();   // eval's barriers separate its reads of sT from the next solve
    if (sBad) { status |= 8; break; }   // uniform: H is not positive definite to working precision, T kept
    ++k;
  }
  if (k == a.max_iters && !converged && (a.tol_fitness > 0.0 || a.tol_rmse > 0.0)) status |= 2;
  if (tid == 0) {
    for (int q = 0; q < 12; ++q) To[q] = sT[q];
    a.fitness[p] = fit;
    a.rmse[p] = rm;
    if (a.n_corr) a.n_corr[p] = n;
    if (a.iters) a.iters[p] = k;
    a.status[p] = status;
  }
  if (trace)
    for (int64_t e = 2 * ((int64_t)k + 1) + tid; e < 2 * rows; e += kGicpThreads) trace[e] = -1.0;
}

}  // namespace mvr

extern "C" int mvr_icp_refine_generalized(const void* index, size_t index_bytes, const double* xyz,
                                          const double* normals, const int64_t* off, int B, int64_t M, double r_index,
                                          const int64_t* pairs, const double* T0, int P, double max_dist,
                                          double epsilon, int max_iters, double tol_fitness, double tol_rmse, double* T,
                                          double* fitness, double* rmse, int32_t* n_corr, int32_t* iters,
                                          int32_t* status, double* trace, hipStream_t stream) {
  if (P < 0 || M < 0 || M > 0x7fffffff || max_iters < 0 || B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (!(max_dist > 0.0) || !(r_index > 0.0) || max_dist > r_index || !(tol_fitness >= 0.0) || !(tol_rmse >= 0.0))
    return MVR_EINVAL;
  if (!(epsilon > 0.0) || !(epsilon <= 1.0)) return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T0 || !T || !fitness || !rmse || !status) return MVR_EINVAL;
  if (M > 0 && (!index || !xyz || !normals || !off || index_bytes < mvr_radius_index_bytes(M))) return MVR_EINVAL;
  mvr::IcpGicpArgs a{};
  if (M > 0) a.ix = mvr::index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.normals = normals; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T0 = T0;
  a.max_dist = max_dist; a.epsilon = epsilon; a.max_iters = max_iters;
  a.tol_fitness = tol_fitness; a.tol_rmse = tol_rmse;
  a.T = T; a.fitness = fitness; a.rmse = rmse; a.n_corr = n_corr; a.iters = iters; a.status = status; a.trace = trace;
  hipLaunchKernelGGL(mvr::icp_gicp_kernel, dim3(P), dim3(mvr::kGicpThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
