// Batched point-to-plane ICP refinement on the radius index (mvreg.h mvr_icp_refine_plane): the
// loop of Open3D's registration_icp with TransformationEstimationPointToPlane, restated from the maths, beside the
// point-to-point form of icp.hip.  eval(T) is that file's, statement for statement (the nearest target point, strict
// < max_dist, the lowest row on a tie, fitness and rmse on Euclidean distances); icp.hip itself is not touched, so
// mvr_icp_refine keeps its object code.  What differs is what an evaluation sums and what is solved from it.
//
// One workgroup per pair, every iteration inside the one launch, fp64 throughout.  Per evaluation:
//   search   as icp.hip: 27 cells around floor(q / r_index), the query's own first, boxes that cannot win skipped
//   sums     count, sum d^2, and of a = [(q - c) x n, n], b = (q - y) . n (n the normal of the match y, c the target
//            fragment's first point): the upper triangle of sum a a^T (21) and sum a b (6), per thread in registers
//   reduce   block_sum in a fixed order: no atomics, no workspace, a pair's bits do not depend on the batch
//   solve    lane 0: Cholesky of the 6 x 6 system, xi = -H^-1 g; a pivot that fails pivot > 1e-12 max H_ii ends the
//            loop with status bit 8 and T kept.  T <- [R_inc | xi[3:6] + c - R_inc c] T, R_inc = Rz Ry Rx
// Every loop is bounded: max_iters, 27 cells, a cell's rows, and the hash probe (cap >= 2 M).
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// 16 waves, as icp.hip: the search is a chain of dependent loads that only other waves hide.  128 VGPRs at this size
// with 64 spilled (164 B scratch per lane, touched per query around the search, not per candidate); 512 and 256 threads
// (179 VGPRs, no spill, 2 waves per SIMD) measure 1.5 and 1.7 times slower
#ifndef MVR_ICP_PLANE_THREADS
#define MVR_ICP_PLANE_THREADS 1024
#endif
constexpr int kPlaneThreads = MVR_ICP_PLANE_THREADS;
constexpr int kPlaneSums = 29;   // n, sum d^2, upper triangle of sum a a^T [21], sum a b [6]

struct IcpPlaneArgs {
  RIndex ix;
  const double* xyz; const double* normals; const int64_t* off; int B; int64_t M; double r;
  const int64_t* pairs; const double* T0;
  double max_dist; int max_iters; double tol_fitness, tol_rmse;
  double* T; double* fitness; double* rmse; int32_t* n_corr; int32_t* iters; int32_t* status; double* trace;
};

// lane 0: xi <- -H^-1 g by Cholesky, H given by its upper triangle in row order.  false: a pivot is not above
// 1e-12 of the largest diagonal entry (a NaN fails the test too), xi is then not meaningful
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

__global__ __launch_bounds__(kPlaneThreads) void icp_plane_kernel(IcpPlaneArgs a) {
  __shared__ double red[kPlaneSums * (kPlaneThreads / 64)];
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
      for (int64_t e = tid; e < 2 * rows; e += kPlaneThreads) trace[e] = -1.0;
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

  // v <- the sums of eval(sT), in every thread.  T and the origin are read from LDS (broadcasts) where they are used
  auto eval = [&](double (&v)[kPlaneSums]) {
#pragma unroll
    for (int q = 0; q < kPlaneSums; ++q) v[q] = 0.0;
    for (int64_t i = s0 + tid; i < s1; i += kPlaneThreads) {
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
        const double e[3] = {q[0] - a.xyz[3 * bt], q[1] - a.xyz[3 * bt + 1], q[2] - a.xyz[3 * bt + 2]};
        const double w[3] = {q[0] - sC[0], q[1] - sC[1], q[2] - sC[2]};
        const double ja[6] = {w[1] * n[2] - w[2] * n[1], w[2] * n[0] - w[0] * n[2], w[0] * n[1] - w[1] * n[0],
                              n[0], n[1], n[2]};
        const double b = e[0] * n[0] + e[1] * n[1] + e[2] * n[2];
        v[0] += 1.0;
        v[1] += best;
        int h = 2;
#pragma unroll
        for (int f = 0; f < 6; ++f)
#pragma unroll
          for (int g = f; g < 6; ++g) v[h++] += ja[f] * ja[g];
#pragma unroll
        for (int f = 0; f < 6; ++f) v[23 + f] += ja[f] * b;
      }
    }
    block_sum<kPlaneSums>(v, red);
  };

  double v[kPlaneSums];
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
    for (int64_t e = 2 * ((int64_t)k + 1) + tid; e < 2 * rows; e += kPlaneThreads) trace[e] = -1.0;
}

}  // namespace mvr

extern "C" int mvr_icp_refine_plane(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                                    const int64_t* off, int B, int64_t M, double r_index, const int64_t* pairs,
                                    const double* T0, int P, double max_dist, int max_iters, double tol_fitness,
                                    double tol_rmse, double* T, double* fitness, double* rmse, int32_t* n_corr,
                                    int32_t* iters, int32_t* status, double* trace, hipStream_t stream) {
  if (P < 0 || M < 0 || M > 0x7fffffff || max_iters < 0 || B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (!(max_dist > 0.0) || !(r_index > 0.0) || max_dist > r_index || !(tol_fitness >= 0.0) || !(tol_rmse >= 0.0))
    return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T0 || !T || !fitness || !rmse || !status) return MVR_EINVAL;
  if (M > 0 && (!index || !xyz || !normals || !off || index_bytes < mvr_radius_index_bytes(M))) return MVR_EINVAL;
  mvr::IcpPlaneArgs a{};
  if (M > 0) a.ix = mvr::index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.normals = normals; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T0 = T0;
  a.max_dist = max_dist; a.max_iters = max_iters; a.tol_fitness = tol_fitness; a.tol_rmse = tol_rmse;
  a.T = T; a.fitness = fitness; a.rmse = rmse; a.n_corr = n_corr; a.iters = iters; a.status = status; a.trace = trace;
  hipLaunchKernelGGL(mvr::icp_plane_kernel, dim3(P), dim3(mvr::kPlaneThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
