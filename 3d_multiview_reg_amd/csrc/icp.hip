// Batched point-to-point ICP refinement on the radius index of overlap.hip (mvreg.h mvr_icp_refine).
// The reference stops at the coarse estimate (weighted Procrustes / RANSAC over 5000 correspondences); this is the
// fine registration on the fragments' own points that Open3D's registration_icp does after it, restated from the
// maths: nearest target point per transformed source point, unweighted Kabsch on the pairs closer than max_dist.
//
// One 1024-thread workgroup per pair, every iteration inside the one launch, fp64 throughout.  Per evaluation:
//   search   threads stride over the source points; q = R x + t walks the 27 cells around floor(q / r_index) through
//            the cell hash, centre cell first; a cell whose box lies farther than the best so far (or than max_dist)
//            is skipped, which cannot change the result.  Nearest by squared distance, the lowest row on a tie
//   sums     count, sum d^2, sum x, sum y, sum x y^T per thread in registers, relative to a per-pair origin (the
//            source fragment's first point and its image under T0), so that sum x y^T - n mx my^T cancels little
//   reduce   block_sum: a lane tree, then the waves in index order through LDS.  No atomics and no workspace, so a
//            pair's bits do not depend on the batch around it
//   solve    lane 0: centred covariance from the sums, jacobi_svd3, det-corrected R, t; broadcast through LDS
// Every loop is bounded: max_iters, the Jacobi sweep cap, and the hash probe (cap >= 2 M ends it at an empty slot).
#include "common.hpp"
#include "rindex.hpp"
#include "svd3.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// 16 waves = 4 per SIMD: a query is a chain of dependent loads (hash slot -> cell range -> row -> point), and the
// other waves are what hides it.  128 VGPRs at this size, 13 of them spilled (once per query, outside the cell and
// candidate loops); 512 and 256 threads need no spill and measure 1.5 and 1.8 times slower
#ifndef MVR_ICP_THREADS
#define MVR_ICP_THREADS 1024
#endif
constexpr int kIcpThreads = MVR_ICP_THREADS;
constexpr int kIcpSums = 17;   // n, sum d^2, sum x [3], sum y [3], sum x y^T [9]

struct IcpArgs {
  RIndex ix;
  const double* xyz; const int64_t* off; int B; int64_t M; double r;
  const int64_t* pairs; const double* T0;
  double max_dist; int max_iters; double tol_fitness, tol_rmse;
  double* T; double* fitness; double* rmse; int32_t* n_corr; int32_t* iters; int32_t* status; double* trace;
};

__global__ __launch_bounds__(kIcpThreads) void icp_kernel(IcpArgs a) {
  __shared__ double red[kIcpSums * (kIcpThreads / 64)];
  __shared__ double sT[12], sO[6];   // the current T; the origins of the sums (source side, target side)
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t sf = a.pairs[2 * (int64_t)p], tf = a.pairs[2 * (int64_t)p + 1];
  const int64_t rows = (int64_t)a.max_iters + 1;
  double* trace = a.trace ? a.trace + (int64_t)p * rows * 2 : nullptr;
  double* To = a.T + 12 * (int64_t)p;

  const double* T0 = a.T0 + 12 * (int64_t)p;
  bool ok = sf >= 0 && sf < a.B && tf >= 0 && tf < a.B;
  for (int q = 0; q < 12; ++q) ok = ok && isfinite(T0[q]);
  int64_t s0 = 0, s1 = 0;
  if (ok && a.off) {
    s0 = a.off[sf];
    s1 = a.off[sf + 1];
    ok = s0 >= 0 && s0 <= s1 && s1 <= a.M && a.off[tf] >= 0 && a.off[tf + 1] <= a.M;
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
      for (int64_t e = tid; e < 2 * rows; e += kIcpThreads) trace[e] = -1.0;
    return;
  }
  const int64_t n_src = s1 - s0;
  if (tid == 0) {
    double o[3] = {0.0, 0.0, 0.0};
    if (n_src > 0)
      for (int e = 0; e < 3; ++e) o[e] = a.xyz[3 * s0 + e];
    for (int q = 0; q < 12; ++q) sT[q] = T0[q];
    for (int e = 0; e < 3; ++e) {
      sO[e] = o[e];
      sO[3 + e] = T0[4 * e] * o[0] + T0[4 * e + 1] * o[1] + T0[4 * e + 2] * o[2] + T0[4 * e + 3];
    }
  }
  __syncthreads();
  const double r = a.r, slack = 1e-9 * a.r, md2 = a.max_dist * a.max_dist * (1.0 + 1e-9);

  // v <- the sums of eval(sT), in every thread.  T and the origins are read from LDS (broadcasts) where they are
  // used: twelve registers fewer per value held across the search
  auto eval = [&](double (&v)[kIcpSums]) {
#pragma unroll
    for (int q = 0; q < kIcpSums; ++q) v[q] = 0.0;
    for (int64_t i = s0 + tid; i < s1; i += kIcpThreads) {
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
        const double xr[3] = {x - sO[0], y - sO[1], z - sO[2]};
        const double yr[3] = {a.xyz[3 * bt] - sO[3], a.xyz[3 * bt + 1] - sO[4], a.xyz[3 * bt + 2] - sO[5]};
        v[0] += 1.0;
        v[1] += best;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          v[2 + e] += xr[e];
          v[5 + e] += yr[e];
#pragma unroll
          for (int f = 0; f < 3; ++f) v[8 + 3 * e + f] += xr[e] * yr[f];
        }
      }
    }
    block_sum<kIcpSums>(v, red);
  };

  double v[kIcpSums];
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
    if (n < 3) { status |= 1; break; }
    if (tid == 0) {   // argmin |R x + t - y|^2 over the valid pairs, on the original source points
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
        sT[4 * e + 3] = (my[e] + sO[3 + e]) -
                        (R[0] * (mx[0] + sO[0]) + R[1] * (mx[1] + sO[1]) + R[2] * (mx[2] + sO[2]));
      }
    }
    __syncthreads();   // eval's barriers separate its reads of sT from the next solve
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
    for (int64_t e = 2 * ((int64_t)k + 1) + tid; e < 2 * rows; e += kIcpThreads) trace[e] = -1.0;
}

}  // namespace mvr

extern "C" int mvr_icp_refine(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                              int64_t M, double r_index, const int64_t* pairs, const double* T0, int P,
                              double max_dist, int max_iters, double tol_fitness, double tol_rmse, double* T,
                              double* fitness, double* rmse, int32_t* n_corr, int32_t* iters, int32_t* status,
                              double* trace, hipStream_t stream) {
  if (P < 0 || M < 0 || M > 0x7fffffff || max_iters < 0 || B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (!(max_dist > 0.0) || !(r_index > 0.0) || max_dist > r_index || !(tol_fitness >= 0.0) || !(tol_rmse >= 0.0))
    return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T0 || !T || !fitness || !rmse || !status) return MVR_EINVAL;
  if (M > 0 && (!index || !xyz || !off || index_bytes < mvr_radius_index_bytes(M))) return MVR_EINVAL;
  mvr::IcpArgs a{};
  if (M > 0) a.ix = mvr::index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T0 = T0;
  a.max_dist = max_dist; a.max_iters = max_iters; a.tol_fitness = tol_fitness; a.tol_rmse = tol_rmse;
  a.T = T; a.fitness = fitness; a.rmse = rmse; a.n_corr = n_corr; a.iters = iters; a.status = status; a.trace = trace;
  hipLaunchKernelGGL(mvr::icp_kernel, dim3(P), dim3(mvr::kIcpThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
