// What the radius-index nearest-neighbour kernels share: the search of the nearest target point
// (icp.hip, icp_plane.hip, icp_gicp.hip, info.hip), the validation of a pair, and for the three ICP kernels the args
// struct with its host-side checks, the loop with its stopping rule, trace and status bits, and the 6 x 6 solve with
// the update of T.  A kernel supplies a model: what a match adds to the sums and what lane 0 solves from them.
// Everything is inlined into the kernel that uses it; each of the four sources stays its own translation unit.
#pragma once
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// ------------------------------------------------------------------------------------------------------------ search
// q <- T x_i, T the 3 x 4 in sT (LDS: broadcasts, read where they are used rather than held across the search)
__device__ __forceinline__ void moved_point(const double* sT, const double* xyz, int64_t i, double (&q)[3]) {
  const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  q[0] = sT[0] * x + sT[1] * y + sT[2] * z + sT[3];
  q[1] = sT[4] * x + sT[5] * y + sT[6] * z + sT[7];
  q[2] = sT[8] * x + sT[9] * y + sT[10] * z + sT[11];
}

// The row of fragment tf's point nearest to q among those with sqrt(d^2) < max_dist (strictly), the lowest row on a
// tie; -1 if there is none.  d2 <- its squared distance (md2 = max_dist^2 (1 + 1e-9) if there is none).  Walks the 27
// cells around floor(q / r) through the cell hash, the query's own first.  A cell whose box lies farther than the best
// so far (or than max_dist, through md2) is skipped: the bound is a lower bound of the distance to every point of the
// box, shrunk by slack = 1e-9 r, far above the rounding of q / r, so a skipped box holds no point that could win or tie
// and the result is that of all 27.  The constants come by value and the best lives in locals: that shape keeps the
// callers at their 128 VGPRs without a scratch access inside the two loops, and the Makefile's per-source flag keeps
// the three bounds behind their uniform dx / dy / dz == 0 branches.
__device__ __forceinline__ int64_t nearest_row(const RIndex& ix, const double* xyz, int64_t tf, const double (&q)[3],
                                               double r, double slack, double md2, double max_dist, double& d2_out) {
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
    const double gx = dx == 0 ? 0.0 : fmax((dx < 0 ? lo[0] : r - lo[0]) - slack, 0.0);
    const double gy = dy == 0 ? 0.0 : fmax((dy < 0 ? lo[1] : r - lo[1]) - slack, 0.0);
    const double gz = dz == 0 ? 0.0 : fmax((dz < 0 ? lo[2] : r - lo[2]) - slack, 0.0);
    if (gx * gx + gy * gy + gz * gz > best) continue;   // no point of that cell can win
    const int2 se = cell_find(ix, pack_key((int)tf, c[0] + dx, c[1] + dy, c[2] + dz));
    for (int j = se.x; j < se.y; ++j) {
      const int64_t t = ix.sidx[j];
      const double ex = q[0] - xyz[3 * t], ey = q[1] - xyz[3 * t + 1], ez = q[2] - xyz[3 * t + 2];
      const double d2 = ex * ex + ey * ey + ez * ez;
      if (sqrt(d2) < max_dist && (bt < 0 || d2 < best || (d2 == best && t < bt))) {
        best = d2;
        bt = t;
      }
    }
  }
  d2_out = best;
  return bt;
}

// -------------------------------------------------------------------------------------------------------------- pair
struct PairRange {
  int64_t tf, s0, s1, t0, t1;   // the target fragment; the rows [s0, s1) of the source and [t0, t1) of the target
  bool ok;                      // both fragment indices in [0, B), T finite, the offsets inside [0, M]
};
// pair p of the batch; T its 12 doubles.  off NULL (M == 0): every fragment is empty
__device__ __forceinline__ PairRange pair_range(const int64_t* pairs, const double* T, const int64_t* off, int B,
                                                int64_t M, int p) {
  PairRange g{};
  const int64_t sf = pairs[2 * (int64_t)p];
  g.tf = pairs[2 * (int64_t)p + 1];
  g.ok = sf >= 0 && sf < B && g.tf >= 0 && g.tf < B;
  for (int q = 0; q < 12; ++q) g.ok = g.ok && isfinite(T[q]);
  if (g.ok && off) {
    g.s0 = off[sf];
    g.s1 = off[sf + 1];
    g.t0 = off[g.tf];
    g.t1 = off[g.tf + 1];
    g.ok = g.s0 >= 0 && g.s0 <= g.s1 && g.s1 <= M && g.t0 >= 0 && g.t1 <= M;
  }
  return g;
}

// ------------------------------------------------------------------------------------------------------- 6 x 6 solve
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

// --------------------------------------------------------------------------------------------- the three ICP kernels
struct IcpArgs {
  RIndex ix;
  const double* xyz; const double* normals; const int64_t* off; int B; int64_t M; double r;   // normals, epsilon:
  const int64_t* pairs; const double* T0;                                                      // where they apply
  double max_dist, epsilon; int max_iters; double tol_fitness, tol_rmse;
  double* T; double* fitness; double* rmse; int32_t* n_corr; int32_t* iters; int32_t* status; double* trace;
};

// The loop of one pair, every iteration inside the one launch (mvreg.h mvr_icp_refine has the semantics).  Model:
//   kSums, kMinCorr, kOrigin   the number of sums (the first two are n and sum d^2, added here), the least number of
//                              correspondences for a solve, the doubles of the origin
//   kCanFail                   whether solve can return false; where it cannot, nothing refers to the verdict's LDS
//                              word and the compiler drops it (LDS 2320 B for point-to-point)
//   origin(a, g, T0, sO)       lane 0: the per-pair origin of the sums
//   accumulate(a, sT, sO, v, i, bt, q)   what source row i, moved to q and matched with target row bt, adds to v[2:]
//   solve(v, sT, sO) -> bool   lane 0: the next T into sT from the block's sums; false ends the loop with status bit 8
template <class Model, int kThreads>
__device__ __forceinline__ void icp_loop(const IcpArgs& a) {
  constexpr int kSums = Model::kSums;
  __shared__ double red[kSums * (kThreads / 64)];
  __shared__ double sT[12], sO[Model::kOrigin];   // the current T; the origin of the sums
  __shared__ int sBad;                            // the solve's verdict, from lane 0 to everyone
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t rows = (int64_t)a.max_iters + 1;
  double* trace = a.trace ? a.trace + (int64_t)p * rows * 2 : nullptr;
  double* To = a.T + 12 * (int64_t)p;
  const double* T0 = a.T0 + 12 * (int64_t)p;

  const PairRange g = pair_range(a.pairs, T0, a.off, a.B, a.M, p);
  if (!g.ok) {   // uniform: T = T0 bit for bit, nothing evaluated
    if (tid == 0) {
      for (int q = 0; q < 12; ++q) To[q] = T0[q];
      a.fitness[p] = 0.0;
      a.rmse[p] = 0.0;
      if (a.n_corr) a.n_corr[p] = 0;
      if (a.iters) a.iters[p] = 0;
      a.status[p] = 4;
    }
    if (trace)
      for (int64_t e = tid; e < 2 * rows; e += kThreads) trace[e] = -1.0;
    return;
  }
  const int64_t n_src = g.s1 - g.s0;
  if (tid == 0) {
    for (int q = 0; q < 12; ++q) sT[q] = T0[q];
    Model::origin(a, g, T0, sO);
    if constexpr (Model::kCanFail) sBad = 0;
  }
  __syncthreads();
  const double r = a.r, slack = 1e-9 * a.r, md2 = a.max_dist * a.max_dist * (1.0 + 1e-9);

  double v[kSums];
  int k = 0, n = 0, status = 0;
  double fit = 0.0, rm = 0.0;
  bool converged = false;
  while (true) {
    // v <- the sums of eval(sT), in every thread: per thread in registers, then block_sum in a fixed order
#pragma unroll
    for (int q = 0; q < kSums; ++q) v[q] = 0.0;
    for (int64_t i = g.s0 + tid; i < g.s1; i += kThreads) {
      double q[3], best;
      moved_point(sT, a.xyz, i, q);
      const int64_t bt = nearest_row(a.ix, a.xyz, g.tf, q, r, slack, md2, a.max_dist, best);
      if (bt >= 0) {
        Model::accumulate(a, sT, sO, v, i, bt, q);
        v[0] += 1.0;
        v[1] += best;
      }
    }
    block_sum<kSums>(v, red);
    n = (int)v[0];
    const double nfit = n_src > 0 ? v[0] / (double)n_src : 0.0, nrm = n > 0 ? sqrt(v[1] / v[0]) : 0.0;
    converged = k > 0 && fabs(nfit - fit) < a.tol_fitness && fabs(nrm - rm) < a.tol_rmse;
    fit = nfit;
    rm = nrm;
    if (trace && tid == 0) { trace[2 * k] = fit; trace[2 * k + 1] = rm; }
    if (converged || k == a.max_iters) break;
    if (n < Model::kMinCorr) { status |= 1; break; }
    if (tid == 0) {
      [[maybe_unused]] const bool solved = Model::solve(v, sT, sO);
      if constexpr (Model::kCanFail) sBad = !solved;   // one store: a store per failing pivot spills more (4.27)
    }
    __syncthreads();   // block_sum's barriers separate the evaluation's reads of sT from the next solve
    if constexpr (Model::kCanFail)
      if (sBad) { status |= 8; break; }   // uniform: T kept
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
    for (int64_t e = 2 * ((int64_t)k + 1) + tid; e < 2 * rows; e += kThreads) trace[e] = -1.0;
}

// What the models of point-to-plane and generalized ICP share: the layout of the sums, the origin c (the target
// fragment's first point, so that the cross products stay small) and the solve.  Theirs is accumulate
struct SixDofModel {
  static constexpr int kSums = 29;   // n, sum d^2, upper triangle of H [21], g [6]
  static constexpr int kMinCorr = 6, kOrigin = 3;
  static constexpr bool kCanFail = true;

  __device__ __forceinline__ static void origin(const IcpArgs& a, const PairRange& g, const double*, double* sC) {
    for (int e = 0; e < 3; ++e) sC[e] = g.t0 < g.t1 ? a.xyz[3 * g.t0 + e] : 0.0;
  }

  // xi = -H^-1 g, then T <- D T in sT with D = [R_inc | xi[3:6] + c - R_inc c], R_inc = Rz(xi2) Ry(xi1) Rx(xi0).
  // false: H is not positive definite to working precision, sT kept
  __device__ __forceinline__ static bool solve(const double (&v)[kSums], double* sT, const double* sC) {
    double xi[6];
    if (!solve6(v + 2, v + 23, xi)) return false;
    const double cx = cos(xi[0]), sx = sin(xi[0]), cy = cos(xi[1]), sy = sin(xi[1]), cz = cos(xi[2]), sz = sin(xi[2]);
    const double R[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx},
                            {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx},
                            {-sy, cy * sx, cy * cx}};
    double Tn[12];
    for (int e = 0; e < 3; ++e) {
      for (int f = 0; f < 4; ++f) Tn[4 * e + f] = R[e][0] * sT[f] + R[e][1] * sT[4 + f] + R[e][2] * sT[8 + f];
      Tn[4 * e + 3] += xi[3 + e] + sC[e] - (R[e][0] * sC[0] + R[e][1] * sC[1] + R[e][2] * sC[2]);
    }
    for (int q = 0; q < 12; ++q) sT[q] = Tn[q];
    return true;
  }
};

// ------------------------------------------------------------------------------------------------------- entry points
// the value checks every entry makes before it looks at P, and the pointer checks it makes once P > 0
inline bool search_values_ok(int B, int64_t M, int P, double r_index, double max_dist) {
  return P >= 0 && M >= 0 && M <= 0x7fffffff && B > 0 && B < (1 << 15) && max_dist > 0.0 && r_index > 0.0 &&
         !(max_dist > r_index);
}
inline bool search_pointers_ok(const void* index, size_t index_bytes, const double* xyz, const int64_t* off,
                               int64_t M) {
  return M == 0 || (index && xyz && off && index_bytes >= mvr_radius_index_bytes(M));
}

// The checks the three ICP entries share, then the args.  MVR_EINVAL comes before P == 0, and P == 0 returns MVR_OK
// before any pointer is looked at: the caller returns whatever this returns when that is not MVR_OK or P == 0
inline int icp_args(IcpArgs& a, const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                    int64_t M, double r_index, const int64_t* pairs, const double* T0, int P, double max_dist,
                    int max_iters, double tol_fitness, double tol_rmse, double* T, double* fitness, double* rmse,
                    int32_t* n_corr, int32_t* iters, int32_t* status, double* trace) {
  if (!search_values_ok(B, M, P, r_index, max_dist) || max_iters < 0 || !(tol_fitness >= 0.0) || !(tol_rmse >= 0.0))
    return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T0 || !T || !fitness || !rmse || !status) return MVR_EINVAL;
  if (!search_pointers_ok(index, index_bytes, xyz, off, M)) return MVR_EINVAL;
  a = IcpArgs{};
  if (M > 0) a.ix = index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T0 = T0;
  a.max_dist = max_dist; a.max_iters = max_iters; a.tol_fitness = tol_fitness; a.tol_rmse = tol_rmse;
  a.T = T; a.fitness = fitness; a.rmse = rmse; a.n_corr = n_corr; a.iters = iters; a.status = status; a.trace = trace;
  return MVR_OK;
}

}  // namespace mvr
