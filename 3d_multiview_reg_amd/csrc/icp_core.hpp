// What the radius-index nearest-neighbour kernels share: the search of the nearest target point
// (icp.hip, icp_plane.hip, icp_gicp.hip, icp_robust.hip, icp_colored.hip, info.hip), the validation of a pair, and for the ICP kernels
// the args struct with its host-side checks, the loop with its stopping rule, trace and status bits, and the 6 x 6
// solve with the update of T.  A kernel supplies a model: what a match adds to the sums and what lane 0 solves from
// them.
// The four models live here too, each with a weight policy: UnitWeight for the plain kernels, where
// the weight is a type and nothing is generated for it, KernelWeight for the robust kernels of icp_robust.hip and
// icp_colored.hip.
// Everything is inlined into the kernel that uses it; each of the six sources stays its own translation unit.
#pragma once
#include "common.hpp"
#include "rindex.hpp"
#include "svd3.hpp"
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

// --------------------------------------------------------------------------------------------------- the ICP kernels
struct IcpArgs {
  RIndex ix;
  const double* xyz; const double* normals; const int64_t* off; int B; int64_t M; double r;   // normals, epsilon:
  const int64_t* pairs; const double* T0;                                                      // where they apply
  double max_dist, epsilon; int max_iters; double tol_fitness, tol_rmse;
  double* T; double* fitness; double* rmse; int32_t* n_corr; int32_t* iters; int32_t* status; double* trace;
};

// mvr_icp_refine_robust's: the kernel and its scale (uniform), and where sum w of the returned T's evaluation goes
struct RobustArgs : IcpArgs {
  int kernel; double kernel_k; double* w_sum;
};

// mvr_icp_refine_colored's: the intensities and their tangent-plane gradients (color_grad.hip), and the share lambda
// of the geometric term (uniform)
struct ColoredArgs : RobustArgs {
  const double* intensity; const double* grad; double lambda;
};

// ----------------------------------------------------------------------------------------------------- weight policies
// What a model multiplies a match's terms with.  The plain kernels' weight is a type: w * x is x, and neither the
// residual nor a product is generated for it, so their code is what it was without weights.
struct Unit {};
__device__ __forceinline__ double operator*(Unit, double x) { return x; }
struct UnitWeight {
  using Args = IcpArgs;
  static constexpr bool kWeighted = false;
  template <class Residual>
  __device__ __forceinline__ static Unit weight(const Args&, Residual&&) { return {}; }
};
// w(r) of mvreg.h mvr_icp_refine_robust, k > 0: one switch on a uniform value per match, after the search.  Every
// weight is continuous in r, Tukey's at |r| == k too (u == 0 there).  L2 is exactly 1.0, and x * 1.0 is x exactly
struct KernelWeight {
  using Args = RobustArgs;
  static constexpr bool kWeighted = true;
  template <class Residual>
  __device__ __forceinline__ static double weight(const Args& a, Residual&& residual) {
    if (a.kernel == MVR_KERNEL_L2) return 1.0;
    const double k = a.kernel_k, r = residual();
    switch (a.kernel) {
      case MVR_KERNEL_HUBER: return k / fmax(fabs(r), k);
      case MVR_KERNEL_CAUCHY: { const double s = r / k; return 1.0 / (1.0 + s * s); }
      case MVR_KERNEL_GM: { const double s = k + r * r; return k / (s * s); }
      default: { const double s = r / k, u = 1.0 - s * s; return fabs(r) <= k ? u * u : 0.0; }   // Tukey
    }
  }
};

// Whether an unweighted model still reports w_sum: kCountIsWeightSum in the model (the coloured one, whose unit weights
// sum to the count).  The models without it generate nothing for it
template <class Model, class = void>
struct CountIsWeightSum { static constexpr bool value = false; };
template <class Model>
struct CountIsWeightSum<Model, decltype((void)Model::kCountIsWeightSum)> {
  static constexpr bool value = Model::kCountIsWeightSum;
};

// The loop of one pair, every iteration inside the one launch (mvreg.h mvr_icp_refine has the semantics).  Model:
//   kSums, kMinCorr, kOrigin   the number of sums (the first two are n and sum d^2, added here), the least number of
//                              correspondences for a solve, the doubles of the origin
//   Args, kWeighted            IcpArgs / false, or RobustArgs / true: then the last sum is sum w, and it goes to w_sum
//   kCanFail                   whether solve can return false; where it cannot, nothing refers to the verdict's LDS
//                              word and the compiler drops it (LDS 2320 B for point-to-point)
//   origin(a, g, T0, sO)       lane 0: the per-pair origin of the sums
//   accumulate(a, sT, sO, v, i, bt, q, d2)   what source row i, moved to q and matched with target row bt at squared
//                              distance d2, adds to v[2:]
//   solve(v, sT, sO) -> bool   lane 0: the next T into sT from the block's sums; false ends the loop with status bit 8
template <class Model, int kThreads>
__device__ __forceinline__ void icp_loop(const typename Model::Args& a) {
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
      if constexpr (Model::kWeighted || CountIsWeightSum<Model>::value)
        if (a.w_sum) a.w_sum[p] = 0.0;
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
        Model::accumulate(a, sT, sO, v, i, bt, q, best);
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
    if constexpr (Model::kWeighted)
      if (a.w_sum) a.w_sum[p] = v[kSums - 1];   // of the last evaluation: the returned T's, also after a failed solve
    if constexpr (CountIsWeightSum<Model>::value)
      if (a.w_sum) a.w_sum[p] = v[0];
  }
  if (trace)
    for (int64_t e = 2 * ((int64_t)k + 1) + tid; e < 2 * rows; e += kThreads) trace[e] = -1.0;
}

// ------------------------------------------------------------------------------------------------------------ models
// Point-to-point (mvreg.h mvr_icp_refine): count, sum d^2, sum w x, sum w y, sum w x y^T per thread in registers,
// relative to a per-pair origin (the source fragment's first point and its image under T0), so that
// sum w x y^T - W mx my^T cancels little; weighted also W = sum w.  Lane 0 solves: centred covariance from the sums,
// jacobi_svd3, det-corrected R, t
template <class Wt>
struct PointToPointT {
  using Args = typename Wt::Args;
  static constexpr bool kWeighted = Wt::kWeighted;
  static constexpr int kSums = 17 + kWeighted;   // n, sum d^2, sum x [3], sum y [3], sum x y^T [9], (sum w)
  static constexpr int kMinCorr = 3, kOrigin = 6;   // the origins of the sums: source side, target side
  static constexpr bool kCanFail = kWeighted;       // sum w > 0 can fail; a count >= 3 cannot

  __device__ __forceinline__ static void origin(const IcpArgs& a, const PairRange& g, const double* T0, double* sO) {
    double o[3] = {0.0, 0.0, 0.0};
    if (g.s0 < g.s1)
      for (int e = 0; e < 3; ++e) o[e] = a.xyz[3 * g.s0 + e];
    for (int e = 0; e < 3; ++e) {
      sO[e] = o[e];
      sO[3 + e] = T0[4 * e] * o[0] + T0[4 * e + 1] * o[1] + T0[4 * e + 2] * o[2] + T0[4 * e + 3];
    }
  }

  __device__ __forceinline__ static void accumulate(const Args& a, const double* sT, const double* sO,
                                                    double (&v)[kSums], int64_t i, int64_t bt, const double (&q)[3],
                                                    double d2) {
    // x is read again (moved_point had it): the same values, and no register held across the search for it
    const double xr[3] = {a.xyz[3 * i] - sO[0], a.xyz[3 * i + 1] - sO[1], a.xyz[3 * i + 2] - sO[2]};
    const double yr[3] = {a.xyz[3 * bt] - sO[3], a.xyz[3 * bt + 1] - sO[4], a.xyz[3 * bt + 2] - sO[5]};
    const auto w = Wt::weight(a, [&] { return sqrt(d2); });   // r = |q - y|, the search's own distance
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double wx = w * xr[e];
      v[2 + e] += wx;
      v[5 + e] += w * yr[e];
#pragma unroll
      for (int f = 0; f < 3; ++f) v[8 + 3 * e + f] += wx * yr[f];
    }
    if constexpr (kWeighted) v[kSums - 1] += w;
  }

  // argmin sum w |R x + t - y|^2 over the valid pairs, on the original source points.  false: not sum w > 0
  __device__ __forceinline__ static bool solve(const double (&v)[kSums], double* sT, const double* sO) {
    const double W = kWeighted ? v[kSums - 1] : v[0];
    if constexpr (kWeighted)
      if (!(W > 0.0)) return false;
    double mx[3], my[3], H[3][3], U[3][3], S[3], V[3][3];
    for (int e = 0; e < 3; ++e) { mx[e] = v[2 + e] / W; my[e] = v[5 + e] / W; }
    for (int e = 0; e < 3; ++e)
      for (int f = 0; f < 3; ++f) H[e][f] = v[8 + 3 * e + f] - W * mx[e] * my[f];
    jacobi_svd3(H, U, S, V);
    const double d = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int e = 0; e < 3; ++e) {
      double R[3];
      for (int f = 0; f < 3; ++f) R[f] = V[e][0] * U[f][0] + V[e][1] * U[f][1] + d * V[e][2] * U[f][2];
      for (int f = 0; f < 3; ++f) sT[4 * e + f] = R[f];
      sT[4 * e + 3] = (my[e] + sO[3 + e]) - (R[0] * (mx[0] + sO[0]) + R[1] * (mx[1] + sO[1]) + R[2] * (mx[2] + sO[2]));
    }
    return true;
  }
};

// What the models of point-to-plane and generalized ICP share: the layout of the sums, the origin c (the target
// fragment's first point, so that the cross products stay small) and the solve.  Theirs is accumulate
template <class Wt>
struct SixDofModelT {
  using Args = typename Wt::Args;
  static constexpr bool kWeighted = Wt::kWeighted;
  static constexpr int kSums = 29 + kWeighted;   // n, sum d^2, upper triangle of H [21], g [6], (sum w)
  static constexpr int kMinCorr = 6, kOrigin = 3;
  static constexpr bool kCanFail = true;

  __device__ __forceinline__ static void origin(const IcpArgs& a, const PairRange& g, const double*, double* sC) {
    for (int e = 0; e < 3; ++e) sC[e] = g.t0 < g.t1 ? a.xyz[3 * g.t0 + e] : 0.0;
  }

  // xi = -H^-1 g, then T <- D T in sT with D = [R_inc | xi[3:6] + c - R_inc c], R_inc = Rz(xi2) Ry(xi1) Rx(xi0).
  // false: H is not positive definite to working precision (all weights zero: the first pivot), sT kept
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
using SixDofModel = SixDofModelT<UnitWeight>;   // fgr.hip solves its own 6 x 6 system with it

// Point-to-plane (mvreg.h mvr_icp_refine_plane).  Per match, in registers: of a = [(q - c) x n, n], b = (q - y) . n
// (n the normal of the match y) the upper triangle of sum w a a^T (21) and sum w a b (6); the weight's residual is b
template <class Wt>
struct PointToPlaneT : SixDofModelT<Wt> {
  using Base = SixDofModelT<Wt>;
  using Base::kSums;
  __device__ __forceinline__ static void accumulate(const typename Base::Args& a, const double* sT, const double* sC,
                                                    double (&v)[kSums], int64_t i, int64_t bt, const double (&q)[3],
                                                    double d2) {
    const double n[3] = {a.normals[3 * bt], a.normals[3 * bt + 1], a.normals[3 * bt + 2]};
    const double e[3] = {q[0] - a.xyz[3 * bt], q[1] - a.xyz[3 * bt + 1], q[2] - a.xyz[3 * bt + 2]};
    const double w[3] = {q[0] - sC[0], q[1] - sC[1], q[2] - sC[2]};
    const double ja[6] = {w[1] * n[2] - w[2] * n[1], w[2] * n[0] - w[0] * n[2], w[0] * n[1] - w[1] * n[0],
                          n[0], n[1], n[2]};
    const double b = e[0] * n[0] + e[1] * n[1] + e[2] * n[2];
    const auto wt = Wt::weight(a, [&] { return b; });
    int h = 2;   // (w a_f) a_g: with w == 1.0 the products and their FMAs are those of the unweighted sums
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
      for (int g = f; g < 6; ++g) v[h++] += (wt * ja[f]) * ja[g];
#pragma unroll
    for (int f = 0; f < 6; ++f) v[23 + f] += (wt * ja[f]) * b;
    if constexpr (Base::kWeighted) v[kSums - 1] += wt;
  }
};

// Generalized (mvreg.h mvr_icp_refine_generalized; icp_gicp.hip has the algebra).  Per match, in registers: the two
// normals are loaded, n_s rotated, M inverted and the products formed only once a match is found, so nothing of it is
// live across the search.  The residual of the weight is sqrt(d^T A d); the weight enters as w A
template <class Wt>
struct GeneralizedT : SixDofModelT<Wt> {
  using Base = SixDofModelT<Wt>;
  using Base::kSums;
  __device__ __forceinline__ static void accumulate(const typename Base::Args& a, const double* sT, const double* sC,
                                                    double (&v)[kSums], int64_t i, int64_t bt, const double (&q)[3],
                                                    double d2) {
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
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double e[3] = {q[0] - a.xyz[3 * bt], q[1] - a.xyz[3 * bt + 1], q[2] - a.xyz[3 * bt + 2]};
    const double w[3] = {q[0] - sC[0], q[1] - sC[1], q[2] - sC[2]};
    // The weight scales 1 / det(M), and everything below is linear in A = adj(M) (w / det(M)): with a weight of exactly
    // 1.0 every product and every FMA below is that of the unweighted sums.  A weight applied later would not do: the
    // compiler fuses a term's last product with the addition to its sum (the entries adj * inv of A that enter H as
    // they are, the cross products' second halves), so a product in between rounds once more
    const auto wt = Wt::weight(a, [&] {
      const double dCd = e[0] * (c00 * e[0] + c01 * e[1] + c02 * e[2]) + e[1] * (c01 * e[0] + c11 * e[1] + c12 * e[2]) +
                         e[2] * (c02 * e[0] + c12 * e[1] + c22 * e[2]);
      return sqrt(fmax(dCd * inv, 0.0));   // sqrt(d^T A d)
    });
    const double winv = wt * inv;
    const double A[3][3] = {{c00 * winv, c01 * winv, c02 * winv},
                            {c01 * winv, c11 * winv, c12 * winv},
                            {c02 * winv, c12 * winv, c22 * winv}};
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
    if constexpr (Base::kWeighted) v[kSums - 1] += wt;
  }
};

// Coloured (mvreg.h mvr_icp_refine_colored; Park et al. 2017, Open3D's registration_colored_icp): per match two
// rank-one terms on the point-to-plane layout, the geometric one a_G = [(q - c) x n, n], b_G = (q - y) . n with the
// share lambda, and the photometric one a_I = [(q - c) x dM, dM], b_I = I_s - (I_t + d . (e - b_G n)) with dM =
// -(d - (d . n) n) (d the target's gradient) and the share 1 - lambda.  Each has its own weight, of its residual scaled
// by the root of its share; sum w is sum (lambda w_G + (1 - lambda) w_I), with unit weights the count.  One term is
// added after the other, so only one a of 6 is live beside the sums
template <class Wt>
struct ColoredT : SixDofModelT<Wt> {
  using Base = SixDofModelT<Wt>;
  using Base::kSums;
  using Args = ColoredArgs;
  static constexpr bool kCountIsWeightSum = !Base::kWeighted;

  template <class W>
  __device__ __forceinline__ static void rank_one(double (&v)[kSums], W wt, const double (&w)[3], const double (&m)[3],
                                                  double b) {
    const double ja[6] = {w[1] * m[2] - w[2] * m[1], w[2] * m[0] - w[0] * m[2], w[0] * m[1] - w[1] * m[0],
                          m[0], m[1], m[2]};
    int h = 2;
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
      for (int g = f; g < 6; ++g) v[h++] += (wt * ja[f]) * ja[g];
#pragma unroll
    for (int f = 0; f < 6; ++f) v[23 + f] += (wt * ja[f]) * b;
  }

  __device__ __forceinline__ static void accumulate(const Args& a, const double* sT, const double* sC,
                                                    double (&v)[kSums], int64_t i, int64_t bt, const double (&q)[3],
                                                    double d2) {
    const double lam = a.lambda, oml = 1.0 - a.lambda;
    const double n[3] = {a.normals[3 * bt], a.normals[3 * bt + 1], a.normals[3 * bt + 2]};
    const double e[3] = {q[0] - a.xyz[3 * bt], q[1] - a.xyz[3 * bt + 1], q[2] - a.xyz[3 * bt + 2]};
    const double w[3] = {q[0] - sC[0], q[1] - sC[1], q[2] - sC[2]};
    const double bG = e[0] * n[0] + e[1] * n[1] + e[2] * n[2];
    const auto wG = Wt::weight(a, [&] { return sqrt(lam) * bG; });
    rank_one(v, wG * lam, w, n, bG);
    const double d[3] = {a.grad[3 * bt], a.grad[3 * bt + 1], a.grad[3 * bt + 2]};
    const double dn = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
    const double dM[3] = {-(d[0] - dn * n[0]), -(d[1] - dn * n[1]), -(d[2] - dn * n[2])};
    const double bI = a.intensity[i] - (a.intensity[bt] + (d[0] * (e[0] - bG * n[0]) + d[1] * (e[1] - bG * n[1]) +
                                                           d[2] * (e[2] - bG * n[2])));
    const auto wI = Wt::weight(a, [&] { return sqrt(oml) * bI; });
    rank_one(v, wI * oml, w, dM, bI);
    if constexpr (Base::kWeighted) v[kSums - 1] += wG * lam + wI * oml;
  }
};

// ------------------------------------------------------------------------------------------------------- entry points
// the value checks every entry makes before it looks at P: rindex.hpp's, the ball being the search's.  The pointer
// checks it makes once P > 0 are rindex.hpp's index_pointers_ok
inline bool search_values_ok(int B, int64_t M, int P, double r_index, double max_dist) {
  return P >= 0 && ball_values_ok(B, M, r_index, max_dist);
}

// The checks the ICP entries share, then the args.  MVR_EINVAL comes before P == 0, and P == 0 returns MVR_OK
// before any pointer is looked at: the caller returns whatever this returns when that is not MVR_OK or P == 0
inline int icp_args(IcpArgs& a, const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                    int64_t M, double r_index, const int64_t* pairs, const double* T0, int P, double max_dist,
                    int max_iters, double tol_fitness, double tol_rmse, double* T, double* fitness, double* rmse,
                    int32_t* n_corr, int32_t* iters, int32_t* status, double* trace) {
  if (!search_values_ok(B, M, P, r_index, max_dist) || max_iters < 0 || !(tol_fitness >= 0.0) || !(tol_rmse >= 0.0))
    return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T0 || !T || !fitness || !rmse || !status) return MVR_EINVAL;
  if (!index_pointers_ok(index, index_bytes, xyz, off, M)) return MVR_EINVAL;
  a = IcpArgs{};
  if (M > 0) a.ix = index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T0 = T0;
  a.max_dist = max_dist; a.max_iters = max_iters; a.tol_fitness = tol_fitness; a.tol_rmse = tol_rmse;
  a.T = T; a.fitness = fitness; a.rmse = rmse; a.n_corr = n_corr; a.iters = iters; a.status = status; a.trace = trace;
  return MVR_OK;
}

}  // namespace mvr
