// Per-pair 6 x 6 information matrices on the radius index of overlap.hip (mvreg.h mvr_pair_information; DESIGN.md
// 4.22): what Open3D's get_information_matrix_from_point_clouds gives a pose graph's edge, restated from the maths.
// With G_y = [ I | -[y]x ] per valid correspondence (y the matched target point), info = sum G_y^T G_y in the
// parameter order (translation, rotation).  Open3D parity and parity with Redwood's published .info files are
// unpinned (mvreg.h).
//
// One workgroup per pair, fp64 throughout.  The correspondences are those of eval(T) in icp.hip; that file is pinned
// bit for bit by its tests and stays as it is, so the 27-cell walk below is a copy of its search:
//   search   threads stride over the source points; q = R x + t walks the 27 cells around floor(q / r_index) through
//            the cell hash, centre cell first; nearest by squared distance, the lowest row on a tie
//   sums     eleven per thread: n, sum d^2, sum y [3] and the six distinct entries of sum y y^T, about the target
//            frame's origin (the matrix is defined about it: there is no origin to choose)
//   reduce   block_sum: a lane tree, then the waves in index order through LDS.  No atomics and no workspace, so a
//            pair's bits do not depend on the batch around it
//   assemble lane 0: [ n I, -[sum y]x ; [sum y]x, tr(S) I - S ]
// Every loop is bounded: the source points, the 27 cells, and the hash probe (cap >= 2 M ends it at an empty slot).
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// 16 waves = 4 per SIMD, as icp.hip: the search is a chain of dependent loads and the other waves hide it.  With
// eleven sums instead of seventeen the kernel fits the 128 VGPRs of this size without a spill
#ifndef MVR_INFO_THREADS
#define MVR_INFO_THREADS 1024
#endif
constexpr int kInfoThreads = MVR_INFO_THREADS;
constexpr int kInfoSums = 11;   // n, sum d^2, sum y [3], sum y y^T (xx xy xz yy yz zz)

struct InfoArgs {
  RIndex ix;
  const double* xyz; const int64_t* off; int B; int64_t M; double r;
  const int64_t* pairs; const double* T;
  double max_dist;
  double* info; int32_t* n_corr; double* rmse; int32_t* status;
};

__global__ __launch_bounds__(kInfoThreads) void info_kernel(InfoArgs a) {
  __shared__ double red[kInfoSums * (kInfoThreads / 64)];
  __shared__ double sT[12];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t sf = a.pairs[2 * (int64_t)p], tf = a.pairs[2 * (int64_t)p + 1];
  double* out = a.info + 36 * (int64_t)p;

  const double* T = a.T + 12 * (int64_t)p;
  bool ok = sf >= 0 && sf < a.B && tf >= 0 && tf < a.B;
  for (int q = 0; q < 12; ++q) ok = ok && isfinite(T[q]);
  int64_t s0 = 0, s1 = 0;
  if (ok && a.off) {
    s0 = a.off[sf];
    s1 = a.off[sf + 1];
    ok = s0 >= 0 && s0 <= s1 && s1 <= a.M && a.off[tf] >= 0 && a.off[tf + 1] <= a.M;
  }
  if (!ok) {   // uniform
    if (tid < 36) out[tid] = 0.0;
    if (tid == 0) {
      a.rmse[p] = 0.0;
      if (a.n_corr) a.n_corr[p] = 0;
      a.status[p] = 4;
    }
    return;
  }
  if (tid < 12) sT[tid] = T[tid];
  __syncthreads();
  const double r = a.r, slack = 1e-9 * a.r, md2 = a.max_dist * a.max_dist * (1.0 + 1e-9);

  double v[kInfoSums];
#pragma unroll
  for (int q = 0; q < kInfoSums; ++q) v[q] = 0.0;
  for (int64_t i = s0 + tid; i < s1; i += kInfoThreads) {
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
      const double y0 = a.xyz[3 * bt], y1 = a.xyz[3 * bt + 1], y2 = a.xyz[3 * bt + 2];
      v[0] += 1.0;
      v[1] += best;
      v[2] += y0; v[3] += y1; v[4] += y2;
      v[5] += y0 * y0; v[6] += y0 * y1; v[7] += y0 * y2;
      v[8] += y1 * y1; v[9] += y1 * y2; v[10] += y2 * y2;
    }
  }
  block_sum<kInfoSums>(v, red);

  if (tid == 0) {
    const double n = v[0], tr = v[5] + v[8] + v[10];
    const double S[3][3] = {{v[5], v[6], v[7]}, {v[6], v[8], v[9]}, {v[7], v[9], v[10]}};
    // [sum y]x
    const double C[3][3] = {{0.0, -v[4], v[3]}, {v[4], 0.0, -v[2]}, {-v[3], v[2], 0.0}};
    for (int e = 0; e < 3; ++e)
      for (int f = 0; f < 3; ++f) {
        out[6 * e + f] = e == f ? n : 0.0;
        out[6 * e + 3 + f] = -C[e][f];
        out[6 * (3 + e) + f] = C[e][f];
        out[6 * (3 + e) + 3 + f] = (e == f ? tr : 0.0) - S[e][f];
      }
    a.rmse[p] = n > 0.0 ? sqrt(v[1] / n) : 0.0;
    if (a.n_corr) a.n_corr[p] = (int)n;
    a.status[p] = 0;
  }
}

}  // namespace mvr

extern "C" int mvr_pair_information(const void* index, size_t index_bytes, const double* xyz, const int64_t* off,
                                    int B, int64_t M, double r_index, const int64_t* pairs, const double* T, int P,
                                    double max_dist, double* info, int32_t* n_corr, double* rmse, int32_t* status,
                                    hipStream_t stream) {
  if (P < 0 || M < 0 || M > 0x7fffffff || B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (!(max_dist > 0.0) || !(r_index > 0.0) || max_dist > r_index) return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T || !info || !rmse || !status) return MVR_EINVAL;
  if (M > 0 && (!index || !xyz || !off || index_bytes < mvr_radius_index_bytes(M))) return MVR_EINVAL;
  mvr::InfoArgs a{};
  if (M > 0) a.ix = mvr::index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T = T; a.max_dist = max_dist;
  a.info = info; a.n_corr = n_corr; a.rmse = rmse; a.status = status;
  hipLaunchKernelGGL(mvr::info_kernel, dim3(P), dim3(mvr::kInfoThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
