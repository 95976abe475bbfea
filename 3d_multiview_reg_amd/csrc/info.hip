// Per-pair 6 x 6 information matrices on the radius index of overlap.hip (mvreg.h mvr_pair_information; DESIGN.md
// 4.22): what Open3D's get_information_matrix_from_point_clouds gives a pose graph's edge, restated from the maths.
// With G_y = [ I | -[y]x ] per valid correspondence (y the matched target point), info = sum G_y^T G_y in the
// parameter order (translation, rotation).  Open3D parity and parity with Redwood's published .info files are
// unpinned (mvreg.h).
//
// One workgroup per pair, fp64 throughout.  The correspondences are those of an evaluation in the ICP kernels: the
// same nearest_row of icp_core.hpp finds them.
//   sums     eleven per thread: n, sum d^2, sum y [3] and the six distinct entries of sum y y^T, about the target
//            frame's origin (the matrix is defined about it: there is no origin to choose)
//   reduce   block_sum: a lane tree, then the waves in index order through LDS.  No atomics and no workspace, so a
//            pair's bits do not depend on the batch around it
//   assemble lane 0: [ n I, -[sum y]x ; [sum y]x, tr(S) I - S ]
// Every loop is bounded: the source points, the 27 cells, and the hash probe (cap >= 2 M ends it at an empty slot).
#include "icp_core.hpp"

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
  double* out = a.info + 36 * (int64_t)p;
  const double* T = a.T + 12 * (int64_t)p;
  const PairRange g = pair_range(a.pairs, T, a.off, a.B, a.M, p);
  if (!g.ok) {   // uniform
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
  for (int64_t i = g.s0 + tid; i < g.s1; i += kInfoThreads) {
    double q[3], best;
    moved_point(sT, a.xyz, i, q);
    const int64_t bt = nearest_row(a.ix, a.xyz, g.tf, q, r, slack, md2, a.max_dist, best);
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
  if (!mvr::search_values_ok(B, M, P, r_index, max_dist)) return MVR_EINVAL;
  if (P == 0) return MVR_OK;   // no pairs: NULL pointers allowed
  if (!pairs || !T || !info || !rmse || !status) return MVR_EINVAL;
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M)) return MVR_EINVAL;
  mvr::InfoArgs a{};
  if (M > 0) a.ix = mvr::index_view(const_cast<void*>(index), M);
  a.xyz = xyz; a.off = M > 0 ? off : nullptr; a.B = B; a.M = M; a.r = r_index;
  a.pairs = pairs; a.T = T; a.max_dist = max_dist;
  a.info = info; a.n_corr = n_corr; a.rmse = rmse; a.status = status;
  hipLaunchKernelGGL(mvr::info_kernel, dim3(P), dim3(mvr::kInfoThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
