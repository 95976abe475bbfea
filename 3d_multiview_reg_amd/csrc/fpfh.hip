// FPFH descriptors on the radius index of overlap.hip (mvreg.h mvr_compute_fpfh): the Fast Point
// Feature Histogram of Rusu et al. (PCL's FPFHEstimation, Open3D's compute_fpfh_feature) restated from the maths.
//
// Two launches, one thread per point in both, fp64 geometry, no atomics.  Thread s takes the point at position s of
// the index's sorted order and walks its ball with rindex.hpp's ball_walk, as normals.hip does.
//   spfh_kernel: the three angular features of every (point, neighbour) pair, binned into 3 x 11 integer counters;
//                the counters live in LDS, one column per thread (a register array indexed by a computed bin would go
//                to scratch), and leave as 100 count / k in fp64 to the workspace row s (the sorted position: the
//                second pass then reads a cell's rows contiguously) and, rounded, to spfh_out.
//   fpfh_kernel: sum of the neighbours' SPFH rows weighted by 1 / d^2 in 33 statically indexed fp64 registers, each
//                group of 11 scaled to 100, plus the point's own row.
// Every loop is bounded: 27 cells, a cell's rows, 33 bins, and the hash probe (cap >= 2 M).
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

constexpr int kFpfhThreads = 64;
constexpr int kFpfhBins = 33;
// the counters' column stride in 32-bit words: odd, so the lanes of a wave that hit the same bin sit in 64 different
// banks.  32-bit counters: a count is at most k_i < M < 2^31, so there is no overflow case to check
constexpr int kFpfhStride = kFpfhThreads + 1;

__device__ __forceinline__ int bin11(double x) {   // x in bin units; NaN converts to 0
  const int b = (int)floor(x);
  return b < 0 ? 0 : (b > 10 ? 10 : b);
}

__global__ __launch_bounds__(kFpfhThreads) void spfh_kernel(RIndex ix, const double* __restrict__ xyz,
                                                            const double* __restrict__ normals, int64_t M, double r,
                                                            double radius, double* __restrict__ spfh_ws,
                                                            float* __restrict__ spfh_out) {
  __shared__ uint32_t cnt[kFpfhBins * kFpfhStride];
  const int64_t s = (int64_t)blockIdx.x * kFpfhThreads + threadIdx.x;
  if (s >= M) return;   // no barrier below: a thread touches its own column only
  uint32_t* my = cnt + threadIdx.x;
#pragma unroll
  for (int c = 0; c < kFpfhBins; ++c) my[c * kFpfhStride] = 0u;
  int64_t i;
  int b, k = 0;
  double p[3];
  point_at(ix, xyz, s, i, b, p);
  const double ni[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  const double kPi = 3.14159265358979323846;
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t t, int, double ex, double ey, double ez) {
    if (t == i) return;
    ++k;
    const double d = sqrt(ex * ex + ey * ey + ez * ez);
    if (d == 0.0) return;
    const double nj[3] = {normals[3 * t], normals[3 * t + 1], normals[3 * t + 2]};
    const double a1 = (ni[0] * ex + ni[1] * ey + ni[2] * ez) / d;
    const double a2 = (nj[0] * ex + nj[1] * ey + nj[2] * ez) / d;
    const bool swap = fabs(a1) < fabs(a2);
    const double na0 = swap ? nj[0] : ni[0], na1 = swap ? nj[1] : ni[1], na2 = swap ? nj[2] : ni[2];
    const double nb0 = swap ? ni[0] : nj[0], nb1 = swap ? ni[1] : nj[1], nb2 = swap ? ni[2] : nj[2];
    const double f2 = swap ? -a2 : a1;
    if (swap) { ex = -ex; ey = -ey; ez = -ez; }
    double v0 = ey * na2 - ez * na1, v1 = ez * na0 - ex * na2, v2 = ex * na1 - ey * na0;   // e x n_a
    const double vl = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    if (!(vl > 0.0)) return;
    v0 /= vl; v1 /= vl; v2 /= vl;
    const double w0 = na1 * v2 - na2 * v1, w1 = na2 * v0 - na0 * v2, w2 = na0 * v1 - na1 * v0;   // n_a x v
    const double f0 = atan2(w0 * nb0 + w1 * nb1 + w2 * nb2, na0 * nb0 + na1 * nb1 + na2 * nb2);
    const double f1 = v0 * nb0 + v1 * nb1 + v2 * nb2;
    my[bin11(11.0 * (f0 + kPi) / (2.0 * kPi)) * kFpfhStride] += 1u;
    my[(11 + bin11(11.0 * (f1 + 1.0) / 2.0)) * kFpfhStride] += 1u;
    my[(22 + bin11(11.0 * (f2 + 1.0) / 2.0)) * kFpfhStride] += 1u;
  });
  const double dk = (double)k;
#pragma unroll
  for (int cb = 0; cb < kFpfhBins; ++cb) {
    const double h = k > 0 ? 100.0 * (double)my[cb * kFpfhStride] / dk : 0.0;
    spfh_ws[s * kFpfhBins + cb] = h;
    if (spfh_out) spfh_out[i * kFpfhBins + cb] = (float)h;
  }
}

__global__ __launch_bounds__(kFpfhThreads) void fpfh_kernel(RIndex ix, const double* __restrict__ xyz, int64_t M,
                                                            double r, double radius,
                                                            const double* __restrict__ spfh_ws,
                                                            float* __restrict__ fpfh) {
  const int64_t s = (int64_t)blockIdx.x * kFpfhThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b;
  double p[3], acc[kFpfhBins];
  point_at(ix, xyz, s, i, b, p);
#pragma unroll
  for (int cb = 0; cb < kFpfhBins; ++cb) acc[cb] = 0.0;
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t t, int j, double ex, double ey, double ez) {
    const double d2 = ex * ex + ey * ey + ez * ez;
    if (t == i || !(d2 > 0.0)) return;
    const double wgt = 1.0 / d2;
    const double* row = spfh_ws + (int64_t)j * kFpfhBins;   // the neighbour's row, by its sorted position
#pragma unroll
    for (int cb = 0; cb < kFpfhBins; ++cb) acc[cb] += row[cb] * wgt;
  });
  const double* own = spfh_ws + s * kFpfhBins;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    double sum = 0.0;
#pragma unroll
    for (int cb = 0; cb < 11; ++cb) sum += acc[11 * g + cb];
    const double scale = sum > 0.0 ? 100.0 / sum : 1.0;
#pragma unroll
    for (int cb = 0; cb < 11; ++cb)
      fpfh[i * kFpfhBins + 11 * g + cb] = (float)(acc[11 * g + cb] * scale + own[11 * g + cb]);
  }
}

}  // namespace mvr

extern "C" size_t mvr_compute_fpfh_workspace_bytes(int64_t M) {
  return ((size_t)(M > 0 ? M : 1) * mvr::kFpfhBins * sizeof(double) + 255) & ~(size_t)255;
}

extern "C" int mvr_compute_fpfh(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                                const int64_t* off, int B, int64_t M, double r_index, double radius, float* fpfh,
                                float* spfh_out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, radius)) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !normals || !fpfh || !workspace ||
      workspace_bytes < mvr_compute_fpfh_workspace_bytes(M))
    return MVR_EINVAL;
  double* ws = reinterpret_cast<double*>(workspace);
  const int rc = mvr::launch_per_point<mvr::kFpfhThreads>(mvr::spfh_kernel, index, M, 0, stream, xyz, normals, M, r_index,
                                                          radius, ws, spfh_out);
  if (rc != MVR_OK) return rc;
  return mvr::launch_per_point<mvr::kFpfhThreads>(mvr::fpfh_kernel, index, M, 0, stream, xyz, M, r_index, radius, ws,
                                                  fpfh);
}
