// Outlier statistics on a fragment's own points (mvreg.h mvr_statistical_outlier, mvr_radius_count):
// what Open3D's remove_statistical_outlier and remove_radius_outlier decide on, restated from the maths, each fragment
// its own cloud.
//
// statistical_kernel: one workgroup per fragment.  Thread t takes the rows t, t + 256, ... of the fragment in that
// order and the workgroup's sums go through one fixed tree in LDS, so thresholds and masks are bit-identical from run
// to run and a fragment's outputs do not depend on the batch around it.  Three passes over the fragment's rows: the
// mean distances and their sum, the squared deviations, the mask.
// radius_count_kernel: one thread per point in the index's sorted order, the ball walk of rindex.hpp.
#include "common.hpp"
#include "rindex.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

constexpr int kStatThreads = 256;
constexpr int kCountThreads = 64;   // as normals.hip: nothing is shared between a workgroup's waves

// the sum of v over the workgroup by a fixed tree, in every thread
__device__ __forceinline__ double tree_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = kStatThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kStatThreads) void statistical_kernel(const double* __restrict__ dist2,
                                                                   const int64_t* __restrict__ off, int64_t M, int k,
                                                                   double std_ratio, uint8_t* __restrict__ keep,
                                                                   double* __restrict__ mean_dist,
                                                                   double* __restrict__ thr) {
#pragma clang fp contract(off)
  __shared__ double red[kStatThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  int64_t t0, t1;
  frag_rows(off, b, M, t0, t1);
  const int64_t n_b = t1 - t0;   // uniform over the workgroup, as every branch on it below
  const double found = (double)(n_b < k ? n_b : k);
  double acc = 0.0;
  for (int64_t i = t0 + tid; i < t1; i += kStatThreads) {
    const double* d = dist2 + i * k;
    double s = 0.0;
    for (int q = 0; q < k; ++q)
      if (d[q] < (double)INFINITY) s += sqrt(d[q]);   // ascending slots; padding (+inf) and NaN add nothing
    const double m = s / found;
    mean_dist[i] = m;
    acc += m;
  }
  if (n_b < 2) {   // no deviation to speak of: everything is kept
    for (int64_t i = t0 + tid; i < t1; i += kStatThreads) keep[i] = 1;
    if (tid == 0) thr[b] = (double)INFINITY;
    return;
  }
  const double mu = tree_sum(acc, red) / (double)n_b;
  acc = 0.0;
  for (int64_t i = t0 + tid; i < t1; i += kStatThreads) {   // the rows this thread wrote above
    const double e = mean_dist[i] - mu;
    acc += e * e;
  }
  const double sd = sqrt(tree_sum(acc, red) / (double)(n_b - 1));
  const double th = mu + std_ratio * sd;
  for (int64_t i = t0 + tid; i < t1; i += kStatThreads) keep[i] = mean_dist[i] < th ? 1 : 0;
  if (tid == 0) thr[b] = th;
}

__global__ __launch_bounds__(kCountThreads) void radius_count_kernel(RIndex ix, const double* __restrict__ xyz,
                                                                     int64_t M, double r, double radius,
                                                                     int32_t* __restrict__ count) {
  const int64_t s = (int64_t)blockIdx.x * kCountThreads + threadIdx.x;
  if (s >= M) return;
  int64_t i;
  int b, n = 0;
  double p[3];
  point_at(ix, xyz, s, i, b, p);
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t, int, double, double, double) { ++n; });
  count[i] = n;
}

}  // namespace mvr

extern "C" int mvr_statistical_outlier(const double* dist2, const int64_t* off, int B, int64_t M, int k,
                                       double std_ratio, uint8_t* keep, double* mean_dist, double* thr,
                                       hipStream_t stream) {
  if (M < 0 || M > 0x7fffffff || B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (k < 1 || k > 64 || !(std_ratio > 0.0)) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed, thr is not written
  if (!dist2 || !off || !keep || !mean_dist || !thr) return MVR_EINVAL;
  hipLaunchKernelGGL(mvr::statistical_kernel, dim3((unsigned)B), dim3(mvr::kStatThreads), 0, stream, dist2, off, M, k,
                     std_ratio, keep, mean_dist, thr);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}

extern "C" int mvr_radius_count(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                                int64_t M, double r_index, double radius, int32_t* count, hipStream_t stream) {
  if (!mvr::ball_values_ok(B, M, r_index, radius)) return MVR_EINVAL;
  if (M == 0) return MVR_OK;   // no points: NULL pointers allowed
  if (!mvr::index_pointers_ok(index, index_bytes, xyz, off, M) || !count) return MVR_EINVAL;
  return mvr::launch_per_point<mvr::kCountThreads>(mvr::radius_count_kernel, index, M, 0, stream, xyz, M, r_index,
                                                   radius, count);
}
