// Fast Global Registration over given correspondences, batched over pairs (mvr_fgr; include/mvreg.h has the
// semantics, DESIGN.md 4.28 the maths and the measurements).
//
// Zhou, Park, Koltun (ECCV 2016), what Open3D offers as registration_fgr_based_on_feature_matching, restated from the
// maths: no hypotheses are sampled and scored; a few dozen Gauss-Newton steps on a Geman-McClure cost whose scale mu
// shrinks (graduated non-convexity) run over a few thousand correspondences.  The only draws are those of the tuple
// filter (mvr_ransac's counter stream), whose comparisons are mvr_ransac_checked's check 2.
//
// One workgroup per pair, every phase and every iteration inside the one launch (as icp_core.hpp's icp_loop), nothing
// atomic, every sum through block_sum in its fixed order: the result is a function of (inputs, seed) alone.
//   1. all n rows: finiteness, the means mu1, mu2 and scale = max |x - mu| (common.hpp's block_sum and block_max);
//   2. the used rows, normalised ((x - mu) / scale), into the pair's slab of the workspace: with the tuple filter the
//      tests are walked in chunks of one test per thread in ascending order, the passing ones appended in order
//      (a 64-bit ballot per wave, per-wave counts through LDS) until max_tuples is reached or the tests are exhausted;
//      without it every row.  The slab (6 doubles per used row, at most 144 KB at the defaults) does not fit the 64 KB
//      of LDS a workgroup can have; it is written and read by the one workgroup and stays in its L2;
//   3. the loop: 17 sums per iteration (sum w, w p', w p' p'^T, w p' x e, w e, w |e|^2) give H and g of
//      J = [-[p']x | I]; lane 0 solves (icp_core.hpp solve6) and updates T (SixDofModel::solve, origin 0);
//   4. T back in the clouds' units; fitness and rmse over all n rows as mvr_ransac scores a hypothesis.
#include "icp_core.hpp"
#include "ransac.hpp"

namespace mvr {

// The loop is a stream of independent rows (no search, no dependent loads): it does not need the 16 waves of the ICP
// kernels to hide latency.  128 VGPRs at 256 and 512 threads, 124 at 1024, no scratch, 664 / 1224 / 2344 B of LDS.
// Measured on 435 pairs x 2000 rows, tuple filter on / off: 256 threads 2.09 / 0.90 ms, 512 threads
// 1.99 / 1.14 ms, 1024 threads 3.3 / 2.6 ms (one workgroup per CU: 435 pairs take two rounds of the 256 CUs).  The
// tuple phase (draws, gathers, one chunk of tests per pass) gains from more threads, the loop (17 sums, two barriers,
// one lane's solve per iteration) from fewer waves at its barriers; the filter is on by default, so 512
#ifndef MVR_FGR_THREADS
#define MVR_FGR_THREADS 512
#endif
constexpr int kFgrThreads = MVR_FGR_THREADS;
constexpr int kFgrSums = 17;

struct FgrArgs {
  const double* x1; const double* x2; int64_t ps; const int32_t* n;
  int n_max, iters, tuple_factor, max_tuples;
  int64_t cap;                       // rows of a pair's slab
  double max_dist, div, s2;
  uint64_t seed;
  double* T; double* fitness; double* rmse; int32_t* n_used; int32_t* n_tuples; int32_t* status; double* trace;
  double* pts;                       // [P][cap][6]: the used rows, normalised (p, q)
};

template <int kThreads>
__device__ __forceinline__ void fgr_pair(const FgrArgs& a) {
  constexpr int kWaves = kThreads / 64;
  __shared__ double red[kFgrSums * kWaves];
  __shared__ double sT[12];
  __shared__ int sCnt[kWaves];
  __shared__ int sBad;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n[p];
  const double* x1 = a.x1 + (int64_t)p * a.ps;
  const double* x2 = a.x2 + (int64_t)p * a.ps;
  double* pts = a.pts + (int64_t)p * a.cap * 6;
  double* trace = a.trace ? a.trace + (int64_t)p * a.iters * 2 : nullptr;
  double* To = a.T + 16 * (int64_t)p;

  // bits 1 and 4: the identity, nothing evaluated, no row used (every test below is uniform)
  auto give_up = [&](int status) {
    if (tid == 0) {
      for (int q = 0; q < 16; ++q) To[q] = (q % 5 == 0) ? 1.0 : 0.0;
      a.fitness[p] = 0.0;
      a.rmse[p] = 0.0;
      a.n_used[p] = 0;
      a.n_tuples[p] = 0;
      a.status[p] = status;
    }
    if (trace)
      for (int64_t e = tid; e < 2 * (int64_t)a.iters; e += kThreads) trace[e] = -1.0;
  };
  if (n < 0 || n > a.n_max) return give_up(4);   // a count the rows cannot hold

  // ---- 1. finiteness, means, scale over all n rows
  double v[kFgrSums];
  {
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kThreads) {
      bool fin = true;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const double u = x1[3 * (int64_t)i + e], w = x2[3 * (int64_t)i + e];
        fin = fin && isfinite(u) && isfinite(w);
        s[e] += u;
        s[3 + e] += w;
      }
      if (!fin) s[6] = 1.0;
    }
    s[6] = block_max(s[6], red);   // a flag, kept apart from the sums a NaN would spoil
    if (s[6] != 0.0) return give_up(4);
    if (n < 3) return give_up(1);
    block_sum<7>(s, red);
#pragma unroll
    for (int e = 0; e < 6; ++e) v[e] = s[e] / (double)n;
  }
  const double mu1[3] = {v[0], v[1], v[2]}, mu2[3] = {v[3], v[4], v[5]};
  double far2 = 0.0;
  for (int i = tid; i < n; i += kThreads) {
    double r1 = 0.0, r2 = 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double u = x1[3 * (int64_t)i + e] - mu1[e], w = x2[3 * (int64_t)i + e] - mu2[e];
      r1 += u * u;
      r2 += w * w;
    }
    far2 = fmax(far2, fmax(r1, r2));
  }
  const double scale = sqrt(block_max(far2, red));
  if (!(scale > 0.0)) return give_up(1);

  auto put = [&](int64_t slot, int64_t row) {   // used row `slot` <- given row `row`, normalised
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      pts[6 * slot + e] = (x1[3 * row + e] - mu1[e]) / scale;
      pts[6 * slot + 3 + e] = (x2[3 * row + e] - mu2[e]) / scale;
    }
  };

  // ---- 2. the used rows
  auto edge_ok = [&](int64_t i, int64_t j) {   // check 2 of mvr_ransac_checked on rows i, j
    return ransac_edge_ok(x1 + 3 * i, x1 + 3 * j, x2 + 3 * i, x2 + 3 * j, a.s2);
  };
  int n_tuples = 0, m = n;
  if (a.tuple_factor > 0) {   // uniform
    const int64_t total = (int64_t)a.tuple_factor * n;   // < 2^31 (checked by the entry point)
    int count = 0;                                       // passing tests so far, uniform
    for (int64_t base = 0; base < total && count < a.max_tuples; base += kThreads) {
      const int64_t it = base + tid;
      int64_t c[3] = {0, 0, 0};
      bool ok = it < total;
      if (ok) {
        ransac_draws(a.seed, p, (uint64_t)it, n, 3, c);
        ok = c[0] != c[1] && c[0] != c[2] && c[1] != c[2];
        if (ok) ok = edge_ok(c[0], c[1]) && edge_ok(c[0], c[2]) && edge_ok(c[1], c[2]);
      }
      const unsigned long long mask = __ballot(ok);
      const int pre = __popcll(mask & ((1ull << lane) - 1ull));
      if (lane == 0) sCnt[wave] = __popcll(mask);
      __syncthreads();
      int off = count, tot = 0;
      for (int w = 0; w < kWaves; ++w) {
        if (w < wave) off += sCnt[w];
        tot += sCnt[w];
      }
      const int slot = off + pre;
      if (ok && slot < a.max_tuples)
        for (int j = 0; j < 3; ++j) put(3 * (int64_t)slot + j, c[j]);
      count += tot;
      __syncthreads();   // sCnt is rewritten by the next chunk
    }
    n_tuples = min(count, a.max_tuples);
    m = 3 * n_tuples;
    if (m < 3) return give_up(1);
  } else {
    for (int i = tid; i < n; i += kThreads) put(i, i);
  }
  if (tid == 0) {
    for (int q = 0; q < 12; ++q) sT[q] = (q % 5 == 0) ? 1.0 : 0.0;
    sBad = 0;
  }
  __syncthreads();   // the slab and sT: written above, read by other threads below

  // ---- 3. graduated non-convexity
  const double delta = a.max_dist / scale, delta2 = delta * delta;
  double mu = 1.0;
  int status = 0, k = 0;
  for (; k < a.iters; ++k) {
    if (k % 4 == 0 && mu > delta2) mu = mu / a.div;
    double R[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) R[q] = sT[q];
#pragma unroll
    for (int q = 0; q < kFgrSums; ++q) v[q] = 0.0;
    for (int i = tid; i < m; i += kThreads) {
      const double* r = pts + 6 * (int64_t)i;
      const double px = r[0], py = r[1], pz = r[2];
      const double x = R[0] * px + R[1] * py + R[2] * pz + R[3];
      const double y = R[4] * px + R[5] * py + R[6] * pz + R[7];
      const double z = R[8] * px + R[9] * py + R[10] * pz + R[11];
      const double ex = x - r[3], ey = y - r[4], ez = z - r[5];
      const double e2 = ex * ex + ey * ey + ez * ez;
      const double g = mu / (e2 + mu), w = g * g;
      const double wx = w * x, wy = w * y, wz = w * z;
      v[0] += w;
      v[1] += wx; v[2] += wy; v[3] += wz;
      v[4] += wx * x; v[5] += wx * y; v[6] += wx * z; v[7] += wy * y; v[8] += wy * z; v[9] += wz * z;
      v[10] += w * (y * ez - z * ey); v[11] += w * (z * ex - x * ez); v[12] += w * (x * ey - y * ex);
      v[13] += w * ex; v[14] += w * ey; v[15] += w * ez;
      v[16] += w * e2;
    }
    block_sum<kFgrSums>(v, red);
    if (tid == 0) {
      if (trace) { trace[2 * k] = mu; trace[2 * k + 1] = v[16] / (double)m; }
      // H = [[sum w (|p'|^2 I - p' p'^T), [s]x], [., sum w I]] with s = sum w p', upper triangle in row order;
      // g = [sum w p' x e, sum w e]
      const double h[SixDofModel::kSums] = {
          0.0, 0.0,
          v[7] + v[9], -v[5], -v[6], 0.0, -v[3], v[2],
          v[4] + v[9], -v[8], v[3], 0.0, -v[1],
          v[4] + v[7], -v[2], v[1], 0.0,
          v[0], 0.0, 0.0,
          v[0], 0.0,
          v[0],
          v[10], v[11], v[12], v[13], v[14], v[15]};
      const double zero[3] = {0.0, 0.0, 0.0};
      sBad = !SixDofModel::solve(h, sT, zero);
    }
    __syncthreads();   // block_sum's barriers separate this iteration's reads of sT from the solve
    if (sBad) { status |= 8; ++k; break; }   // uniform: T kept, row k of the trace written
  }
  if (trace)
    for (int64_t e = 2 * (int64_t)k + tid; e < 2 * (int64_t)a.iters; e += kThreads) trace[e] = -1.0;

  // ---- 4. T in the clouds' units, scored over all n rows
  __syncthreads();
  if (tid == 0) {
    for (int e = 0; e < 3; ++e) {
      const double* r = sT + 4 * e;
      sT[4 * e + 3] = scale * r[3] + mu2[e] - (r[0] * mu1[0] + r[1] * mu1[1] + r[2] * mu1[2]);
    }
    for (int q = 0; q < 12; ++q) To[q] = sT[q];
    To[12] = 0.0; To[13] = 0.0; To[14] = 0.0; To[15] = 1.0;
  }
  __syncthreads();
  const double d2max = a.max_dist * a.max_dist;
  double s[2] = {0.0, 0.0};
  for (int i = tid; i < n; i += kThreads) {
    const double dd = ransac_row_d2<4, 4>(sT, sT + 3, x1 + 3 * (int64_t)i, x2 + 3 * (int64_t)i);
    if (dd < d2max) {
      s[0] += 1.0;
      s[1] += dd;
    }
  }
  block_sum<2>(s, red);
  if (tid == 0) {
    a.fitness[p] = s[0] / (double)n;
    a.rmse[p] = s[0] > 0.0 ? sqrt(s[1] / s[0]) : 0.0;
    a.n_used[p] = m;
    a.n_tuples[p] = n_tuples;
    a.status[p] = status;
  }
}

__global__ __launch_bounds__(kFgrThreads) void fgr_kernel(FgrArgs a) { fgr_pair<kFgrThreads>(a); }

static size_t fgr_rows(int n_max, int max_tuples) {
  const size_t t = 3 * (size_t)(max_tuples > 0 ? max_tuples : 0), r = (size_t)(n_max > 0 ? n_max : 0);
  return t > r ? t : r;
}

}  // namespace mvr

// per pair a slab of max(n_max, 3 max_tuples) used rows of 6 doubles
extern "C" size_t mvr_fgr_workspace_bytes(int P, int n_max, int max_tuples) {
  if (P <= 0) return 0;
  return (size_t)P * mvr::fgr_rows(n_max, max_tuples) * 6 * sizeof(double);
}

extern "C" int mvr_fgr(const double* x1, const double* x2, int64_t x_pstride, const int32_t* n, int P, double max_dist,
                       int iters, double division_factor, int tuple_factor, int max_tuples, double tuple_scale,
                       uint64_t seed, double* T, double* fitness, double* rmse, int32_t* n_used, int32_t* n_tuples,
                       int32_t* status, double* trace, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (P < 0 || P >= (1 << 23) || iters < 0 || !(max_dist > 0.0) || !isfinite(max_dist) ||
      !isfinite(division_factor) || !(division_factor > 1.0) || tuple_factor < 0 || max_tuples < 1 ||
      x_pstride < 0)
    return MVR_EINVAL;
  if (tuple_factor > 0 && !(tuple_scale > 0.0 && tuple_scale <= 1.0)) return MVR_EINVAL;
  const int64_t n_max64 = x_pstride / 3;
  if (n_max64 >= ((int64_t)1 << 31) || (int64_t)tuple_factor * n_max64 >= ((int64_t)1 << 31)) return MVR_EINVAL;
  const int n_max = (int)n_max64;
  if (workspace_bytes < mvr_fgr_workspace_bytes(P, n_max, max_tuples)) return MVR_EINVAL;
  if (P == 0) return MVR_OK;
  if (!x1 || !x2 || !n || !T || !fitness || !rmse || !n_used || !n_tuples || !status) return MVR_EINVAL;
  const size_t rows = mvr::fgr_rows(n_max, max_tuples);
  if (rows > 0 && !workspace) return MVR_EINVAL;
  mvr::FgrArgs a{};
  a.x1 = x1; a.x2 = x2; a.ps = x_pstride; a.n = n;
  a.n_max = n_max; a.iters = iters; a.tuple_factor = tuple_factor; a.max_tuples = max_tuples;
  a.cap = (int64_t)rows;
  a.max_dist = max_dist; a.div = division_factor; a.s2 = tuple_scale * tuple_scale; a.seed = seed;
  a.T = T; a.fitness = fitness; a.rmse = rmse; a.n_used = n_used; a.n_tuples = n_tuples; a.status = status;
  a.trace = trace;
  a.pts = static_cast<double*>(workspace);
  hipLaunchKernelGGL(mvr::fgr_kernel, dim3(P), dim3(mvr::kFgrThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
