// RANSAC over given correspondences, batched over pairs: mvr_ransac, and mvr_ransac_checked with correspondence
// checkers and a validation cap (include/mvreg.h has the semantics, DESIGN.md 4.26 the measurements).
//
// mvr_ransac: lib/utils.py:671-709 run_ransac ->
// Open3D 0.9 registration_ransac_based_on_correspondence(TransformationEstimationPointToPoint(False),
// ransac_n = 4, max_correspondence_distance = 0.05, RANSACConvergenceCriteria(50000, 2500)).
// Open3D 0.9's loop (restated; oracle/ransac.py): min(max_iteration, max_validation) iterations; each draws
// ransac_n correspondences with replacement, fits R, t by Umeyama without scaling (fp64), and scores the
// fit over ALL correspondences: inlier iff |R x1 + t - x2|^2 < d^2, fitness = inliers / n,
// rmse = sqrt(sum of inlier d^2 / inliers); the result is the first hypothesis that is best by (fitness
// desc, rmse asc) among those with fitness > 0, identity when none (or n < ransac_n).  Open3D seeds
// std::rand from the clock; here the draws are a counter stream over (seed, pair, iteration, draw)
// (ransac.hpp ransac_draws) — reproducible, and the same on the host (oracle/ransac.py:draws).
//
// One thread per (pair, hypothesis): its draws, the Umeyama fit (jacobi_svd3), then a sequential pass
// over the pair's correspondences staged through LDS in 256-row tiles (every thread of the workgroup reads
// the same row: LDS broadcast), in correspondence order and with rounded fp64 ops (no contraction), so the
// counts and error sums equal the host restatement's bit for bit.  A second kernel picks each pair's best.
// Work per pair: iters x n x ~15 fp64 ops (2500 x 5000: 0.19 GFLOP) — fp64 VALU-bound.
//
// mvr_ransac_checked: what Open3D's global-registration examples configure: 3-point samples, the edge-length (0.9),
// distance and normal checkers, 100000 iterations, of which only the samples that pass every checker are scored against
// all correspondences.  Scoring is the expensive step (n x ~27 fp64 ops per hypothesis); the checkers need the sample's
// own points only, so 40 times mvr_ransac's draws cost less than its 2500 evaluations.  No confidence-based early
// exit: when to stop depends on each pair's running best, which a batched launch of all iterations does not have.
//
// Four launches, nothing atomic, every result a function of (inputs, seed) alone:
//   rc_check_kernel   one thread per (pair, iteration): the draws (mvr_ransac's counter stream), the repeated-index
//                     and edge-length tests on the sample's 2 x ransac_n points (L2-resident: 48 B x n per pair).
//                     About 1 sample in 300 survives them at edge_sim 0.9, so nearly every 256-thread workgroup holds
//                     a survivor and a per-lane fit would run the fp64 Jacobi SVD at 1 / 64 occupancy in most
//                     waves: the survivors are compacted within the workgroup instead (64-bit __ballot + popcount
//                     prefixes -> an LDS list in thread order) and threads 0 .. survivors-1 redo the draws, fit and
//                     apply the distance and normal tests on dense lanes.  The pass flags leave as one 64-bit ballot
//                     word per wave (lane 0 stores it).
//   rc_scan_kernel    one workgroup per pair: popcounts of the words, a prefix sum, and the ordered list of the first
//                     max_validation passing iterations; n_pass, n_valid.
//   ransac_eval_kernel<RansacListed>    one thread per validated hypothesis: re-derives it from its iteration id
//                     (draws + fit, dense), exports it and scores it.  Workgroups beyond n_valid[p] exit at once.
//   ransac_select_kernel<RansacListed>  the best of the validated list (ascending iteration = ascending slot).
// mvr_ransac is the last two alone, as <RansacPlain>: every iteration is a slot of its own.  The two policies hold
// all that the entries differ in there; the draws, the fit, the scoring loop and the order of the selection stand once.
#include "common.hpp"
#include "prof.hpp"
#include "ransac.hpp"
#include "svd3.hpp"
#include <math.h>

namespace mvr {

constexpr int RC_MAXN = 8;     // ransac_n <= 8
constexpr int RC_TILE = 256;

// (the fields stay in this order: with mvr_ransac's fields moved to the front rc_check_kernel, the same instructions
// but for the kernel-argument offsets, measured 2.6 % slower, 5.08 against 4.95 ms — DESIGN.md 4.26)
struct RansacArgs {
  const double* x1; const double* x2; int64_t ps;   // [P][ps] rows of 3 doubles
  const double* nrm1; const double* nrm2;           // both set or both null
  const int32_t* n;                                  // [P] correspondences per pair
  int P, iters, rn, maxv, nwords;
  int bpp, vpp;                                      // 256-thread blocks per pair: check, eval
  double d2, sim2, cd2, ncos;                        // max distance squared; the checkers' thresholds
  uint64_t seed;
  uint64_t* bits;                                    // [P][nwords]
  int32_t* n_pass; int32_t* n_valid;                 // [P]
  int32_t* valid; int32_t* cnt; double* err;         // [P][maxv]; mvr_ransac: cnt, err [P][iters]
  double* hyp;                                       // [P][maxv][12] (R row-major, t); mvr_ransac: [P][iters][12]
};                                                   // mvr_ransac leaves the checkers' fields 0

// What the evaluation and the selection of the two entries differ in: a pair's hypotheses sit in slots
// 0 .. live - 1 of its rows of cnt / err / hyp, `stride` slots apart from the next pair's.
struct RansacPlain {    // mvr_ransac: grid (blocks, pairs); slot = iteration, all of them live
  static __device__ __forceinline__ int pair(const RansacArgs&) { return blockIdx.y; }
  static __device__ __forceinline__ int block(const RansacArgs&) { return blockIdx.x; }
  static __device__ __forceinline__ int live(const RansacArgs& a, int) { return a.iters; }
  static __device__ __forceinline__ int iter(const RansacArgs&, int, int slot) { return slot; }
  static __device__ __forceinline__ int stride(const RansacArgs& a) { return a.iters; }
};
struct RansacListed {   // mvr_ransac_checked: grid pairs x vpp, flattened; slot = index into the validated list
  static __device__ __forceinline__ int pair(const RansacArgs& a) { return blockIdx.x / a.vpp; }
  static __device__ __forceinline__ int block(const RansacArgs& a) { return blockIdx.x % a.vpp; }
  static __device__ __forceinline__ int live(const RansacArgs& a, int p) { return a.n_valid[p]; }
  static __device__ __forceinline__ int iter(const RansacArgs& a, int p, int slot) {
    return a.valid[(int64_t)p * a.maxv + slot];
  }
  static __device__ __forceinline__ int stride(const RansacArgs& a) { return a.maxv; }
};

__device__ __forceinline__ void rc_load(const double* x, const int64_t c[RC_MAXN], int k, double v[RC_MAXN][3]) {
#pragma unroll
  for (int j = 0; j < RC_MAXN; ++j)
#pragma unroll
    for (int e = 0; e < 3; ++e) v[j][e] = j < k ? x[3 * c[j] + e] : 0.0;
}

// Umeyama without scaling on k sample points (unrolled to RC_MAXN and predicated: no array is indexed at run time):
// sigma = sum (dst - mu_d)(src - mu_s)^T / k = U S V^T, R = U diag(1, 1, sign(det U det V)) V^T, t = mu_d - R mu_s
__device__ __forceinline__ void rc_fit(const double s[RC_MAXN][3], const double d[RC_MAXN][3], int k, double R[3][3],
                                       double t[3]) {
#pragma clang fp contract(off)
  double ms[3] = {0, 0, 0}, md[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < RC_MAXN; ++j)
    if (j < k)
      for (int e = 0; e < 3; ++e) {
        ms[e] = ms[e] + s[j][e];
        md[e] = md[e] + d[j][e];
      }
  for (int e = 0; e < 3; ++e) {
    ms[e] = ms[e] / k;
    md[e] = md[e] / k;
  }
  double H[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < RC_MAXN; ++j)
        if (j < k) acc = acc + (d[j][r] - md[r]) * (s[j][c] - ms[c]);
      H[r][c] = acc / k;
    }
  double U[3][3], S[3], V[3][3];
  jacobi_svd3(H, U, S, V);
  const double sg = (det3(U) * det3(V) < 0.0) ? -1.0 : 1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R[r][c] = (U[r][0] * V[c][0] + U[r][1] * V[c][1]) + (sg * U[r][2]) * V[c][2];
  for (int r = 0; r < 3; ++r)
    t[r] = md[r] - ((R[r][0] * ms[0] + R[r][1] * ms[1]) + R[r][2] * ms[2]);
}

// inliers and their error sum of (R, t) over the pair's n rows, in row order: the whole workgroup calls it and stages
// the rows through `tile`
__device__ __forceinline__ void rc_score(const double* x1, const double* x2, int n, const double R[3][3],
                                         const double t[3], double d2, double (*tile)[6], int& good, double& e2) {
#pragma clang fp contract(off)   // hipcc contracts a * b + c into fma by default; the evaluation rounds every op
  int cnt = 0;          // locals: accumulated through the reference parameters, the two-row loop body carried a second
  double err = 0.0;     // copy of the count (86 instructions for 79)
  for (int b0 = 0; b0 < n; b0 += RC_TILE) {
    const int nb = min(RC_TILE, n - b0);
    __syncthreads();
    for (int i = threadIdx.x; i < nb * 6; i += blockDim.x) {
      const int r = i / 6, e = i % 6;
      tile[r][e] = e < 3 ? x1[3 * (int64_t)(b0 + r) + e] : x2[3 * (int64_t)(b0 + r) + e - 3];
    }
    __syncthreads();
    for (int r = 0; r < nb; ++r) {
      const double dd = ransac_row_d2<3, 1>(&R[0][0], t, tile[r], tile[r] + 3);
      if (dd < d2) {
        ++cnt;
        err = err + dd;
      }
    }
  }
  good = cnt;
  e2 = err;
}

__global__ __launch_bounds__(256) void rc_check_kernel(RansacArgs a) {
#pragma clang fp contract(off)   // every comparison is against rounded fp64 ops, as the host restatement's
  __shared__ int s_list[256];
  __shared__ int s_wtot[4];
  __shared__ int s_pass[256];
  const int p = blockIdx.x / a.bpp, blk = blockIdx.x % a.bpp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int it = blk * 256 + tid;
  const int n = a.n[p];
  const int k = a.rn;
  const double* x1 = a.x1 + (int64_t)p * a.ps;
  const double* x2 = a.x2 + (int64_t)p * a.ps;
  const bool edge = a.sim2 > 0.0;
  const bool fitted = a.cd2 > 0.0 || a.nrm1 != nullptr;   // checks that need the hypothesis
  bool ok = it < a.iters && n >= k;
  if (ok && edge) {
    int64_t c[RC_MAXN];
    ransac_draws(a.seed, p, it, n, k, c);
#pragma unroll
    for (int j = 0; j < RC_MAXN; ++j)
#pragma unroll
      for (int l = j + 1; l < RC_MAXN; ++l)
        if (l < k && c[j] == c[l]) ok = false;
    if (ok) {
      double s[RC_MAXN][3], d[RC_MAXN][3];
      rc_load(x1, c, k, s);
      rc_load(x2, c, k, d);
#pragma unroll
      for (int j = 0; j < RC_MAXN; ++j)
#pragma unroll
        for (int l = j + 1; l < RC_MAXN; ++l)
          if (l < k && !ransac_edge_ok(s[j], s[l], d[j], d[l], a.sim2)) ok = false;
    }
  }
  bool pass = ok;
  if (fitted) {   // uniform
    // compact the survivors of this workgroup in thread order: wave ballots, popcount prefixes, an LDS list
    const unsigned long long m = __ballot(ok);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wtot[wave] = __popcll(m);
    s_pass[tid] = 0;
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += s_wtot[w];
      tot += s_wtot[w];
    }
    if (ok) s_list[off + pre] = tid;
    __syncthreads();
    if (tid < tot) {   // dense lanes: survivor tid of the list
      const int lt = s_list[tid];
      int64_t c[RC_MAXN];
      double s[RC_MAXN][3], d[RC_MAXN][3], R[3][3], t[3];
      ransac_draws(a.seed, p, blk * 256 + lt, n, k, c);
      rc_load(x1, c, k, s);
      rc_load(x2, c, k, d);
      rc_fit(s, d, k, R, t);
      bool good = true;
      if (a.cd2 > 0.0) {
#pragma unroll
        for (int j = 0; j < RC_MAXN; ++j)
          // (as one condition, `j < k && !(.. < a.cd2)`, the kernel grew from 5,031 to 6,306 instructions)
          if (j < k) {
            const double dd = ransac_row_d2<3, 1>(&R[0][0], t, s[j], d[j]);
            if (!(dd < a.cd2)) good = false;
          }
      }
      if (a.nrm1) {
        const double* n1 = a.nrm1 + (int64_t)p * a.ps;
        const double* n2 = a.nrm2 + (int64_t)p * a.ps;
#pragma unroll
        for (int j = 0; j < RC_MAXN; ++j)
          if (j < k) {
            const double u0 = n1[3 * c[j]], u1 = n1[3 * c[j] + 1], u2 = n1[3 * c[j] + 2];
            double r[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) r[e] = (R[e][0] * u0 + R[e][1] * u1) + R[e][2] * u2;
            const double dot = (r[0] * n2[3 * c[j]] + r[1] * n2[3 * c[j] + 1]) + r[2] * n2[3 * c[j] + 2];
            if (!(dot >= a.ncos)) good = false;
          }
      }
      s_pass[lt] = good ? 1 : 0;
    }
    __syncthreads();
    pass = s_pass[tid] != 0;
  }
  const unsigned long long word = __ballot(pass);
  const int wi = blk * 4 + wave;
  if (lane == 0 && wi < a.nwords) a.bits[(int64_t)p * a.nwords + wi] = word;
}

// the ordered list of the first maxv passing iterations of each pair, and the counts
__global__ __launch_bounds__(256) void rc_scan_kernel(RansacArgs a) {
  __shared__ int s_sum[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  const uint64_t* bits = a.bits + (int64_t)p * a.nwords;
  const int per = (a.nwords + 255) / 256;
  const int w0 = min(tid * per, a.nwords), w1 = min(w0 + per, a.nwords);
  int mine = 0;
  for (int w = w0; w < w1; ++w) mine += __popcll(bits[w]);
  s_sum[tid] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {   // inclusive prefix sums
    const int v = tid >= o ? s_sum[tid - o] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  const int total = s_sum[255];
  int32_t* valid = a.valid + (int64_t)p * a.maxv;
  int slot = s_sum[tid] - mine;
  for (int w = w0; w < w1 && slot < a.maxv; ++w) {
    uint64_t m = bits[w];
    while (m && slot < a.maxv) {
      valid[slot++] = w * 64 + __builtin_ctzll(m);
      m &= m - 1;
    }
  }
  const int nv = min(total, a.maxv);
  for (int i = nv + tid; i < a.maxv; i += 256) valid[i] = -1;
  if (tid == 0) {
    a.n_pass[p] = total;
    a.n_valid[p] = nv;
  }
}

// one thread per slot: the hypothesis of its iteration, exported and scored
template <typename Policy>
__global__ __launch_bounds__(256) void ransac_eval_kernel(RansacArgs a) {
#pragma clang fp contract(off)   // the evaluation rounds every op
  __shared__ double tile[RC_TILE][6];
  const int p = Policy::pair(a), blk = Policy::block(a);
  const int n = a.n[p];
  const int nlive = n >= a.rn ? Policy::live(a, p) : 0;   // no hypotheses below ransac_n (selection: identity)
  if (blk * 256 >= nlive) return;   // uniform
  const double* x1 = a.x1 + (int64_t)p * a.ps;
  const double* x2 = a.x2 + (int64_t)p * a.ps;
  const int slot = blk * 256 + threadIdx.x;
  const bool live = slot < nlive;
  const int it = Policy::iter(a, p, live ? slot : 0);   // a dead lane redoes slot 0's and writes nothing
  const int64_t at = (int64_t)p * Policy::stride(a) + slot;
  double R[3][3], t[3];
  {
    int64_t c[RC_MAXN];
    double s[RC_MAXN][3], d[RC_MAXN][3];
    ransac_draws(a.seed, p, it, n, a.rn, c);
    rc_load(x1, c, a.rn, s);
    rc_load(x2, c, a.rn, d);
    rc_fit(s, d, a.rn, R, t);
  }
  if (live) {
    double* h = a.hyp + at * 12;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) h[3 * r + c] = R[r][c];
      h[9 + r] = t[r];
    }
  }
  int good;
  double e2;
  rc_score(x1, x2, n, R, t, a.d2, tile, good, e2);
  if (live) {
    a.cnt[at] = good;
    a.err[at] = e2;
  }
}

// best hypothesis per pair: inliers desc, rmse asc, slot (= iteration) asc (= Open3D's strict-improvement loop)
template <typename Policy>
__global__ __launch_bounds__(256) void ransac_select_kernel(RansacArgs a, double* T, double* fitness, double* rmse,
                                                            int32_t* best) {
  __shared__ int bi[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = a.n[p];
  const int nlive = n >= a.rn ? Policy::live(a, p) : 0;
  const int32_t* cnt = a.cnt + (int64_t)p * Policy::stride(a);
  const double* err = a.err + (int64_t)p * Policy::stride(a);
  auto better = [&](int i, int j) {   // slot i strictly before j in the order
    if (j < 0) return i >= 0;
    if (i < 0) return false;
    const int ci = cnt[i], cj = cnt[j];
    if (ci != cj) return ci > cj;
    const double ri = sqrt(err[i] / ci), rj = sqrt(err[j] / cj);
    if (ri != rj) return ri < rj;
    return i < j;
  };
  int mine = -1;
  for (int i = tid; i < nlive; i += blockDim.x)
    if (cnt[i] > 0 && better(i, mine)) mine = i;
  bi[tid] = mine;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w && better(bi[tid + w], bi[tid])) bi[tid] = bi[tid + w];
    __syncthreads();
  }
  if (tid != 0) return;
  const int b = bi[0];
  double* Tp = T + (int64_t)p * 16;
  for (int i = 0; i < 16; ++i) Tp[i] = (i % 5 == 0) ? 1.0 : 0.0;
  if (b < 0) {
    best[p] = -1;
    fitness[p] = 0.0;
    rmse[p] = 0.0;
    return;
  }
  best[p] = Policy::iter(a, p, b);
  fitness[p] = (double)cnt[b] / n;
  rmse[p] = sqrt(err[b] / cnt[b]);
  // the winner's transformation: read back from the hypothesis buffer (always allocated by the launchers)
  const double* h = a.hyp + ((int64_t)p * Policy::stride(a) + b) * 12;
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) Tp[4 * r + cc] = h[3 * r + cc];
    Tp[4 * r + 3] = h[9 + r];
  }
}

static size_t rc_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace mvr

extern "C" size_t mvr_ransac_workspace_bytes(int P, int iters) {
  if (P <= 0 || iters <= 0) return 0;
  return (size_t)P * iters * (sizeof(int32_t) + sizeof(double) + 12 * sizeof(double)) + 256;
}

extern "C" int mvr_ransac(const double* x1, const double* x2, int64_t x_pstride, const int32_t* n, int P, int ransac_n,
                          int iters, double max_dist, uint64_t seed, double* T, double* fitness, double* rmse,
                          int32_t* best_iter, double* hyp_out, void* workspace, size_t workspace_bytes,
                          hipStream_t stream) {
  if (P < 0 || ransac_n < 3 || ransac_n > mvr::RC_MAXN || iters <= 0 || iters >= (1 << 30) || P >= (1 << 23) ||
      !(max_dist > 0.0))
    return MVR_EINVAL;
  if (P == 0) return MVR_OK;
  if (!x1 || !x2 || !n || !T || !fitness || !rmse || !best_iter) return MVR_EINVAL;
  const size_t need = mvr_ransac_workspace_bytes(P, iters) - (hyp_out ? (size_t)P * iters * 12 * sizeof(double) : 0);
  if (!workspace || workspace_bytes < need) return MVR_EINVAL;
  mvr::RansacArgs a{};
  a.x1 = x1; a.x2 = x2; a.ps = x_pstride; a.n = n;
  a.P = P; a.iters = iters; a.rn = ransac_n; a.d2 = max_dist * max_dist; a.seed = seed;
  char* w = static_cast<char*>(workspace);
  a.err = reinterpret_cast<double*>(w);
  a.cnt = reinterpret_cast<int32_t*>(w + (size_t)P * iters * sizeof(double));
  a.hyp = hyp_out
          ? hyp_out
          : reinterpret_cast<double*>(w + mvr::rc_align((size_t)P * iters * (sizeof(double) + sizeof(int32_t))));
  hipLaunchKernelGGL(mvr::ransac_eval_kernel<mvr::RansacPlain>, dim3((iters + 255) / 256, P), dim3(256), 0, stream, a);
  MVR_CHECK_LAUNCH();
  hipLaunchKernelGGL(mvr::ransac_select_kernel<mvr::RansacPlain>, dim3(P), dim3(256), 0, stream, a, T, fitness, rmse,
                     best_iter);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}

// per pair: the pass bits, and per validated hypothesis the iteration id, a count, an error sum and 12 doubles
extern "C" size_t mvr_ransac_checked_workspace_bytes(int P, int iters, int max_validation) {
  if (P <= 0 || iters <= 0 || max_validation <= 0) return 0;
  const size_t nwords = ((size_t)iters + 63) / 64, pv = (size_t)P * (size_t)max_validation;
  return mvr::rc_align((size_t)P * nwords * sizeof(uint64_t)) + mvr::rc_align(pv * sizeof(double)) +
         mvr::rc_align(pv * 12 * sizeof(double)) + mvr::rc_align(pv * sizeof(int32_t)) +
         mvr::rc_align(pv * sizeof(int32_t));
}

extern "C" int mvr_ransac_checked(const double* x1, const double* x2, int64_t x_pstride, const int32_t* n, int P,
                                  int ransac_n, int iters, double max_dist, uint64_t seed, int max_validation,
                                  double edge_sim, double check_dist, const double* nrm1, const double* nrm2,
                                  double normal_cos, double* T, double* fitness, double* rmse, int32_t* best_iter,
                                  int32_t* n_pass, int32_t* n_valid, uint64_t* pass_bits, int32_t* valid_iter,
                                  double* hyp_out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (P < 0 || P >= (1 << 23) || ransac_n < 3 || ransac_n > mvr::RC_MAXN || iters <= 0 || iters >= (1 << 30) ||
      max_validation < 1 || !(max_dist > 0.0) || !isfinite(max_dist) || !(edge_sim >= 0.0 && edge_sim < 1.0) ||
      !(check_dist >= 0.0) || !isfinite(check_dist) || !(normal_cos >= -1.0 && normal_cos <= 1.0))
    return MVR_EINVAL;
  const int bpp = (iters + 255) / 256;
  if ((int64_t)P * bpp >= ((int64_t)1 << 31)) return MVR_EINVAL;
  if (P == 0) return MVR_OK;
  if (!x1 || !x2 || !n || !T || !fitness || !rmse || !best_iter || !n_pass || !n_valid) return MVR_EINVAL;
  if (!workspace || workspace_bytes < mvr_ransac_checked_workspace_bytes(P, iters, max_validation))
    return MVR_EINVAL;
  mvr::RansacArgs a{};
  a.x1 = x1; a.x2 = x2; a.ps = x_pstride; a.n = n;
  const bool normals = nrm1 && nrm2;
  a.nrm1 = normals ? nrm1 : nullptr; a.nrm2 = normals ? nrm2 : nullptr;
  a.P = P; a.iters = iters; a.rn = ransac_n; a.maxv = max_validation; a.nwords = (iters + 63) / 64;
  a.bpp = bpp; a.vpp = ((max_validation < iters ? max_validation : iters) + 255) / 256;
  a.d2 = max_dist * max_dist; a.sim2 = edge_sim * edge_sim; a.cd2 = check_dist * check_dist; a.ncos = normal_cos;
  a.seed = seed;
  const size_t pv = (size_t)P * (size_t)max_validation;
  char* w = static_cast<char*>(workspace);
  a.bits = pass_bits ? pass_bits : reinterpret_cast<uint64_t*>(w);
  w += mvr::rc_align((size_t)P * a.nwords * sizeof(uint64_t));
  a.err = reinterpret_cast<double*>(w);
  w += mvr::rc_align(pv * sizeof(double));
  a.hyp = hyp_out ? hyp_out : reinterpret_cast<double*>(w);
  w += mvr::rc_align(pv * 12 * sizeof(double));
  a.valid = valid_iter ? valid_iter : reinterpret_cast<int32_t*>(w);
  w += mvr::rc_align(pv * sizeof(int32_t));
  a.cnt = reinterpret_cast<int32_t*>(w);
  a.n_pass = n_pass; a.n_valid = n_valid;
  {
    mvr::ProfScope prof(mvr::PK_RANSAC_CHECK, 0.0, 0.0, stream);
    hipLaunchKernelGGL(mvr::rc_check_kernel, dim3(P * bpp), dim3(256), 0, stream, a);
  }
  MVR_CHECK_LAUNCH();
  {
    mvr::ProfScope prof(mvr::PK_RANSAC_SCAN, 0.0, 0.0, stream);
    hipLaunchKernelGGL(mvr::rc_scan_kernel, dim3(P), dim3(256), 0, stream, a);
  }
  MVR_CHECK_LAUNCH();
  {
    mvr::ProfScope prof(mvr::PK_RANSAC_EVAL, 0.0, 0.0, stream);
    hipLaunchKernelGGL(mvr::ransac_eval_kernel<mvr::RansacListed>, dim3(P * a.vpp), dim3(256), 0, stream, a);
  }
  MVR_CHECK_LAUNCH();
  {
    mvr::ProfScope prof(mvr::PK_RANSAC_SELECT, 0.0, 0.0, stream);
    hipLaunchKernelGGL(mvr::ransac_select_kernel<mvr::RansacListed>, dim3(P), dim3(256), 0, stream, a, T, fitness,
                       rmse, best_iter);
  }
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
