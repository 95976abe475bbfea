// Nearest neighbour in feature space between ragged fragments (mvreg.h mvr_feat_match), for any
// channel count up to 64: the matcher of the FPFH descriptors (33 channels), where feat_nn.hip's MFMA kernel
// (C == 32, equal-sized sampled sets) does not apply.
//
// One workgroup per (pair, tile of 512 queries).  A thread keeps TWO query rows in registers, channel by channel as
// the two halves of a float2 (CP channels, C padded with zeros up to a compiled width: a zero channel adds exactly 0
// to every distance), so that the difference and the multiply-add of both queries are one packed fp32 instruction
// each (v_pk_add_f32, v_pk_fma_f32) against the target value in both halves.  The target fragment streams through
// LDS in tiles of kMatchRows rows that every lane reads at the same address (broadcasts, no bank conflicts); two
// queries per thread also halve those reads per distance.
// Distances are plain fp32 differences squared and summed over c ascending, each query its own chain; `<` against
// the running best keeps the smallest row on ties.  Deliberately not MFMA: flat regions give many identical
// descriptors, and the argmin has to be well-defined to fp32.  No atomics; the loop over the target fragment is
// bounded by its size.
#include "common.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

constexpr int kMatchThreads = 256;
constexpr int kMatchQueries = 2 * kMatchThreads;   // per workgroup: thread t takes queries t and t + 256 of the tile
constexpr int kMatchRows = 64;                     // target rows per LDS tile: 64 x 64 floats = 16 KiB at the widest

typedef float v2f __attribute__((ext_vector_type(2)));

template <int CP>
__global__ __launch_bounds__(kMatchThreads) void feat_match_kernel(const float* __restrict__ F, int C,
                                                                   const int64_t* __restrict__ off, int B,
                                                                   const int64_t* __restrict__ pairs,
                                                                   const int64_t* __restrict__ qoff,
                                                                   int32_t* __restrict__ idx,
                                                                   float* __restrict__ dist2) {
  __shared__ float tile[kMatchRows * CP];
  const int p = blockIdx.x;
  const int64_t q0 = qoff[p], nq_out = qoff[p + 1] - q0;
  const int64_t base = (int64_t)blockIdx.y * kMatchQueries;
  if (base >= nq_out) return;   // the whole workgroup: uniform, before any barrier
  const int64_t qa = base + threadIdx.x, qb = qa + kMatchThreads;
  const int64_t fq = pairs[2 * p], ft = pairs[2 * p + 1];
  const bool ok = fq >= 0 && fq < B && ft >= 0 && ft < B;
  const int64_t sb = ok ? off[fq] : 0, nq = ok ? off[fq + 1] - sb : 0;
  const int64_t tb = ok ? off[ft] : 0, nt = ok ? off[ft + 1] - tb : 0;
  const bool live_a = qa < nq && qa < nq_out, live_b = qb < nq && qb < nq_out;
  v2f q[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    q[c].x = (live_a && c < C) ? F[(sb + qa) * C + c] : 0.0f;
    q[c].y = (live_b && c < C) ? F[(sb + qb) * C + c] : 0.0f;
  }
  float best_a = INFINITY, best_b = INFINITY;
  int32_t bi_a = -1, bi_b = -1;
  for (int64_t t0 = 0; t0 < nt; t0 += kMatchRows) {
    const int rows = (int)(nt - t0 < kMatchRows ? nt - t0 : kMatchRows);
    __syncthreads();   // the previous tile has been read by everyone
    for (int e = threadIdx.x; e < rows * CP; e += kMatchThreads) {
      const int row = e / CP, c = e % CP;
      tile[e] = c < C ? F[(tb + t0 + row) * C + c] : 0.0f;
    }
    __syncthreads();
    for (int row = 0; row < rows; ++row) {   // not unrolled: two rows at a time measured 1.5 % slower
      const float* tr = tile + row * CP;
      v2f acc = {0.0f, 0.0f};
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float t = tr[c];
        const v2f d = q[c] - (v2f){t, t};
        acc += d * d;
      }
      const int32_t r = (int32_t)(t0 + row);
      if (acc.x < best_a || bi_a < 0) {   // the first row always: a NaN or infinite distance still names a row
        best_a = acc.x;
        bi_a = r;
      }
      if (acc.y < best_b || bi_b < 0) {
        best_b = acc.y;
        bi_b = r;
      }
    }
  }
  if (qa < nq_out) {
    idx[q0 + qa] = live_a ? bi_a : -1;
    if (dist2) dist2[q0 + qa] = (live_a && bi_a >= 0) ? best_a : INFINITY;
  }
  if (qb < nq_out) {
    idx[q0 + qb] = live_b ? bi_b : -1;
    if (dist2) dist2[q0 + qb] = (live_b && bi_b >= 0) ? best_b : INFINITY;
  }
}

}  // namespace mvr

extern "C" int mvr_feat_match(const float* F, int C, const int64_t* off, int B, int64_t M, const int64_t* pairs,
                              const int64_t* qoff, int P, int64_t n_queries, int64_t max_q, int32_t* idx,
                              float* dist2, hipStream_t stream) {
  if (C < 1 || C > 64 || P < 0 || M < 0 || M > 0x7fffffff || n_queries < 0 || max_q < 0 || max_q > 65535 * 256)
    return MVR_EINVAL;
  if (B <= 0 || B >= (1 << 15)) return MVR_EINVAL;
  if (P == 0 || n_queries == 0) return MVR_OK;   // nothing to match: NULL pointers allowed
  if (!F || !off || !pairs || !qoff || !idx) return MVR_EINVAL;
  if (max_q == 0) return MVR_EINVAL;             // queries but no query fragment
  const dim3 grid((unsigned)P, (unsigned)((max_q + mvr::kMatchQueries - 1) / mvr::kMatchQueries));
  const dim3 block(mvr::kMatchThreads);
  if (C <= 8)
    hipLaunchKernelGGL(mvr::feat_match_kernel<8>, grid, block, 0, stream, F, C, off, B, pairs, qoff, idx, dist2);
  else if (C <= 32)
    hipLaunchKernelGGL(mvr::feat_match_kernel<32>, grid, block, 0, stream, F, C, off, B, pairs, qoff, idx, dist2);
  else if (C <= 36)
    hipLaunchKernelGGL(mvr::feat_match_kernel<36>, grid, block, 0, stream, F, C, off, B, pairs, qoff, idx, dist2);
  else
    hipLaunchKernelGGL(mvr::feat_match_kernel<64>, grid, block, 0, stream, F, C, off, B, pairs, qoff, idx, dist2);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
