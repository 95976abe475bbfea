// Multiview pose synchronisation: one pose per fragment from a scene's pairwise estimates (mvreg.h mvr_sync_poses;
// DESIGN.md 4.18).  The closed-form weighted solve of the paper's sections 3.2-3.3 — the bottom
// three eigenvectors of the 3N x 3N rotation Laplacian, then an SPD solve for the translations — wrapped in IRLS.
// The reference never released this stage (its README.md:116); tests/sync_oracle.py restates the closed form.
//
// One 512-thread workgroup per scene, every IRLS pass inside the one launch, fp64 throughout.  Per pass:
//   build    L + sigma I from the edge list, staged through LDS in chunks of 128 edges; entry (3f + r, 3g + c) is
//            written by the one work-item (f, r, c), which walks the edges in order: no atomics, so a scene's bits do
//            not depend on the batch around it
//   invert   in place by Gauss-Jordan on 3 x 3 blocks (SPD: no pivoting), N steps of two barriers
//   iterate  Q <- orth(M Q) on three vectors (inverse subspace iteration): one mat-vec, two block reductions and a
//            3 x 3 Cholesky per step, until |M Q - Q (Q^T M Q)|_F <= 1e-13 |M Q|_F (ratio (l3 + sigma) / (l4 + sigma)
//            per step; status bit 2 at the cap).  The gauge-fixed rotations depend on span(Q) only, so no Ritz step
//   project  each fragment's 3 x 3 block onto SO(3) (jacobi_svd3), gauge to the anchor
//   solve    the grounded graph Laplacian (N x N, in the matrix's storage) inverted the same way, t = A^-1 b
//   weigh    per-edge residuals and the next pass's weights
// The matrix lives in LDS up to kSyncLdsFrags fragments (3N <= 126: 124 KiB) and in the workspace (L2) above that;
// the code is the same, the launcher picks the instantiation from max_frags.
// Which edges count, the anchor's component and the entry's shared argument rules are scene.hpp's, as posegraph.hip's
// (DESIGN.md 4.31); w0 (the base weight of every IRLS pass) and w (the pass's) stay apart here.
#include "scene.hpp"
#include "svd3.hpp"

namespace mvr {

constexpr int kSyncThreads = 512;   // 2 waves per SIMD: every phase is a latency chain, a second wave overlaps it
constexpr int kSyncChunk = 128;     // edges staged per LDS chunk
constexpr int kSyncLdsFrags = 42;   // largest max_frags whose matrix stays in LDS
constexpr int kSyncCap = 500;       // subspace-iteration cap per pass
constexpr double kSyncTol = 1e-13;

struct SyncArgs {
  const double* Rp; const double* tp; const int32_t* ij; const double* w; int64_t es;
  const int32_t* n_edges; const int32_t* n_frags;
  int max_frags, max_edges, anchor, iters;
  double c_rot, c_trans;
  double* R; double* t; int64_t fs;
  int32_t* member; double* w_out; double* res_rot; double* res_trans; int32_t* status;
  double* ws; int64_t ws_stride;   // doubles per scene: w0 [max_edges], w [max_edges], matrix [9 max_frags^2]
};

// A <- A^-1 in place, A symmetric positive definite n x n (row-major, ld n), n a multiple of 3: Gauss-Jordan on
// 3 x 3 blocks without pivoting, n / 3 steps of two barriers.  Step k with K = {3k, 3k+1, 3k+2}, P = A[K,K]^-1,
// C = A[:,K], W = A[K,:]:  A[i,j] -= (C P)[i,:] W[:,j] off the pivot, A[K,j] = P W[:,j], A[i,K] = -(C P)[i,:],
// A[K,K] = P.  A wave takes every eighth row, a lane the columns ln, ln + 64, ..; W's columns stay in registers
// and the next row is loaded before this one is stored, so the rows' load -> fma -> store chains overlap.
// sC / sW: [3][kN] doubles of LDS each.
template <int kN>
__device__ static void gj_invert3(double* A, int n, double (*sC)[kN], double (*sW)[kN]) {
  constexpr int J = (kN + 63) / 64, kRows = kSyncThreads / 64;
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  for (int k0 = 0; k0 < n; k0 += 3) {
    for (int i = tid; i < n; i += kSyncThreads)
      for (int q = 0; q < 3; ++q) {
        sC[q][i] = A[(int64_t)i * n + k0 + q];
        sW[q][i] = A[(int64_t)(k0 + q) * n + i];
      }
    __syncthreads();
    // P: the symmetric pivot block's inverse by its adjugate (every thread, from LDS broadcasts)
    const double m00 = sW[0][k0], m01 = sW[0][k0 + 1], m02 = sW[0][k0 + 2];
    const double m11 = sW[1][k0 + 1], m12 = sW[1][k0 + 2], m22 = sW[2][k0 + 2];
    const double a00 = m11 * m22 - m12 * m12, a01 = m02 * m12 - m01 * m22, a02 = m01 * m12 - m02 * m11;
    const double a11 = m00 * m22 - m02 * m02, a12 = m01 * m02 - m00 * m12, a22 = m00 * m11 - m01 * m01;
    const double idet = 1.0 / (m00 * a00 + m01 * a01 + m02 * a02);
    const double p00 = a00 * idet, p01 = a01 * idet, p02 = a02 * idet;
    const double p11 = a11 * idet, p12 = a12 * idet, p22 = a22 * idet;
    // a lane's columns: W's entries, with unit vectors at the pivot columns and `keep` = 0 there, so that one
    // expression  keep * A[i,j] - (d0 w0 + d1 w1 + d2 w2)  covers all four cases: d = (C P)[i,:] off the pivot
    // rows, and d = -P[i - k0,:] with keep = 0 on them
    double w0[J], w1[J], w2[J], cur[J], nxt[J];
    bool keep[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      const int j = ln + 64 * jj, jb = j - k0;
      const bool in = j < n, pc = jb >= 0 && jb < 3;
      keep[jj] = !pc;
      w0[jj] = pc ? (jb == 0 ? 1.0 : 0.0) : (in ? sW[0][j] : 0.0);
      w1[jj] = pc ? (jb == 1 ? 1.0 : 0.0) : (in ? sW[1][j] : 0.0);
      w2[jj] = pc ? (jb == 2 ? 1.0 : 0.0) : (in ? sW[2][j] : 0.0);
      cur[jj] = (in && wv < n) ? A[(int64_t)wv * n + j] : 0.0;
    }
    for (int i = wv; i < n; i += kRows) {
      double* row = A + (int64_t)i * n;
      const int inext = i + kRows;
#pragma unroll
      for (int jj = 0; jj < J; ++jj) {
        const int j = ln + 64 * jj;
        nxt[jj] = (j < n && inext < n) ? A[(int64_t)inext * n + j] : 0.0;
      }
      const int ib = i - k0;   // wave-uniform
      const bool prow = ib >= 0 && ib < 3;
      const double c0 = sC[0][i], c1 = sC[1][i], c2 = sC[2][i];
      double d0 = c0 * p00 + c1 * p01 + c2 * p02;
      double d1 = c0 * p01 + c1 * p11 + c2 * p12;
      double d2 = c0 * p02 + c1 * p12 + c2 * p22;
      if (prow) {
        d0 = -(ib == 0 ? p00 : (ib == 1 ? p01 : p02));
        d1 = -(ib == 0 ? p01 : (ib == 1 ? p11 : p12));
        d2 = -(ib == 0 ? p02 : (ib == 1 ? p12 : p22));
      }
#pragma unroll
      for (int jj = 0; jj < J; ++jj) {
        const int j = ln + 64 * jj;
        const double base = (keep[jj] && !prow) ? cur[jj] : 0.0;
        if (j < n) row[j] = base - (d0 * w0[jj] + d1 * w1[jj] + d2 * w2[jj]);
        cur[jj] = nxt[jj];
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double sync_start_value(int idx) {   // splitmix64 -> [-1, 1): a generic start block
  uint64_t z = ((uint64_t)idx + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// -DMVR_SYNC_STAMPS (tools/sync_micro.py --stamps, a variant build): scene 0 writes wall_clock64() (100 MHz) at
// the phase boundaries of its first pass into the workspace's 256 spare bytes, slot 31 = that pass's iterations
#ifdef MVR_SYNC_STAMPS
#define MVR_SYNC_STAMP(k) \
  if (tid == 0 && s == 0 && pass == 0) reinterpret_cast<uint64_t*>(a.ws + (int64_t)gridDim.x * a.ws_stride)[k] = wall_clock64()
#else
#define MVR_SYNC_STAMP(k)
#endif

template <int kF, bool kLds>
__global__ __launch_bounds__(kSyncThreads) void sync_kernel(SyncArgs a) {
  constexpr int kN = 3 * kF;
  __shared__ double sM[kLds ? kN * kN : 1];
  __shared__ double sX[3][kN], sY[3][kN];
  __shared__ double sP[kF][9], sR[kF][9], sT[kF][3], sB[kF][3];
  __shared__ double sGc[3][kN], sGw[3][kN];   // gj_invert3's pivot columns and rows
  __shared__ double red[15 * (kSyncThreads / 64)];
  __shared__ double sW[kSyncChunk], sRk[kSyncChunk * 9], sTk[kSyncChunk * 3];
  __shared__ int sI[kSyncChunk], sJ[kSyncChunk];
  __shared__ int sMem[kF];
  __shared__ int sFlag[2];

  const int s = blockIdx.x, tid = threadIdx.x;
  const int N = a.n_frags[s], E = a.n_edges[s];
  const int anchor = a.anchor;
  const double* Rp = a.Rp + (int64_t)s * a.es * 9;
  const double* tp = a.tp + (int64_t)s * a.es * 3;
  const int32_t* ij = a.ij + (int64_t)s * a.es * 2;
  const double* win = a.w ? a.w + (int64_t)s * a.es : nullptr;
  double* Ro = a.R + (int64_t)s * a.fs * 9;
  double* to = a.t + (int64_t)s * a.fs * 3;
  int32_t* memo = a.member ? a.member + (int64_t)s * a.fs : nullptr;
  double* wo = a.w_out ? a.w_out + (int64_t)s * a.es : nullptr;
  double* ero = a.res_rot ? a.res_rot + (int64_t)s * a.es : nullptr;
  double* eto = a.res_trans ? a.res_trans + (int64_t)s * a.es : nullptr;
  double* w0 = a.ws + (int64_t)s * a.ws_stride;
  double* wc = w0 + a.max_edges;
  double* M = kLds ? sM : wc + a.max_edges;

  // the scene as identity: every fragment R = I, t = 0, every edge weight and residuals 0
  auto identity_scene = [&](int nf, int ne, int mem, int st) {
    for (int f = tid; f < nf; f += kSyncThreads) {
      for (int q = 0; q < 9; ++q) Ro[9 * f + q] = (q % 4 == 0) ? 1.0 : 0.0;
      for (int q = 0; q < 3; ++q) to[3 * f + q] = 0.0;
      if (memo) memo[f] = mem;
    }
    for (int e = tid; e < ne; e += kSyncThreads) {
      if (wo) wo[e] = 0.0;
      if (ero) ero[e] = 0.0;
      if (eto) eto[e] = 0.0;
    }
    if (tid == 0) a.status[s] = st;
  };

  {
    const bool bad = N < 0 || N > a.max_frags || E < 0 || E > a.max_edges || (N > 0 && anchor >= N) ||
                     (N == 0 && E > 0);
    if (bad || N == 0) {   // uniform
      const int nf = min(max(N, 0), a.max_frags), ne = min(max(E, 0), a.max_edges);
      identity_scene(nf, ne, 0, bad ? (4 | (nf > 0 ? 1 : 0)) : 0);
      return;
    }
  }
  const int n = 3 * N;

  // ---- the edges that count (scene.hpp): w0 = the weight, -1 for an ignored edge
  if (tid == 0) sFlag[0] = 0;
  for (int f = tid; f < N; f += kSyncThreads) sMem[f] = (f == anchor);
  __syncthreads();
  scene_edge_test<kSyncThreads>(Rp, tp, ij, win, N, E, w0, sFlag, [](int) { return true; });
  if (N == 1) {   // uniform
    identity_scene(1, E, 1, sFlag[0]);
    return;
  }

  // ---- members: the anchor's component.  w0 stays the base of every IRLS pass, wc is the pass's weight
  const int Nm = scene_component<kSyncThreads>(ij, N, E, w0, sMem, sFlag);
  int status = sFlag[0] | (Nm < N ? 1 : 0);
  for (int e = tid; e < E; e += kSyncThreads) wc[e] = fmax(w0[e], 0.0);
  __syncthreads();

  // stage edges [c0, c0 + cnt) for the builders: endpoints (-1: contributes nothing), weights, R_k and t_k
  auto stage = [&](int c0, int cnt) {
    for (int q = tid; q < cnt; q += kSyncThreads) {
      const int e = c0 + q;
      const double wv = wc[e];
      sW[q] = wv;
      sI[q] = wv > 0.0 ? ij[2 * e] : -1;
      sJ[q] = wv > 0.0 ? ij[2 * e + 1] : -1;
    }
    for (int q = tid; q < 9 * cnt; q += kSyncThreads) sRk[q] = Rp[(int64_t)9 * c0 + q];
    for (int q = tid; q < 3 * cnt; q += kSyncThreads) sTk[q] = tp[(int64_t)3 * c0 + q];
  };
  // Q = Y C^-T with G = Y^T Y = C C^T (Cholesky QR of the three columns)
  auto orthonormalize = [&](const double* G) {   // G: g00 g10 g11 g20 g21 g22
    const double c00 = sqrt(G[0]), c10 = G[1] / c00, c11 = sqrt(G[2] - c10 * c10);
    const double c20 = G[3] / c00, c21 = (G[4] - c20 * c10) / c11, c22 = sqrt(G[5] - c20 * c20 - c21 * c21);
    for (int i = tid; i < n; i += kSyncThreads) {
      const double q0 = sY[0][i] / c00;
      const double q1 = (sY[1][i] - c10 * q0) / c11;
      const double q2 = (sY[2][i] - c20 * q0 - c21 * q1) / c22;
      sX[0][i] = q0; sX[1][i] = q1; sX[2][i] = q2;
    }
    __syncthreads();
  };

  for (int pass = 0; pass <= a.iters; ++pass) {
    // ---- L + sigma I
    MVR_SYNC_STAMP(0);
    double sw[1] = {0.0};
    for (int e = tid; e < E; e += kSyncThreads) sw[0] += wc[e];
    block_sum<1>(sw, red);
    const double sigma = sw[0] > 0.0 ? 1e-3 * (2.0 * sw[0] / Nm) : 1e-3;
    const double pad = fmax(1.0, 2.0 * sw[0]);
    for (int i = tid >> 6; i < n; i += kSyncThreads / 64) {
      const double dg = sigma + (sMem[i / 3] ? 0.0 : pad);
      for (int j = tid & 63; j < n; j += 64) M[(int64_t)i * n + j] = (i == j) ? dg : 0.0;
    }
    __syncthreads();
    // work-item (f, r, c) = tid + rr * 512 owns the entries (3f + r, 3g + c) of every g: consecutive items share a
    // fragment, so a wave's 64 items cover 8 fragments and most edges of a chunk touch none of them
    constexpr int kItems = (9 * kF + kSyncThreads - 1) / kSyncThreads;
    double dg[kItems];
#pragma unroll
    for (int rr = 0; rr < kItems; ++rr) dg[rr] = 0.0;
    for (int c0 = 0; c0 < E; c0 += kSyncChunk) {
      const int cnt = min(kSyncChunk, E - c0);
      stage(c0, cnt);
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < kItems; ++rr) {
        const int it = tid + rr * kSyncThreads;
        if (it < 9 * N) {
          const int f = it / 9, r = (it % 9) / 3, c = it % 3;
          double* row = M + (int64_t)(3 * f + r) * n + c;
          for (int q = 0; q < cnt; ++q) {
            const int i = sI[q], j = sJ[q];
            if (i == f) {          // block (i, j) -= w R_k^T
              row[3 * j] -= sW[q] * sRk[9 * q + 3 * c + r];
              dg[rr] += sW[q];
            } else if (j == f) {   // block (j, i) -= w R_k
              row[3 * i] -= sW[q] * sRk[9 * q + 3 * r + c];
              dg[rr] += sW[q];
            }
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int rr = 0; rr < kItems; ++rr) {
      const int it = tid + rr * kSyncThreads;
      if (it < 9 * N && (it % 9) / 3 == it % 3) M[(int64_t)(3 * (it / 9) + it % 3) * (n + 1)] += dg[rr];
    }
    __syncthreads();
    MVR_SYNC_STAMP(1);
    gj_invert3<kN>(M, n, sGc, sGw);
    MVR_SYNC_STAMP(2);

    // ---- the dominant three-dimensional invariant subspace of M = (L + sigma I)^-1
    {
      double g[6] = {0, 0, 0, 0, 0, 0};
      for (int i = tid; i < n; i += kSyncThreads) {
        double y[3];
        for (int c = 0; c < 3; ++c) {
          y[c] = sMem[i / 3] ? sync_start_value(3 * i + c) : 0.0;
          sY[c][i] = y[c];
        }
        g[0] += y[0] * y[0]; g[1] += y[1] * y[0]; g[2] += y[1] * y[1];
        g[3] += y[2] * y[0]; g[4] += y[2] * y[1]; g[5] += y[2] * y[2];
      }
      block_sum<6>(g, red);
      orthonormalize(g);
    }
    bool converged = false;
    int steps = 0;
    for (; steps < kSyncCap && !converged; ++steps) {
      double v[15];
#pragma unroll
      for (int q = 0; q < 15; ++q) v[q] = 0.0;
      for (int i0 = 0; i0 < n; i0 += kSyncThreads / 4) {   // 4 adjacent lanes per row, each a quarter of the j's
        const int i = i0 + (tid >> 2);
        double y0 = 0.0, y1 = 0.0, y2 = 0.0;
        if (i < n)
          for (int j = tid & 3; j < n; j += 4) {   // M symmetric: column i read as M[j][i]
            const double m = M[(int64_t)j * n + i];
            y0 += m * sX[0][j]; y1 += m * sX[1][j]; y2 += m * sX[2][j];
          }
        y0 += __shfl_xor(y0, 1, 64); y1 += __shfl_xor(y1, 1, 64); y2 += __shfl_xor(y2, 1, 64);
        y0 += __shfl_xor(y0, 2, 64); y1 += __shfl_xor(y1, 2, 64); y2 += __shfl_xor(y2, 2, 64);
        if (i >= n || (tid & 3)) continue;
        sY[0][i] = y0; sY[1][i] = y1; sY[2][i] = y2;
        const double x0 = sX[0][i], x1 = sX[1][i], x2 = sX[2][i];
        v[0] += x0 * y0; v[1] += x0 * y1; v[2] += x0 * y2;     // H = Q^T Y, row-major
        v[3] += x1 * y0; v[4] += x1 * y1; v[5] += x1 * y2;
        v[6] += x2 * y0; v[7] += x2 * y1; v[8] += x2 * y2;
        v[9] += y0 * y0; v[10] += y1 * y0; v[11] += y1 * y1;   // G = Y^T Y
        v[12] += y2 * y0; v[13] += y2 * y1; v[14] += y2 * y2;
      }
      block_sum<15>(v, red);   // its barriers also order the sY writes before the reads below
      double rs[1] = {0.0};
      for (int i = tid; i < n; i += kSyncThreads) {
        const double x0 = sX[0][i], x1 = sX[1][i], x2 = sX[2][i];
        const double r0 = sY[0][i] - (x0 * v[0] + x1 * v[3] + x2 * v[6]);
        const double r1 = sY[1][i] - (x0 * v[1] + x1 * v[4] + x2 * v[7]);
        const double r2 = sY[2][i] - (x0 * v[2] + x1 * v[5] + x2 * v[8]);
        rs[0] += r0 * r0 + r1 * r1 + r2 * r2;
      }
      block_sum<1>(rs, red);
      converged = rs[0] <= kSyncTol * kSyncTol * (v[9] + v[11] + v[14]);   // uniform: block_sum's result
      orthonormalize(v + 9);
    }
    if (!converged) status |= 2;
    MVR_SYNC_STAMP(3);
#ifdef MVR_SYNC_STAMPS
    if (tid == 0 && s == 0 && pass == 0) reinterpret_cast<uint64_t*>(a.ws + (int64_t)gridDim.x * a.ws_stride)[31] = steps;
#endif

    // ---- rotations: U_f = Q's block f; the members' det signs fix U's handedness; P_f = proj(U_f); R_f = P_a P_f^T
    {
      double sg[1] = {0.0};
      double U[3][3];
      // fragment f on lane f / 8 of wave f % 8: a wave's fragments are few, so its edge scans below skip most edges
      const int f = (tid & 63) < 17 ? (tid & 63) * (kSyncThreads / 64) + (tid >> 6) : kN;   // covers [0, 136) >= Np
      if (f < N && sMem[f]) {
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) U[r][c] = sX[c][3 * f + r];
        const double d = det3(U);
        sg[0] = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
      }
      block_sum<1>(sg, red);
      if (f < N && sMem[f]) {
        if (sg[0] < 0.0)
          for (int r = 0; r < 3; ++r) U[r][2] = -U[r][2];
        double A[3][3], S[3], B[3][3];
        jacobi_svd3(U, A, S, B);
        const double d = det3(A) * det3(B) < 0.0 ? -1.0 : 1.0;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) sP[f][3 * r + c] = A[r][0] * B[c][0] + A[r][1] * B[c][1] + d * A[r][2] * B[c][2];
      }
      __syncthreads();
      if (f < N) {
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            double v = (r == c) ? 1.0 : 0.0;
            if (sMem[f] && f != anchor)
              v = sP[anchor][3 * r] * sP[f][3 * c] + sP[anchor][3 * r + 1] * sP[f][3 * c + 1] +
                  sP[anchor][3 * r + 2] * sP[f][3 * c + 2];
            sR[f][3 * r + c] = v;
          }
      }
      // ---- translations: the grounded Laplacian A (the anchor, the non-members and the rows that pad N to a
      // multiple of 3 as identity rows), b, t = A^-1 b
      double* A = M;
      const int Np = 3 * ((N + 2) / 3);
      for (int e = tid; e < Np * Np; e += kSyncThreads) A[e] = 0.0;
      __syncthreads();
      double bacc[3] = {0.0, 0.0, 0.0}, diag = 0.0;
      const bool solved = f < N && sMem[f] && f != anchor;
      for (int c0 = 0; c0 < E; c0 += kSyncChunk) {
        const int cnt = min(kSyncChunk, E - c0);
        stage(c0, cnt);
        __syncthreads();
        if (solved)
          for (int q = 0; q < cnt; ++q) {
            const int i = sI[q], j = sJ[q];
            if (i != f && j != f) continue;
            const double wv = sW[q];
            const double* tk = sTk + 3 * q;
            const double* Rj = sR[j];
            const double sgn = (i == f) ? wv : -wv;   // b_i += w R_j t_k, b_j -= w R_j t_k
            for (int r = 0; r < 3; ++r) bacc[r] += sgn * (Rj[3 * r] * tk[0] + Rj[3 * r + 1] * tk[1] + Rj[3 * r + 2] * tk[2]);
            diag += wv;
            const int other = (i == f) ? j : i;
            if (other != anchor) A[(int64_t)f * Np + other] -= wv;
          }
        __syncthreads();
      }
      if (f < Np) A[(int64_t)f * Np + f] = solved ? diag : 1.0;
      if (f < N)
        for (int r = 0; r < 3; ++r) sB[f][r] = bacc[r];
      __syncthreads();
      MVR_SYNC_STAMP(4);
      gj_invert3<kN>(A, Np, sGc, sGw);
      MVR_SYNC_STAMP(5);
      if (f < N) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        if (solved)
          for (int g = 0; g < N; ++g) {
            const double m = A[(int64_t)g * Np + f];
            t0 += m * sB[g][0]; t1 += m * sB[g][1]; t2 += m * sB[g][2];
          }
        sT[f][0] = t0; sT[f][1] = t1; sT[f][2] = t2;
      }
      __syncthreads();
    }

    // ---- residuals, and the next pass's weights or the outputs
    MVR_SYNC_STAMP(6);
    const bool last = pass == a.iters;
    for (int e = tid; e < E; e += kSyncThreads) {
      double er = 0.0, et = 0.0, wn = 0.0;
      const double wbase = w0[e];
      if (wbase >= 0.0) {
        const int i = ij[2 * e], j = ij[2 * e + 1];
        const double* Ri = sR[i];
        const double* Rj = sR[j];
        const double* Rk = Rp + (int64_t)9 * e;
        const double* tk = tp + (int64_t)3 * e;
        double acc = 0.0;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            const double d = Rk[3 * r + c] - (Rj[r] * Ri[c] + Rj[3 + r] * Ri[3 + c] + Rj[6 + r] * Ri[6 + c]);
            acc += d * d;
          }
        er = sqrt(acc);
        acc = 0.0;
        for (int r = 0; r < 3; ++r) {
          const double d = sT[i][r] - sT[j][r] - (Rj[3 * r] * tk[0] + Rj[3 * r + 1] * tk[1] + Rj[3 * r + 2] * tk[2]);
          acc += d * d;
        }
        et = sqrt(acc);
        if (last) {
          wn = wc[e];
        } else {
          const double qr = er / a.c_rot, qt = et / a.c_trans;
          wn = wbase / (1.0 + qr * qr) / (1.0 + qt * qt);
        }
      }
      if (last) {
        if (wo) wo[e] = wn;
        if (ero) ero[e] = er;
        if (eto) eto[e] = et;
      } else {
        wc[e] = wn;
      }
    }
    __syncthreads();
    MVR_SYNC_STAMP(7);
  }

  for (int f = tid; f < N; f += kSyncThreads) {
    for (int q = 0; q < 9; ++q) Ro[9 * f + q] = sR[f][q];
    for (int q = 0; q < 3; ++q) to[3 * f + q] = sT[f][q];
    if (memo) memo[f] = sMem[f];
  }
  if (tid == 0) a.status[s] = status;
}

}  // namespace mvr

extern "C" size_t mvr_sync_workspace_bytes(int S, int max_frags, int max_edges) {
  if (S <= 0 || max_frags < 0 || max_edges < 0) return 0;
  return (size_t)S * (2 * (size_t)max_edges + 9 * (size_t)max_frags * max_frags) * sizeof(double) + 256;
}

extern "C" int mvr_sync_poses(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w,
                              int64_t e_sstride, const int32_t* n_edges, const int32_t* n_frags, int S, int max_frags,
                              int max_edges, int anchor, int irls_iters, double c_rot, double c_trans, double* R,
                              double* t, int64_t f_sstride, int32_t* member, double* w_out, double* res_rot,
                              double* res_trans, int32_t* status, void* workspace, size_t workspace_bytes,
                              hipStream_t stream) {
  if (!mvr::scene_counts_ok(S, max_frags, max_edges, anchor) || irls_iters < 0) return MVR_EINVAL;
  if (irls_iters > 0 && !(c_rot > 0.0 && c_trans > 0.0)) return MVR_EINVAL;
  if (S == 0) return MVR_OK;
  if (!n_edges || !n_frags || !status) return MVR_EINVAL;
  if (max_frags > 0 && (!R || !t)) return MVR_EINVAL;
  if (max_edges > 0 && (!R_pair || !t_pair || !ij)) return MVR_EINVAL;
  if (!mvr::scene_buffers_ok(S, max_frags, max_edges, e_sstride, f_sstride, workspace, workspace_bytes,
                             mvr_sync_workspace_bytes(S, max_frags, max_edges)))
    return MVR_EINVAL;
  mvr::SyncArgs a{};
  a.Rp = R_pair; a.tp = t_pair; a.ij = ij; a.w = w; a.es = e_sstride;
  a.n_edges = n_edges; a.n_frags = n_frags;
  a.max_frags = max_frags; a.max_edges = max_edges; a.anchor = anchor; a.iters = irls_iters;
  a.c_rot = c_rot; a.c_trans = c_trans;
  a.R = R; a.t = t; a.fs = f_sstride;
  a.member = member; a.w_out = w_out; a.res_rot = res_rot; a.res_trans = res_trans; a.status = status;
  a.ws = static_cast<double*>(workspace);
  a.ws_stride = 2 * (int64_t)max_edges + 9 * (int64_t)max_frags * max_frags;
  if (max_frags <= mvr::kSyncLdsFrags)
    hipLaunchKernelGGL((mvr::sync_kernel<mvr::kSyncLdsFrags, true>), dim3(S), dim3(mvr::kSyncThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((mvr::sync_kernel<MVR_SYNC_MAX_FRAGS, false>), dim3(S), dim3(mvr::kSyncThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
