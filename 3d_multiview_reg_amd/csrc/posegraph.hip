// Pose-graph refinement over SE(3) with per-edge information matrices, batched over scenes (mvreg.h
// mvr_posegraph_optimize): the last stage of Open3D's multiway registration (global_optimization,
// Levenberg-Marquardt) and of Choi et al. 2015, restated from the maths; tests/posegraph_oracle.py is the normative
// text.  Minimises  c = sum_k w_k xi_k^T L_k xi_k,  xi_k = (v, omega) of D_k = M_j^-1 M_i T_k^-1,  from the poses
// mvr_sync_poses (or anything else) gives, with the anchor held.  mvr_posegraph_optimize_lp (DESIGN.md 4.22a;
// tests/posegraph_lp_oracle.py) is the same kernel with a line process on the uncertain edges.
//
// One 512-thread workgroup per scene, every trial inside the one launch, fp64 throughout, no floating-point or
// global atomics (two flag words in LDS are set by atomicOr: idempotent, so order cannot show).  Per trial:
//   edges    one thread per edge: xi_k, A_k = Ad(M_j^-1), B_k = w A^T L A (6 x 6) and b_k = w A^T L xi into the
//            workspace.  Skipped after a rejected trial: the poses, and with them B and b, have not changed
//   build    M = H + lambda diag H (6N x 6N) and, as row 6N, the gradient g.  Entry (6f + r, 6g + c) of every g is
//            written by the one work-item (f, r, c), which walks the edges in order (their endpoints staged through
//            LDS in chunks): nothing is accumulated atomically, so a scene's bits do not depend on the batch around
//            it.  The anchor and the non-members are identity rows and columns
//   factor   blocked right-looking Cholesky on 6 x 6 blocks, in place, lower triangle: the diagonal block by every
//            thread from broadcast loads, the panel one row per thread, the trailing update one row per wave.  Row
//            6N rides along, so it ends as z = L^-1 g and no forward substitution is needed.  N steps of two barriers.
//            A pivot that is not positive (a NaN is not) fails the trial
//   solve    L^T d = z from the last block up, six block sums per step; delta = -d
//   trial    candidate poses from delta, their cost by a block sum over the edges, accept or reject
// The matrix lives in the workspace (6N x 6N doubles: 1 MB at 60 fragments, 4.7 MB at 128; L2-resident); LDS holds the
// poses, the candidate, delta and the panel.  Every loop is bounded: max_iters, N factor steps, N solve steps.
// Which edges count, the anchor's component and the entries' shared argument rules are scene.hpp's, as sync.hip's
// (DESIGN.md 4.31); the information matrix's test rides in the edge test as its per-edge rule.
#include "scene.hpp"
#include <type_traits>

namespace mvr {

constexpr int kPgThreads = 512;   // 2 waves per SIMD, as sync.hip: every phase is a latency chain
constexpr int kPgF = MVR_SYNC_MAX_FRAGS;
constexpr int kPgN = 6 * kPgF;
constexpr int kPgChunk = 256;     // edges' endpoints staged per LDS chunk

struct PgArgs {
  const double* Rp; const double* tp; const int32_t* ij; const double* w; const double* info; int64_t es;
  const int32_t* n_edges; const int32_t* n_frags;
  int max_frags, max_edges, anchor;
  const double* R0; const double* t0;
  int max_iters; double lambda0, tol_cost, tol_step;
  double* R; double* t; int64_t fs;
  int32_t* member; double* cost; int32_t* iters; int32_t* status; double* trace;
  double* ws; int64_t ws_stride;   // doubles per scene: w [max_edges], B b [42 max_edges], matrix [(6F + 1) 6F]
};

// mvr_posegraph_optimize_lp's: the workspace then ends with l [max_edges] and r [max_edges] per scene
struct PgLpArgs : PgArgs {
  const int32_t* unc; double mu_scale;
  double* line; double* mu;
};

// omega = log(R) as a rotation vector: a = vee(R - R^T) / 2 has |a| = sin(theta), (tr R - 1) / 2 = cos(theta)
__device__ static void so3_log(const double* R, double* om) {
  const double a0 = 0.5 * (R[7] - R[5]), a1 = 0.5 * (R[2] - R[6]), a2 = 0.5 * (R[3] - R[1]);
  const double s = sqrt(a0 * a0 + a1 * a1 + a2 * a2), c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double th = atan2(s, c);
  const double f = s > 1e-8 ? th / s : 1.0 + th * th / 6.0;
  om[0] = f * a0; om[1] = f * a1; om[2] = f * a2;
}

// E = Exp(omega) (Rodrigues), row-major
__device__ static void so3_exp(const double* om, double* E) {
  const double x = om[0], y = om[1], z = om[2];
  const double t2 = x * x + y * y + z * z, th = sqrt(t2);
  const double A = th > 1e-8 ? sin(th) / th : 1.0 - t2 / 6.0;
  const double B = th > 1e-8 ? (1.0 - cos(th)) / t2 : 0.5 - t2 / 24.0;
  E[0] = 1.0 - B * (y * y + z * z); E[1] = -A * z + B * x * y;       E[2] = A * y + B * x * z;
  E[3] = A * z + B * x * y;         E[4] = 1.0 - B * (x * x + z * z); E[5] = -A * x + B * y * z;
  E[6] = -A * y + B * x * z;        E[7] = A * x + B * y * z;         E[8] = 1.0 - B * (x * x + y * y);
}

// xi = (v, omega) of D = M_j^-1 M_i T_k^-1
__device__ static void pg_residual(const double* Ri, const double* ti, const double* Rj, const double* tj,
                                   const double* Rk, const double* tk, double* xi) {
  double P[9], D[9], u[3], s[3];
  for (int r = 0; r < 3; ++r)      // P = R_i R_k^T
    for (int c = 0; c < 3; ++c) P[3 * r + c] = Ri[3 * r] * Rk[3 * c] + Ri[3 * r + 1] * Rk[3 * c + 1] + Ri[3 * r + 2] * Rk[3 * c + 2];
  for (int r = 0; r < 3; ++r)      // D = R_j^T P
    for (int c = 0; c < 3; ++c) D[3 * r + c] = Rj[r] * P[c] + Rj[3 + r] * P[3 + c] + Rj[6 + r] * P[6 + c];
  for (int r = 0; r < 3; ++r)      // s = t_i - P t_k - t_j
    s[r] = ti[r] - (P[3 * r] * tk[0] + P[3 * r + 1] * tk[1] + P[3 * r + 2] * tk[2]) - tj[r];
  for (int r = 0; r < 3; ++r) u[r] = Rj[r] * s[0] + Rj[3 + r] * s[1] + Rj[6 + r] * s[2];
  xi[0] = u[0]; xi[1] = u[1]; xi[2] = u[2];
  so3_log(D, xi + 3);
}

// L [36] <- (info + info^T) / 2 of edge e
__device__ static void pg_lambda(const double* info, double* L) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) L[6 * r + c] = 0.5 * (info[6 * r + c] + info[6 * c + r]);
}

__device__ static double pg_quad(const double* L, const double* xi) {
  double acc = 0.0;
  for (int r = 0; r < 6; ++r) {
    double row = 0.0;
    for (int c = 0; c < 6; ++c) row += L[6 * r + c] * xi[c];
    acc += xi[r] * row;
  }
  return acc;
}

// the lower Cholesky factor of the 6 x 6 block at A (leading dimension n), read through loads every thread shares;
// false on a pivot that is not positive
__device__ static bool chol6(const double* A, int n, double (&L)[21]) {
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      double s = A[(int64_t)r * n + c];
#pragma unroll
      for (int q = 0; q < c; ++q) s -= L[r * (r + 1) / 2 + q] * L[c * (c + 1) / 2 + q];
      if (c == r) {
        ok = ok && s > 0.0;
        L[r * (r + 1) / 2 + r] = sqrt(s);
      } else {
        L[r * (r + 1) / 2 + c] = s / L[c * (c + 1) / 2 + c];
      }
    }
  return ok;
}

// kLineProcess (mvr_posegraph_optimize_lp; tests/posegraph_lp_oracle.py): the counted uncertain edges carry a weight
// l_k = (mu / (mu + r_k))^2, r_k = w_k xi_k^T L_k xi_k, held through a trial and recomputed in closed form after an
// accepted one from the r_k the candidate's cost pass left in the workspace.  Thread e % 512 owns edge e in every
// per-edge pass, so l and r need no barrier of their own.  The held cost is (sum_certain r + sum_uncertain l r) + pen,
// pen = mu sum_uncertain (s - 1)^2: without an uncertain edge the last two are 0.0 and the first is the plain
// kernel's sum, term for term
template <bool kLineProcess>
__global__ __launch_bounds__(kPgThreads) void posegraph_kernel(
    std::conditional_t<kLineProcess, PgLpArgs, PgArgs> a) {
  __shared__ double sP[6][kPgN + 1];            // the factor's current panel, by column
  __shared__ double sD[kPgN];                   // delta
  __shared__ double sR[kPgF][9], sT[kPgF][3];   // the poses
  __shared__ double cR[kPgF][9], cT[kPgF][3];   // the candidate
  __shared__ double red[6 * (kPgThreads / 64)];
  __shared__ int sI[kPgChunk], sJ[kPgChunk];
  __shared__ int sMem[kPgF];
  __shared__ int sFlag[2];

  const int s = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const int N = a.n_frags[s], E = a.n_edges[s];
  const int anchor = a.anchor;
  const double* Rp = a.Rp + (int64_t)s * a.es * 9;
  const double* tp = a.tp + (int64_t)s * a.es * 3;
  const int32_t* ij = a.ij + (int64_t)s * a.es * 2;
  const double* win = a.w ? a.w + (int64_t)s * a.es : nullptr;
  const double* info = a.info + (int64_t)s * a.es * 36;
  const double* R0 = a.R0 + (int64_t)s * a.fs * 9;
  const double* t0 = a.t0 + (int64_t)s * a.fs * 3;
  double* Ro = a.R + (int64_t)s * a.fs * 9;
  double* to = a.t + (int64_t)s * a.fs * 3;
  int32_t* memo = a.member ? a.member + (int64_t)s * a.fs : nullptr;
  const int64_t rows = (int64_t)a.max_iters + 1;
  double* trace = a.trace ? a.trace + (int64_t)s * rows : nullptr;
  double* wc = a.ws + (int64_t)s * a.ws_stride;   // the weight that counts: 0 for an ignored edge
  double* Bb = wc + a.max_edges;                  // per edge B [36], b [6]
  double* M = Bb + 42 * (int64_t)a.max_edges;
  double* lw = M + (6 * (int64_t)a.max_frags + 1) * 6 * (int64_t)a.max_frags;   // kLineProcess: l per edge
  double* rk = lw + a.max_edges;                                               // kLineProcess: r per uncertain edge

  // ---- an invalid scene: poses copied through
  if (tid == 0) sFlag[0] = 0;
  __syncthreads();
  const bool counts_ok = N >= 0 && N <= a.max_frags && E >= 0 && E <= a.max_edges;
  const int nf = min(max(N, 0), a.max_frags);
  {
    int bad = 0;
    for (int e = tid; e < 12 * nf; e += kPgThreads) {
      const int f = e / 12, q = e % 12;
      bad |= !isfinite(q < 9 ? R0[9 * f + q] : t0[3 * f + q - 9]);
    }
    if (bad) atomicOr(&sFlag[0], 1);
  }
  __syncthreads();
  if (!counts_ok || N == 0 || anchor >= N || sFlag[0]) {   // uniform
    const bool bad = !(counts_ok && N == 0 && E == 0);
    for (int f = tid; f < nf; f += kPgThreads) {
      for (int q = 0; q < 9; ++q) Ro[9 * f + q] = R0[9 * f + q];
      for (int q = 0; q < 3; ++q) to[3 * f + q] = t0[3 * f + q];
      if (memo) memo[f] = 0;
    }
    if (trace)
      for (int64_t e = tid; e < rows; e += kPgThreads) trace[e] = -1.0;
    if constexpr (kLineProcess) {
      for (int e = tid; e < min(max(E, 0), a.max_edges); e += kPgThreads) a.line[(int64_t)s * a.es + e] = 0.0;
      if (tid == 0 && a.mu) a.mu[s] = 0.0;
    }
    if (tid == 0) {
      a.cost[2 * s] = 0.0;
      a.cost[2 * s + 1] = 0.0;
      a.iters[s] = 0;
      a.status[s] = bad ? (4 | (nf > 0 ? 1 : 0)) : 0;
    }
    return;
  }
  const int n = 6 * N;
  __syncthreads();   // sFlag[0] read by everyone before it is reused

  // ---- the edges that count, the members (scene.hpp); the edge's own rule: info finite, symmetric to 1e-9 |L|_F
  for (int f = tid; f < N; f += kPgThreads) {
    sMem[f] = (f == anchor);
    for (int q = 0; q < 9; ++q) sR[f][q] = R0[9 * f + q];
    for (int q = 0; q < 3; ++q) sT[f][q] = t0[3 * f + q];
  }
  __syncthreads();
  scene_edge_test<kPgThreads>(Rp, tp, ij, win, N, E, wc, sFlag, [&](int e) {
    const double* Le = info + (int64_t)36 * e;
    bool ok = true;
    double fro = 0.0, asym = 0.0;
    for (int q = 0; q < 36; ++q) {
      ok = ok && isfinite(Le[q]);
      fro += Le[q] * Le[q];
      asym = fmax(asym, fabs(Le[q] - Le[6 * (q % 6) + q / 6]));
    }
    return ok && !(asym > 1e-9 * sqrt(fro));
  });
  const int Nm = scene_component<kPgThreads>(ij, N, E, wc, sMem, sFlag);
  int status = sFlag[0] | (Nm < N ? 1 : 0);
  for (int e = tid; e < E; e += kPgThreads) wc[e] = fmax(wc[e], 0.0);   // in place: 0 for an ignored edge
  __syncthreads();

  // c = sum_k w_k xi_k^T L_k xi_k at the poses (PR, PT), in every thread
  auto cost_of = [&](const double (*PR)[9], const double (*PT)[3]) {
    double acc[1] = {0.0};
    for (int e = tid; e < E; e += kPgThreads) {
      const double wgt = wc[e];
      if (wgt > 0.0) {
        const int i = ij[2 * e], j = ij[2 * e + 1];
        double xi[6], L[36];
        pg_residual(PR[i], PT[i], PR[j], PT[j], Rp + (int64_t)9 * e, tp + (int64_t)3 * e, xi);
        pg_lambda(info + (int64_t)36 * e, L);
        acc[0] += wgt * pg_quad(L, xi);
      }
    }
    block_sum<1>(acc, red);
    return acc[0];
  };

  // ---- the line process: mu, then l in closed form at the initial poses
  double mu = 0.0, pen = 0.0;
  bool lp_on = false;
  const int32_t* unc = nullptr;
  if constexpr (kLineProcess) {
    unc = a.unc ? a.unc + (int64_t)s * a.es : nullptr;
    double acc[2] = {0.0, 0.0};
    for (int e = tid; e < E; e += kPgThreads) {
      lw[e] = 1.0;
      if (wc[e] > 0.0 && (!unc || unc[e] != 0)) {
        acc[0] += info[(int64_t)36 * e];
        acc[1] += 1.0;
      }
    }
    block_sum<2>(acc, red);
    if (acc[1] > 0.0) {
      mu = a.mu_scale * (acc[0] / acc[1]);
      lp_on = mu > 0.0 && isfinite(mu);
      if (!lp_on) status |= 16;
    }
  }
  // (sum over the certain edges of r, over the uncertain ones of l r with the l held) at the poses (PR, PT), in every
  // thread; r of every uncertain edge is left in rk
  auto cost_lp = [&](const double (*PR)[9], const double (*PT)[3], double (&acc)[2]) {
    acc[0] = 0.0;
    acc[1] = 0.0;
    for (int e = tid; e < E; e += kPgThreads) {
      const double wgt = wc[e];
      if (wgt > 0.0) {
        const int i = ij[2 * e], j = ij[2 * e + 1];
        double xi[6], L[36];
        pg_residual(PR[i], PT[i], PR[j], PT[j], Rp + (int64_t)9 * e, tp + (int64_t)3 * e, xi);
        pg_lambda(info + (int64_t)36 * e, L);
        const double q = pg_quad(L, xi);
        if (lp_on && (!unc || unc[e] != 0)) {
          const double r = wgt * q;
          rk[e] = r;
          acc[1] += lw[e] * r;
        } else {
          acc[0] += wgt * q;
        }
      }
    }
    block_sum<2>(acc, red);
  };
  // l <- (mu / (mu + r))^2 from rk; -> (sum_uncertain l r, sum_uncertain (s - 1)^2) in every thread
  auto lp_update = [&](double (&acc)[2]) {
    acc[0] = 0.0;
    acc[1] = 0.0;
    for (int e = tid; e < E; e += kPgThreads)
      if (wc[e] > 0.0 && (!unc || unc[e] != 0)) {
        const double r = rk[e], sk = mu / (mu + r), l = sk * sk;
        lw[e] = l;
        acc[0] += l * r;
        acc[1] += (sk - 1.0) * (sk - 1.0);
      }
    block_sum<2>(acc, red);
  };

  double c;
  if constexpr (kLineProcess) {
    double sums[2], upd[2] = {0.0, 0.0};
    cost_lp(sR, sT, sums);       // l is 1 still: the second sum is formed and dropped
    if (lp_on) lp_update(upd);   // uniform
    pen = mu * upd[1];
    c = (sums[0] + upd[0]) + pen;
  } else {
    c = cost_of(sR, sT);
  }
  const double c_init = c;
  if (trace && tid == 0) trace[0] = c;
  double lam = a.lambda0;
  int k = 0;
  bool converged = c == 0.0, fresh = true, failed = false;

  while (!converged && k < a.max_iters) {
    // ---- per edge: B = w A^T L A, b = w A^T L xi
    if (fresh)
      for (int e = tid; e < E; e += kPgThreads) {
        const double wgt = wc[e];
        if (!(wgt > 0.0)) continue;
        double wl = wgt;
        if constexpr (kLineProcess) wl = wgt * lw[e];
        const int i = ij[2 * e], j = ij[2 * e + 1];
        const double* Rj = sR[j];
        const double* tj = sT[j];
        double xi[6], L[36], A[36];
        pg_residual(sR[i], sT[i], Rj, tj, Rp + (int64_t)9 * e, tp + (int64_t)3 * e, xi);
        pg_lambda(info + (int64_t)36 * e, L);
        // A = [[R_j^T, -R_j^T [t_j]x], [0, R_j^T]]
        const double X[9] = {0.0, -tj[2], tj[1], tj[2], 0.0, -tj[0], -tj[1], tj[0], 0.0};
        for (int r = 0; r < 3; ++r)
          for (int cc = 0; cc < 3; ++cc) {
            const double rt = Rj[3 * cc + r];
            A[6 * r + cc] = rt;
            A[6 * (r + 3) + cc + 3] = rt;
            A[6 * (r + 3) + cc] = 0.0;
            A[6 * r + cc + 3] = -(Rj[r] * X[cc] + Rj[3 + r] * X[3 + cc] + Rj[6 + r] * X[6 + cc]);
          }
        double* out = Bb + 42 * (int64_t)e;
        double Lx[6];
        for (int r = 0; r < 6; ++r) {
          double acc = 0.0;
          for (int q = 0; q < 6; ++q) acc += L[6 * r + q] * xi[q];
          Lx[r] = acc;
        }
        for (int cc = 0; cc < 6; ++cc) {
          double u[6];   // L A[:, cc]
          for (int r = 0; r < 6; ++r) {
            double acc = 0.0;
            for (int q = 0; q < 6; ++q) acc += L[6 * r + q] * A[6 * q + cc];
            u[r] = acc;
          }
          for (int r = 0; r < 6; ++r) {
            double acc = 0.0;
            for (int q = 0; q < 6; ++q) acc += A[6 * q + r] * u[q];
            out[6 * r + cc] = wl * acc;
          }
          double acc = 0.0;
          for (int q = 0; q < 6; ++q) acc += A[6 * q + cc] * Lx[q];
          out[36 + cc] = wl * acc;
        }
      }
    __syncthreads();

    // ---- M = H + lambda diag H, row n = g.  Work-item (f, r, c) owns the entries (6f + r, 6g + c) of every g
    for (int it0 = 0; it0 < 36 * N; it0 += kPgThreads) {
      const int it = it0 + tid;
      const bool live = it < 36 * N;
      const int f = live ? it / 36 : 0, r = (it % 36) / 6, cc = it % 6;
      const bool solved = live && sMem[f] && f != anchor;
      double* row = M + (int64_t)(6 * f + r) * n + cc;
      if (live)
        for (int g = 0; g < N; ++g) row[6 * g] = 0.0;
      double dg = 0.0, gr = 0.0;
      for (int c0 = 0; c0 < E; c0 += kPgChunk) {
        const int cnt = min(kPgChunk, E - c0);
        __syncthreads();
        for (int q = tid; q < cnt; q += kPgThreads) {
          const bool on = wc[c0 + q] > 0.0;
          sI[q] = on ? ij[2 * (c0 + q)] : -1;
          sJ[q] = on ? ij[2 * (c0 + q) + 1] : -1;
        }
        __syncthreads();
        if (solved)
          for (int q = 0; q < cnt; ++q) {
            const int i = sI[q], j = sJ[q];
            if (i != f && j != f) continue;
            const double* be = Bb + 42 * (int64_t)(c0 + q);
            const double bv = be[6 * r + cc];
            const int other = (i == f) ? j : i;
            dg += bv;
            if (other != anchor) row[6 * other] -= bv;   // members only: the other end of a counted edge is one
            if (cc == 0) gr += (i == f) ? be[36 + r] : -be[36 + r];
          }
      }
      if (live) {
        row[6 * f] = solved ? (r == cc ? dg * (1.0 + lam) : dg) : (r == cc ? 1.0 : 0.0);
        if (cc == 0) M[(int64_t)n * n + 6 * f + r] = solved ? gr : 0.0;
      }
    }
    __syncthreads();

    // ---- factor, rows 0 .. n (row n: g -> z)
    failed = false;
    for (int k0 = 0; k0 < n; k0 += 6) {
      double L[21];
      const bool ok = chol6(M + (int64_t)k0 * (n + 1), n, L);   // the same loads in every thread: uniform
      if (!ok) { failed = true; break; }
      for (int i = k0 + 6 + tid; i <= n; i += kPgThreads) {   // x L^T = A[i, K]
        double* row = M + (int64_t)i * n + k0;
        double x[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          double sacc = row[q];
#pragma unroll
          for (int p = 0; p < q; ++p) sacc -= x[p] * L[q * (q + 1) / 2 + p];
          x[q] = sacc / L[q * (q + 1) / 2 + q];
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) { row[q] = x[q]; sP[q][i] = x[q]; }
      }
      __syncthreads();   // the panel is in LDS; every read of the diagonal block is done
      if (tid == 0) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int q = 0; q <= r; ++q) M[(int64_t)(k0 + r) * n + k0 + q] = L[r * (r + 1) / 2 + q];
      }
      for (int i = k0 + 6 + wv; i <= n; i += kPgThreads / 64) {
        const double p0 = sP[0][i], p1 = sP[1][i], p2 = sP[2][i], p3 = sP[3][i], p4 = sP[4][i], p5 = sP[5][i];
        double* row = M + (int64_t)i * n;
        const int jend = min(i, n - 1);
        for (int j = k0 + 6 + ln; j <= jend; j += 64)
          row[j] -= p0 * sP[0][j] + p1 * sP[1][j] + p2 * sP[2][j] + p3 * sP[3][j] + p4 * sP[4][j] + p5 * sP[5][j];
      }
      __syncthreads();
    }
    ++k;
    double cn = c, step = 0.0;
    bool accepted = false;
    if (failed) {
      lam *= 10.0;
      fresh = false;
      __syncthreads();
    } else {
      // ---- L^T delta = -z, last block first
      for (int k0 = n - 6; k0 >= 0; k0 -= 6) {
        double sacc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = k0 + 6 + tid; i < n; i += kPgThreads) {
          const double di = sD[i];
          const double* row = M + (int64_t)i * n + k0;
#pragma unroll
          for (int q = 0; q < 6; ++q) sacc[q] += row[q] * di;
        }
        block_sum<6>(sacc, red);
        if (tid == 0) {
          const double* Lk = M + (int64_t)k0 * (n + 1);
          const double* z = M + (int64_t)n * n + k0;
          double d[6];
          for (int q = 5; q >= 0; --q) {
            double v = -z[q] - sacc[q];
            for (int p = q + 1; p < 6; ++p) v -= Lk[(int64_t)p * n + q] * d[p];
            d[q] = v / Lk[(int64_t)q * n + q];
            sD[k0 + q] = d[q];
          }
        }
        __syncthreads();
      }
      // ---- the candidate and its cost
      double mx = 0.0;
      for (int f = tid; f < N; f += kPgThreads) {
        double Ex[9];
        const double* d = sD + 6 * f;
        so3_exp(d + 3, Ex);
        for (int r = 0; r < 3; ++r) {
          for (int cc = 0; cc < 3; ++cc)
            cR[f][3 * r + cc] = Ex[3 * r] * sR[f][cc] + Ex[3 * r + 1] * sR[f][3 + cc] + Ex[3 * r + 2] * sR[f][6 + cc];
          cT[f][r] = Ex[3 * r] * sT[f][0] + Ex[3 * r + 1] * sT[f][1] + Ex[3 * r + 2] * sT[f][2] + d[r];
        }
        for (int q = 0; q < 6; ++q) mx = fmax(mx, fabs(d[q]));
      }
      step = block_max<kPgThreads / 64>(mx, red);   // its barriers order the candidate's writes before the reads below
      double sums[2];
      if constexpr (kLineProcess) {
        cost_lp(cR, cT, sums);
        cn = (sums[0] + sums[1]) + pen;
      } else {
        cn = cost_of(cR, cT);
      }
      accepted = cn < c;
      if (accepted) {
        for (int e = tid; e < 12 * N; e += kPgThreads) {
          const int f = e / 12, q = e % 12;
          if (q < 9) sR[f][q] = cR[f][q]; else sT[f][q - 9] = cT[f][q - 9];
        }
        if constexpr (kLineProcess) {
          if (lp_on) {   // uniform: l in closed form at the accepted poses, c'' <= c'
            double upd[2];
            lp_update(upd);
            pen = mu * upd[1];
            cn = (sums[0] + upd[0]) + pen;
          }
        }
        if (c - cn <= a.tol_cost * c) converged = true;
        c = cn;
        lam /= 10.0;
      } else {
        lam *= 10.0;
      }
      fresh = accepted;
      if (step <= a.tol_step) converged = true;
      if (c == 0.0) converged = true;
      __syncthreads();
    }
    if (trace && tid == 0) trace[k] = c;
  }
  if (!converged && k == a.max_iters && (a.tol_cost > 0.0 || a.tol_step > 0.0)) status |= 2;
  if (failed) status |= 8;

  for (int f = tid; f < N; f += kPgThreads) {
    for (int q = 0; q < 9; ++q) Ro[9 * f + q] = sR[f][q];
    for (int q = 0; q < 3; ++q) to[3 * f + q] = sT[f][q];
    if (memo) memo[f] = sMem[f];
  }
  if (trace)
    for (int64_t e = (int64_t)k + 1 + tid; e < rows; e += kPgThreads) trace[e] = -1.0;
  if constexpr (kLineProcess) {
    for (int e = tid; e < E; e += kPgThreads) a.line[(int64_t)s * a.es + e] = wc[e] > 0.0 ? lw[e] : 0.0;
    if (tid == 0 && a.mu) a.mu[s] = mu;
  }
  if (tid == 0) {
    a.cost[2 * s] = c_init;
    a.cost[2 * s + 1] = c;
    a.iters[s] = k;
    a.status[s] = status;
  }
}

}  // namespace mvr

extern "C" size_t mvr_posegraph_workspace_bytes(int S, int max_frags, int max_edges) {
  if (S <= 0 || max_frags < 0 || max_edges < 0) return 0;
  return (size_t)S * (43 * (size_t)max_edges + (6 * (size_t)max_frags + 1) * 6 * (size_t)max_frags) * sizeof(double);
}

extern "C" size_t mvr_posegraph_lp_workspace_bytes(int S, int max_frags, int max_edges) {
  if (S <= 0 || max_frags < 0 || max_edges < 0) return 0;
  return mvr_posegraph_workspace_bytes(S, max_frags, max_edges) + (size_t)S * 2 * (size_t)max_edges * sizeof(double);
}

// the argument rules both entries share, then the arguments; -> MVR_OK with *launch false when there is nothing to do
static int pg_arguments(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w,
                        const double* info, int64_t e_sstride, const int32_t* n_edges, const int32_t* n_frags, int S,
                        int max_frags, int max_edges, int anchor, const double* R0, const double* t0, int max_iters,
                        double lambda0, double tol_cost, double tol_step, double* R, double* t, int64_t f_sstride,
                        int32_t* member, double* cost, int32_t* iters, int32_t* status, double* trace, void* workspace,
                        size_t workspace_bytes, size_t need, int64_t extra, mvr::PgArgs& a, bool* launch) {
  *launch = false;
  if (!mvr::scene_counts_ok(S, max_frags, max_edges, anchor) || max_iters < 0) return MVR_EINVAL;
  if (!(lambda0 >= 0.0) || !isfinite(lambda0) || !(tol_cost >= 0.0) || !(tol_step >= 0.0)) return MVR_EINVAL;
  if (S == 0 || max_frags == 0) return MVR_OK;   // nothing to write: NULL pointers allowed
  if (!n_edges || !n_frags || !status || !cost || !iters || !R || !t || !R0 || !t0) return MVR_EINVAL;
  if (max_edges > 0 && (!R_pair || !t_pair || !ij || !info)) return MVR_EINVAL;
  if (!mvr::scene_buffers_ok(S, max_frags, max_edges, e_sstride, f_sstride, workspace, workspace_bytes, need))
    return MVR_EINVAL;
  a.Rp = R_pair; a.tp = t_pair; a.ij = ij; a.w = w; a.info = info; a.es = e_sstride;
  a.n_edges = n_edges; a.n_frags = n_frags;
  a.max_frags = max_frags; a.max_edges = max_edges; a.anchor = anchor;
  a.R0 = R0; a.t0 = t0;
  a.max_iters = max_iters; a.lambda0 = lambda0; a.tol_cost = tol_cost; a.tol_step = tol_step;
  a.R = R; a.t = t; a.fs = f_sstride;
  a.member = member; a.cost = cost; a.iters = iters; a.status = status; a.trace = trace;
  a.ws = static_cast<double*>(workspace);
  a.ws_stride = 43 * (int64_t)max_edges + (6 * (int64_t)max_frags + 1) * 6 * (int64_t)max_frags + extra;
  *launch = true;
  return MVR_OK;
}

extern "C" int mvr_posegraph_optimize(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w,
                                      const double* info, int64_t e_sstride, const int32_t* n_edges,
                                      const int32_t* n_frags, int S, int max_frags, int max_edges, int anchor,
                                      const double* R0, const double* t0, int max_iters, double lambda0,
                                      double tol_cost, double tol_step, double* R, double* t, int64_t f_sstride,
                                      int32_t* member, double* cost, int32_t* iters, int32_t* status, double* trace,
                                      void* workspace, size_t workspace_bytes, hipStream_t stream) {
  mvr::PgArgs a{};
  bool launch;
  const int rc = pg_arguments(R_pair, t_pair, ij, w, info, e_sstride, n_edges, n_frags, S, max_frags, max_edges, anchor,
                              R0, t0, max_iters, lambda0, tol_cost, tol_step, R, t, f_sstride, member, cost, iters,
                              status, trace, workspace, workspace_bytes,
                              mvr_posegraph_workspace_bytes(S, max_frags, max_edges), 0, a, &launch);
  if (rc != MVR_OK || !launch) return rc;
  hipLaunchKernelGGL(mvr::posegraph_kernel<false>, dim3(S), dim3(mvr::kPgThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}

extern "C" int mvr_posegraph_optimize_lp(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w,
                                         const double* info, const int32_t* uncertain, int64_t e_sstride,
                                         const int32_t* n_edges, const int32_t* n_frags, int S, int max_frags,
                                         int max_edges, int anchor, const double* R0, const double* t0, int max_iters,
                                         double lambda0, double tol_cost, double tol_step, double mu_scale, double* R,
                                         double* t, int64_t f_sstride, int32_t* member, double* cost, int32_t* iters,
                                         int32_t* status, double* trace, double* line, double* mu, void* workspace,
                                         size_t workspace_bytes, hipStream_t stream) {
  if (!(mu_scale > 0.0) || !isfinite(mu_scale)) return MVR_EINVAL;
  mvr::PgLpArgs a{};
  bool launch;
  const int rc = pg_arguments(R_pair, t_pair, ij, w, info, e_sstride, n_edges, n_frags, S, max_frags, max_edges, anchor,
                              R0, t0, max_iters, lambda0, tol_cost, tol_step, R, t, f_sstride, member, cost, iters,
                              status, trace, workspace, workspace_bytes,
                              mvr_posegraph_lp_workspace_bytes(S, max_frags, max_edges), 2 * (int64_t)max_edges, a,
                              &launch);
  if (rc != MVR_OK || !launch) return rc;
  if (max_edges > 0 && !line) return MVR_EINVAL;  a.unc = uncertain; a.mu_scale = mu_scale; a.line = line; a.mu = mu;
  hipLaunchKernelGGL(mvr::posegraph_kernel<true>, dim3(S), dim3(mvr::kPgThreads), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
