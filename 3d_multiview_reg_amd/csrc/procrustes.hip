// Batched weighted Procrustes (Kabsch) + residuals.
//
// Replaces lib/utils.py:164-256 (kabsch_transformation_estimation +
// transformation_residuals) and the batch-coupled zero-weight guard of
// lib/filtering/oanet.py:177-178.
//
// One 256-thread workgroup per pair.  The reference materialises an N x N
// diag_embed(w) and runs torch.svd; here a single pass accumulates the 16
// weighted first/second moments in fp64 (wave shuffles + one LDS round),
// one lane solves the 3x3 SVD by one-sided Jacobi in fp64, and a second pass
// (L2-resident re-read) writes the fp32 residuals.
//
// Origin of the moments.  The centred covariance comes out of raw moments, so for a cloud of spread 1 at
// distance c from the origin every term is ~c^2 while the result is ~1: fp64 moments about the origin lose
// 2 log10(c) digits (measured on an MI355X, fp64, 257 points, worst |R - R_oracle| of four pairs: 1.0e-12 at
// c = 1e2, 3.1e-11 at 1e3, 4.7e-9 at 1e4), and a covariance that is itself tiny against the moments — one point,
// where H = W (eps / (W + eps))^2 x1 x2^T — comes out as rounding noise in either precision (tr(R H) short of the
// optimum by 1.7e-5 s0 in fp64, 9.4e-5 s0 in fp32).  Both instantiations therefore accumulate about the pair's first point,
// o1 = x1[0], o2 = x2[0] (one address for the whole workgroup), as icp.hip does.  With x' = x - o, sums S' over
// the shifted points and the reference's means mu = S / (W + eps) (utils.py:203-204 — NOT S / W):
//   a = mu1 - o1 = (S1' + W o1) / (W + eps) - o1 = (S1' - eps o1) / (W + eps),   b = mu2 - o2 likewise,
//   H = sum w (x1 - mu1)(x2 - mu2)^T = sum w (x1' - a)(x2' - b)^T = S12' - a S2'^T - S1' b^T + W a b^T,
//   t = mu2 - R mu1 = (b + o2) - R (a + o1).
// Every term is now of the size of the cloud's extent about its first point (the same fp64 clouds: 3.3e-15,
// 8.9e-16, 6.1e-16).  The first point counts as origin whatever its weight: it has to lie with the cloud.
//
// HBM bytes per pair (algorithmic): N*(24 read xyz pairs + 4 read w + 4 write res)
// (+4+4 when the guard rewrites w and its copy).
#include "common.hpp"
#include "prof.hpp"
#include "svd3.hpp"
#include <math.h>

namespace mvr {

template <typename T>
struct ProcrustesArgs {
  const T* x1; const T* x2; int64_t x_ps, x_ns;
  T* w; int64_t w_ps;
  const int32_t* guard_pos; T* w_copy; int64_t wc_ps;
  int P, N, normalize; T eps;
  int guard_group;   // pairs [g*G, (g+1)*G) share the guard; 0 = the whole batch
  T* R; T* t; T* res; int64_t res_ps;
  T* res_copy; int64_t rc_ps;
  int32_t* status;
};

// T = float (the fp32 OANet path) or double (fp64 inputs, as torch would compute them).
template <typename T>
__global__ __launch_bounds__(256) void procrustes_kernel(ProcrustesArgs<T> a) {
  __shared__ double red[16 * 4];
  __shared__ T sRt[12];
  __shared__ int sflag;
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  const T* x1 = a.x1 + (int64_t)p * a.x_ps;
  const T* x2 = a.x2 + (int64_t)p * a.x_ps;
  T* w = a.w ? a.w + (int64_t)p * a.w_ps : nullptr;

  // ---- zero-weight guard (oanet.py:177-178): any pair of the batch (or of this pair's guard
  // group, see ProcrustesArgs::guard_group) with sum(w)==0
  if (tid == 0) sflag = 0;
  __syncthreads();
  if (a.guard_pos) {
    const int q0 = a.guard_group > 0 ? (p / a.guard_group) * a.guard_group : 0;
    const int q1 = a.guard_group > 0 ? min(q0 + a.guard_group, a.P) : a.P;
    int any = 0;
    for (int q = q0 + tid; q < q1; q += blockDim.x) any |= (a.guard_pos[q] == 0);
    if (any) atomicOr(&sflag, 1);
  }
  __syncthreads();
  const bool guard = sflag != 0;
  const T addw = (T)1 / (T)a.N;

  // ---- origin of the moments (header comment): the pair's first point
  double o1[3] = {0.0, 0.0, 0.0}, o2[3] = {0.0, 0.0, 0.0};
  if (a.N > 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { o1[i] = x1[i]; o2[i] = x2[i]; }
  }

  // ---- moments of the shifted points: W, S1[3], S2[3], S12[3][3]
  double m[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = 0.0;
  for (int n = tid; n < a.N; n += blockDim.x) {
    T wi = w ? w[n] : (T)1;
    if (guard) {
      wi = wi + addw;
      w[n] = wi;
      if (a.w_copy) a.w_copy[(int64_t)p * a.wc_ps + n] = wi;
    }
    const T* p1 = x1 + (int64_t)n * a.x_ns;
    const T* p2 = x2 + (int64_t)n * a.x_ns;
    const double wd = wi;
    const double u0 = p1[0] - o1[0], u1 = p1[1] - o1[1], u2 = p1[2] - o1[2];
    const double v0 = p2[0] - o2[0], v1 = p2[1] - o2[1], v2 = p2[2] - o2[2];
    m[0] += wd;
    m[1] += wd * u0; m[2] += wd * u1; m[3] += wd * u2;
    m[4] += wd * v0; m[5] += wd * v1; m[6] += wd * v2;
    m[7] += wd * u0 * v0; m[8] += wd * u0 * v1; m[9] += wd * u0 * v2;
    m[10] += wd * u1 * v0; m[11] += wd * u1 * v1; m[12] += wd * u1 * v2;
    m[13] += wd * u2 * v0; m[14] += wd * u2 * v1; m[15] += wd * u2 * v2;
  }
  block_sum<16>(m, red);

  if (tid == 0) {
    // normalisation (utils.py:187-189): w <- w / (sum(w) + eps)
    double scale = 1.0;
    if (a.normalize) scale = 1.0 / ((double)((T)m[0] + a.eps));
    const double W = m[0] * scale;
    const double den = W + (double)a.eps;  // utils.py:203-204
    double mu1[3], mu2[3], S1[3], S2[3];   // mu: the means relative to the origin (a, b of the header comment)
    for (int i = 0; i < 3; ++i) {
      S1[i] = m[1 + i] * scale; S2[i] = m[4 + i] * scale;
      mu1[i] = (S1[i] - (double)a.eps * o1[i]) / den; mu2[i] = (S2[i] - (double)a.eps * o2[i]) / den;
    }
    double H[3][3];
    bool finite = true;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        // sum w (x1'-mu1)(x2'-mu2)^T = S12 - mu1 S2^T - S1 mu2^T + W mu1 mu2^T
        H[i][j] = m[7 + 3 * i + j] * scale - mu1[i] * S2[j] - S1[i] * mu2[j] + W * mu1[i] * mu2[j];
        finite = finite && isfinite(H[i][j]);
      }
    double R[3][3], t[3];
    int st = 0;
    if (!finite) {  // torch.svd raised -> R = I, t = 0, flag (utils.py:216-223)
      st = 1;
      for (int i = 0; i < 3; ++i) { t[i] = 0.0; for (int j = 0; j < 3; ++j) R[i][j] = (i == j); }
    } else {
      double U[3][3], S[3], V[3][3];
      jacobi_svd3(H, U, S, V);
      double VUt[3][3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) VUt[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + V[i][2] * U[j][2];
      const double d = det3(VUt) < 0 ? -1.0 : 1.0;  // utils.py:225-227
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + d * V[i][2] * U[j][2];
      for (int i = 0; i < 3; ++i) { mu1[i] += o1[i]; mu2[i] += o2[i]; }
      for (int i = 0; i < 3; ++i) t[i] = mu2[i] - (R[i][0] * mu1[0] + R[i][1] * mu1[1] + R[i][2] * mu1[2]);
    }
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) {
        sRt[3 * i + j] = (T)R[i][j];
        a.R[(int64_t)p * 9 + 3 * i + j] = (T)R[i][j];
      }
      sRt[9 + i] = (T)t[i];
      a.t[(int64_t)p * 3 + i] = (T)t[i];
    }
    if (a.status) a.status[p] = st;
  }
  __syncthreads();
  if (!a.res) return;
  T r[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) r[i] = sRt[i];
  for (int n = tid; n < a.N; n += blockDim.x) {
    const T* p1 = x1 + (int64_t)n * a.x_ns;
    const T* p2 = x2 + (int64_t)n * a.x_ns;
    const T u0 = p1[0], u1 = p1[1], u2 = p1[2];
    const T d0 = fma(r[0], u0, fma(r[1], u1, r[2] * u2)) + r[9] - p2[0];
    const T d1 = fma(r[3], u0, fma(r[4], u1, r[5] * u2)) + r[10] - p2[1];
    const T d2 = fma(r[6], u0, fma(r[7], u1, r[8] * u2)) + r[11] - p2[2];
    const T rv = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    a.res[(int64_t)p * a.res_ps + n] = rv;
    if (a.res_copy) a.res_copy[(int64_t)p * a.rc_ps + n] = rv;
  }
}

}  // namespace mvr

template <typename T>
static int procrustes_launch(const T* x1, const T* x2, int64_t x_pstride, int64_t x_nstride, T* w, int64_t w_pstride,
                             const int32_t* guard_pos, T* w_copy, int64_t wc_pstride, int P, int N, int normalize,
                             T eps, T* R, T* t, T* res, int64_t res_pstride, T* res_copy, int64_t rc_pstride,
                             int32_t* status, int guard_group, hipStream_t stream) {
  if (P < 0 || N < 0 || guard_group < 0) return MVR_EINVAL;
  if (P == 0) return MVR_OK;
  if ((N > 0 && (!x1 || !x2)) || !R || !t) return MVR_EINVAL;
  if (guard_pos && N > 0 && !w) return MVR_EINVAL;
  mvr::ProcrustesArgs<T> a{x1, x2, x_pstride, x_nstride, w, w_pstride, guard_pos, w_copy, wc_pstride,
                           P, N, normalize, eps, guard_group, R, t, res, res_pstride, res_copy, rc_pstride, status};
  mvr::ProfScope prof(mvr::PK_PROCRUSTES, 40.0 * P * N, (double)P * N * sizeof(T) * 8, stream);
  hipLaunchKernelGGL(mvr::procrustes_kernel<T>, dim3(P), dim3(256), 0, stream, a);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}

extern "C" int mvr_procrustes(const float* x1, const float* x2, int64_t x_pstride, int64_t x_nstride, float* w,
                              int64_t w_pstride, const int32_t* guard_pos, float* w_copy, int64_t wc_pstride, int P,
                              int N, int normalize, float eps, float* R, float* t, float* res, int64_t res_pstride,
                              float* res_copy, int64_t rc_pstride, int32_t* status, int guard_group,
                              hipStream_t stream) {
  return procrustes_launch<float>(x1, x2, x_pstride, x_nstride, w, w_pstride, guard_pos, w_copy, wc_pstride, P, N,
                                  normalize, eps, R, t, res, res_pstride, res_copy, rc_pstride, status, guard_group,
                                  stream);
}

extern "C" int mvr_procrustes_f64(const double* x1, const double* x2, int64_t x_pstride, int64_t x_nstride, double* w,
                                  int64_t w_pstride, const int32_t* guard_pos, double* w_copy, int64_t wc_pstride,
                                  int P, int N, int normalize, double eps, double* R, double* t, double* res,
                                  int64_t res_pstride, double* res_copy, int64_t rc_pstride, int32_t* status,
                                  int guard_group, hipStream_t stream) {
  return procrustes_launch<double>(x1, x2, x_pstride, x_nstride, w, w_pstride, guard_pos, w_copy, wc_pstride, P, N,
                                   normalize, eps, R, t, res, res_pstride, res_copy, rc_pstride, status, guard_group,
                                   stream);
}
