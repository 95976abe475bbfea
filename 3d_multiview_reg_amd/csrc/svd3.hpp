// 3 x 3 SVD by one-sided Jacobi in fp64 and the 3 x 3 determinant, shared by the Procrustes / RANSAC kernels
// (procrustes.hip, ransac.hip), the ICP solve (icp.hip) and the pose synchronisation (sync.hip).
//
// H = U diag(S) V^T, S descending, V orthogonal; U's columns of singular values <= 1e-13 S[0] are completed (rank
// 1: a unit vector orthogonal to u0; rank <= 2: u2 = u0 x u1), so U is orthogonal to rounding at every rank; the
// zero matrix gives U = V = I.  Every threshold is relative to the matrix (|ga| <= 1e-15 sqrt(al be), tiny =
// 1e-13 S[0]): scaling H by a power of two scales S and leaves U, V bit for bit — as long as al * be, a product of
// two squared column norms, neither overflows nor underflows: entries within about 2^-250 .. 2^250.  Beyond that
// the result is out of contract.  A column that an exactly rank-deficient matrix drives to zero keeps being rotated
// (it shrinks by ~1e-16 per sweep, never orthogonal RELATIVE to its own norm) until it underflows or the 30 sweeps
// are over; the result is the same (tests/test_gpu_procrustes.py, the zero-row matrices).
#pragma once
#include "common.hpp"
#include <math.h>

namespace mvr {

__device__ static void jacobi_svd3(const double H[3][3], double U[3][3], double S[3], double V[3][3]) {
  double a[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { a[i][j] = H[i][j]; V[i][j] = (i == j) ? 1.0 : 0.0; }
  const int pp[3] = {0, 0, 1}, qq[3] = {1, 2, 2};
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int r = 0; r < 3; ++r) {
      const int p = pp[r], q = qq[r];
      double al = 0, be = 0, ga = 0;
      for (int i = 0; i < 3; ++i) { al += a[i][p] * a[i][p]; be += a[i][q] * a[i][q]; ga += a[i][p] * a[i][q]; }
      if (ga == 0.0) continue;
      const double nrm = sqrt(al * be);
      if (fabs(ga) <= 1e-15 * nrm) continue;
      off = fmax(off, fabs(ga) / nrm);
      const double ze = (be - al) / (2.0 * ga);
      const double tt = (ze >= 0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
      const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
      for (int i = 0; i < 3; ++i) {
        const double ap = a[i][p], aq = a[i][q];
        a[i][p] = c * ap - s * aq; a[i][q] = s * ap + c * aq;
        const double vp = V[i][p], vq = V[i][q];
        V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
      }
    }
    if (off < 1e-15) break;
  }
  for (int j = 0; j < 3; ++j) S[j] = sqrt(a[0][j] * a[0][j] + a[1][j] * a[1][j] + a[2][j] * a[2][j]);
  // sort singular values descending (permute columns of a and V together)
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (S[j] < S[j + 1]) {
        double tmp = S[j]; S[j] = S[j + 1]; S[j + 1] = tmp;
        for (int k = 0; k < 3; ++k) {
          tmp = a[k][j]; a[k][j] = a[k][j + 1]; a[k][j + 1] = tmp;
          tmp = V[k][j]; V[k][j] = V[k][j + 1]; V[k][j + 1] = tmp;
        }
      }
  if (!(S[0] > 0.0)) {  // zero matrix: LAPACK (torch.svd) returns U = V = I
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) { U[i][j] = (i == j) ? 1.0 : 0.0; V[i][j] = U[i][j]; }
    return;
  }
  const double tiny = S[0] * 1e-13;
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) U[i][j] = (S[j] > tiny) ? a[i][j] / S[j] : 0.0;
  if (!(S[1] > tiny)) {  // rank 1: any unit vector orthogonal to u0
    const double x = U[0][0], y = U[1][0], z = U[2][0];
    double e[3];
    if (fabs(x) <= fabs(y) && fabs(x) <= fabs(z)) { e[0] = 0; e[1] = -z; e[2] = y; }
    else if (fabs(y) <= fabs(z)) { e[0] = -z; e[1] = 0; e[2] = x; }
    else { e[0] = -y; e[1] = x; e[2] = 0; }
    const double n = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    for (int i = 0; i < 3; ++i) U[i][1] = e[i] / n;
  }
  if (!(S[2] > tiny)) {  // rank <= 2: u2 = u0 x u1
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
}

__device__ static double det3(const double M[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

}  // namespace mvr
