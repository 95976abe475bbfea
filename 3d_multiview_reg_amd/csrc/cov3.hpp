// The sums over rindex.hpp's ball_walk that its per-point kernels share: a ball's covariance and the 3 x 3 symmetric
// Jacobi eigen-solver (normals.hip: with eigenvectors, iss.hip: without), and the tangent-plane sums of the colour
// gradients (color_grad.hip).  fp64, registers only; every loop is bounded (ball_walk's, the Jacobi sweep cap).
#pragma once
#include "common.hpp"
#include "rindex.hpp"
#include <math.h>

namespace mvr {

// One Jacobi rotation of the symmetric a that zeroes a[P][Q]; R is the third index.  V <- V J (kVectors only: the
// rotation of a never reads V, so the eigenvalues are the same bits with and without it).
template <int P, int Q, int R, bool kVectors>
__device__ __forceinline__ void sym_rotate(double (&a)[3][3], double (&V)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0 || fabs(apq) <= 1e-17 * (fabs(a[P][P]) + fabs(a[Q][Q]))) return;
  const double th = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
  if (kVectors) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double vp = V[i][P], vq = V[i][Q];
      V[i][P] = c * vp - s * vq;
      V[i][Q] = s * vp + c * vq;
    }
  }
}

template <bool kVectors>
__device__ __forceinline__ void jacobi_sweeps3(double (&a)[3][3], double (&V)[3][3]) {
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (!(off > 1e-17 * (fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2])))) break;
    sym_rotate<0, 1, 2, kVectors>(a, V);
    sym_rotate<0, 2, 1, kVectors>(a, V);
    sym_rotate<1, 2, 0, kVectors>(a, V);
  }
}

// The symmetric (two-sided) form of svd3.hpp's cyclic Jacobi: eigenvalues on the diagonal of a, eigenvectors in the
// columns of V.  Zero off-diagonals are left alone, so a zero row and column keep their axis exactly.
__device__ __forceinline__ void jacobi_eig3(double (&a)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  jacobi_sweeps3<true>(a, V);
}

// the eigenvalues alone, the bits jacobi_eig3 leaves on the diagonal of a
__device__ __forceinline__ void jacobi_eigvals3(double (&a)[3][3]) {
  double V[3][3];   // never touched
  jacobi_sweeps3<false>(a, V);
}

// The sums over the ball of `radius` around p within fragment b, in coordinates relative to p (the covariance
// cancels at the size of the ball, not of the scene): n points, m = sum e, S = sum e e^T as xx xy xz yy yz zz.
__device__ __forceinline__ void ball_sums(const RIndex& ix, const double* __restrict__ xyz, int b,
                                          const double (&p)[3], double r, double radius, int& n, double (&m)[3],
                                          double (&S)[6]) {
  int k = 0;
  double sm[3] = {0.0, 0.0, 0.0}, sS[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t, int, double ex, double ey, double ez) {
    ++k;
    sm[0] += ex; sm[1] += ey; sm[2] += ez;
    sS[0] += ex * ex; sS[1] += ex * ey; sS[2] += ex * ez;
    sS[3] += ey * ey; sS[4] += ey * ez; sS[5] += ez * ez;
  });
  n = k;
  for (int e = 0; e < 3; ++e) m[e] = sm[e];
  for (int e = 0; e < 6; ++e) S[e] = sS[e];
}

// The walk of the same ball with a per-neighbour value (color_grad.hip): with e = x_j - p and u = e - (e . nv) nv its
// part in the tangent plane of the normal nv, n points, A = sum u u^T as xx xy xz yy yz zz and h = sum u (f(j) - f0),
// in the walk's order.  value(j) is row j's scalar, f0 the point's own (whose row adds u = 0 and a difference of 0).
template <class F>
__device__ __forceinline__ void ball_tangent_sums(const RIndex& ix, const double* __restrict__ xyz, int b,
                                                  const double (&p)[3], const double (&nv)[3], double f0, double r,
                                                  double radius, F&& value, int& n, double (&A)[6], double (&h)[3]) {
  int k = 0;
  double sA[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sh[3] = {0.0, 0.0, 0.0};
  ball_walk(ix, xyz, b, p, r, radius, [&](int64_t t, int, double ex, double ey, double ez) {
    ++k;
    const double en = ex * nv[0] + ey * nv[1] + ez * nv[2];
    const double ux = ex - en * nv[0], uy = ey - en * nv[1], uz = ez - en * nv[2];
    const double df = value(t) - f0;
    sA[0] += ux * ux; sA[1] += ux * uy; sA[2] += ux * uz;
    sA[3] += uy * uy; sA[4] += uy * uz; sA[5] += uz * uz;
    sh[0] += ux * df; sh[1] += uy * df; sh[2] += uz * df;
  });
  n = k;
  for (int e = 0; e < 6; ++e) A[e] = sA[e];
  for (int e = 0; e < 3; ++e) h[e] = sh[e];
}

// a = S / n - (m / n)(m / n)^T, the covariance about the ball's own mean; m becomes the mean.  n >= 1.
__device__ __forceinline__ void ball_covariance(int n, double (&m)[3], const double (&S)[6], double (&a)[3][3]) {
  const double inv = 1.0 / (double)n;
  for (int e = 0; e < 3; ++e) m[e] *= inv;
  a[0][0] = S[0] * inv - m[0] * m[0];
  a[0][1] = a[1][0] = S[1] * inv - m[0] * m[1];
  a[0][2] = a[2][0] = S[2] * inv - m[0] * m[2];
  a[1][1] = S[3] * inv - m[1] * m[1];
  a[1][2] = a[2][1] = S[4] * inv - m[1] * m[2];
  a[2][2] = S[5] * inv - m[2] * m[2];
}

}  // namespace mvr
