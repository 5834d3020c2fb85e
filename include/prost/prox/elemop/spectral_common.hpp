// prost/prox/elemop/spectral_common.hpp -- what the spectral operations (elem_operation_singular_nx2.hpp,
// elem_operation_eigen_2x2.hpp, elem_operation_eigen_3x3.hpp, elem_operation_eigen_nxn.hpp, elem_operation_mass_norm.hpp) share: the
// scalar prox convention on a singular value or an eigenvalue, the symmetric 2x2 / 3x3 / N x N eigendecompositions, and the parts
// of the n x n Jacobi that do not depend on how many lanes share a matrix.
//
// Everything here is fp64 whatever the data type is: the reference decomposes in double for float and double data alike
// (elem_operation_eigen_3x3.hpp:306-325 there), and so do these.  The decompositions are Jacobi rotations, not the
// reference's closed forms: a 2x2 symmetric matrix is diagonalised by ONE rotation, a 3x3 one by cyclic sweeps of three.
// A rotation never divides by a difference of eigenvalues, so close or equal eigenvalues cost no accuracy (Cardano's
// formula loses about half the digits there), there are no trigonometric functions, and the code is straight-line
// register arithmetic: no arrays indexed at run time, nothing that lands in scratch memory.
//
// The same functions run inside the library's own kernel (prost_amd/csrc/kernels_prox_spectral.hip), so a plugin that
// composes them computes what the built-in names compute.
#ifndef PROST_PROX_ELEMOP_SPECTRAL_COMMON_HPP_
#define PROST_PROX_ELEMOP_SPECTRAL_COMMON_HPP_
#include "prost/prox/elemop/elem_operation_1d.hpp"

namespace prost {
namespace elemop {

/// step size of a group as the spectral operations of the reference form it: the product in T, the reciprocal in double
template <class T>
__host__ __device__ __forceinline__ double SpectralStep(T tau_scal, T tau_diag, bool invert_tau) {
  const double t = (double)(tau_scal * tau_diag);
  return invert_tau ? 1. / t : t;
}

/// the seven coefficients of a group as doubles
template <class T>
struct SpectralCoeffs {
  double a, b, c, d, e, alpha, beta;
  __host__ __device__ __forceinline__ explicit SpectralCoeffs(const T* k)
      : a((double)k[0]), b((double)k[1]), c((double)k[2]), d((double)k[3]), e((double)k[4]), alpha((double)k[5]), beta((double)k[6]) {}
};

/// prox of  h(t) = c f(a t - b) + d t + (e/2) t^2  at each of v[0..N) -- the convention of elem_operation_1d.hpp, including its
/// `a == 0 || c == 0` branch.  `fun(x0, step, alpha, beta)` is the scalar prox of f (a Function1D*, or any callable).
template <int N, class C, class FUN_1D>
__host__ __device__ __forceinline__ void SpectralProx1D(double (&v)[N], double tau, const C& k, const FUN_1D& fun) {
  const double den = 1. + tau * k.e;
  if (k.a == 0 || k.c == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = (v[i] - tau * k.d) / den;
  } else {
    const double step = k.c * k.a * k.a * tau / den;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const double x0 = k.a * (v[i] - k.d * tau) / den - k.b;
      v[i] = ((double)fun(x0, step, k.alpha, k.beta) + k.b) / k.a;
    }
  }
}

/// The Jacobi rotation in the (p, q) plane that annihilates a_pq of a symmetric matrix: returns (c, s, t) with t = tan of the angle,
/// |t| <= 1 (the smaller root, the stable one).  a_pq == 0 gives the identity.
__host__ __device__ __forceinline__ void JacobiAngle(double app, double aqq, double apq, double& c, double& s, double& t) {
  c = 1.;
  s = t = 0.;
  if (apq != 0.) {
    const double theta = (aqq - app) / (2. * apq);      // |theta| beyond 1e154: theta^2 overflows to inf and t becomes 0 -- the limit
    const double r = 1. / (t_abs(theta) + t_sqrt(theta * theta + 1.));
    t = theta < 0. ? -r : r;
    c = 1. / t_sqrt(t * t + 1.);
    s = t * c;
  }
}

/// [a b; b d] = [c s; -s c] diag(l1, l2) [c -s; s c]: the eigenvectors are (c, -s) for l1 and (s, c) for l2 (not ordered)
__host__ __device__ __forceinline__ void SymEig2x2(double a, double b, double d, double& l1, double& l2, double& c, double& s) {
  double t;
  JacobiAngle(a, d, b, c, s, t);
  l1 = a - t * b;
  l2 = d + t * b;
}

/// one rotation of a 3x3 sweep: plane (p, q), r the third index; vXp / vXq are rows X of the eigenvector columns p and q
__host__ __device__ __forceinline__ void JacobiRotate3(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                                       double& v1p, double& v1q, double& v2p, double& v2q) {
  double c, s, t;
  JacobiAngle(app, aqq, apq, c, s, t);
  app -= t * apq;
  aqq += t * apq;
  apq = 0.;
  double x = arp, y = arq;
  arp = c * x - s * y; arq = s * x + c * y;
  x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
  x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
  x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
}

/// Symmetric 3x3 eigendecomposition by cyclic Jacobi sweeps.  In: the upper triangle.  Out: w[j] and the columns v[.][j] with
/// A = V diag(w) V^T (not ordered).  The off-diagonal mass falls quadratically from sweep to sweep: random matrices are at
/// rounding level after 4 sweeps; the loop leaves as soon as a sweep finds nothing left next to the diagonal, and at most
/// kJacobiSweeps run (the remaining off-diagonal part, if any, is then far below 1e-16 of the matrix).
constexpr int kJacobiSweeps = 8;
__host__ __device__ __forceinline__ void SymEig3x3(double a00, double a01, double a02, double a11, double a12, double a22, double (&w)[3], double (&v)[3][3]) {
  double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    const double off = t_abs(a01) + t_abs(a02) + t_abs(a12);
    const double diag = t_abs(a00) + t_abs(a11) + t_abs(a22);
    if (diag + off == diag) break;                        // also the zero matrix, and NaNs fall through all sweeps harmlessly
    JacobiRotate3(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
    JacobiRotate3(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
    JacobiRotate3(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
  }
  w[0] = a00; w[1] = a11; w[2] = a22;
  v[0][0] = v00; v[0][1] = v01; v[0][2] = v02;
  v[1][0] = v10; v[1][1] = v11; v[1][2] = v12;
  v[2][0] = v20; v[2][1] = v21; v[2][2] = v22;
}

// ---- n x n (elem_operation_eigen_nxn.hpp, elem_operation_mass_norm.hpp, prost_amd/csrc/kernels_prox_eigen_nxn.hip) ----------------
// What does not depend on how many lanes share a matrix is written once here: the rotation angle (JacobiAngle above), the order
// in which the planes are visited (RoundRobinPair), the convergence test of a sweep (JacobiConverged), the two-sided update of
// a 2x2 block (JacobiBlock) and the scalar prox (SpectralProx1D above).

/// largest n of eigen_nxn (sum_eigen_nxn.m:5)
constexpr int kEigenNxNMax = 32;
/// Sweep cap of the n x n decompositions.  Parallel-ordered Jacobi needed at most 8 sweeps to pass JacobiConverged on the parity
/// inputs and the special matrices up to n = 32 (docs/rounds/r11.md); the cap is twice that.  Every sweep loop is a `for` up to
/// this constant, so NaN or Inf input ends after kJacobiSweepsNxN sweeps.
constexpr int kJacobiSweepsNxN = 16;

/// a sweep is skipped, and the decomposition ends, when the off-diagonal part no longer changes the diagonal sum (both sums of
/// absolute values over the matrix).  True for the zero matrix; false whenever a NaN is involved.
__host__ __device__ __forceinline__ bool JacobiConverged(double diag, double off) { return diag + off == diag; }

/// Round-robin (circle method) schedule for even m: in round 0..m-2, slot 0..m/2-1 names the pair p < q; the m/2 pairs of a round
/// are disjoint, and the m-1 rounds hold every unordered pair of 0..m-1 exactly once.  An odd n plays with m = n + 1: the pair
/// that holds index n is a bye.  No division: the indices are reduced by conditional subtraction.
__host__ __device__ __forceinline__ void RoundRobinPair(int m, int round, int slot, int& p, int& q) {
  const int r = m - 1;
  int a = r, b = round;
  if (slot != 0) {
    a = round + slot;
    if (a >= r) a -= r;
    b = round - slot;
    if (b < 0) b += r;
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

/// B <- J_k^T B J_l for the 2x2 block B = [x00 x01; x10 x11] whose rows are the pair k and whose columns are the pair l of a round,
/// J = [c s; -s c] as JacobiAngle returns it
__host__ __device__ __forceinline__ void JacobiBlock(double ck, double sk, double cl, double sl, double& x00, double& x01, double& x10, double& x11) {
  const double y00 = ck * x00 - sk * x10, y01 = ck * x01 - sk * x11;
  const double y10 = sk * x00 + ck * x10, y11 = sk * x01 + ck * x11;
  x00 = cl * y00 - sl * y01; x01 = sl * y00 + cl * y01;
  x10 = cl * y10 - sl * y11; x11 = sl * y10 + cl * y11;
}

/// Symmetric N x N eigendecomposition, N a compile-time constant: cyclic Jacobi like SymEig3x3, every index a constant after
/// unrolling, so the matrix lives in registers.  In: the upper triangle of a (i <= j).  Out: a[j][j] the eigenvalues and the columns
/// v[.][j] with A = V diag V^T (not ordered); the strict upper triangle is left at rounding level, the lower one is never touched.
/// Returns the number of sweeps that ran.
template <int N>
__host__ __device__ __forceinline__ int SymEigN(double (&a)[N][N], double (&v)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) v[i][j] = i == j ? 1. : 0.;
  int sweep = 0;
#pragma unroll 1
  for (; sweep < kJacobiSweepsNxN; sweep++) {
    double off = 0., diag = 0.;
#pragma unroll
    for (int i = 0; i < N; i++) {
      diag += t_abs(a[i][i]);
#pragma unroll
      for (int j = i + 1; j < N; j++) off += t_abs(a[i][j]);
    }
    if (JacobiConverged(diag, off)) break;
#pragma unroll
    for (int p = 0; p < N - 1; p++) {
#pragma unroll
      for (int q = p + 1; q < N; q++) {
        double c, s, t;
        JacobiAngle(a[p][p], a[q][q], a[p][q], c, s, t);
        a[p][p] -= t * a[p][q];
        a[q][q] += t * a[p][q];
        a[p][q] = 0.;
#pragma unroll
        for (int r = 0; r < N; r++) {
          if (r != p && r != q) {
            double& x = r < p ? a[r][p] : a[p][r];
            double& y = r < q ? a[r][q] : a[q][r];
            const double xx = x, yy = y;
            x = c * xx - s * yy;
            y = s * xx + c * yy;
          }
          const double vp = v[r][p], vq = v[r][q];
          v[r][p] = c * vp - s * vq;
          v[r][q] = s * vp + c * vq;
        }
      }
    }
  }
  return sweep;
}

}  // namespace elemop
}  // namespace prost
#endif
