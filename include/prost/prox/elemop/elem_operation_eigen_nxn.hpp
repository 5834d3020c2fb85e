// prost/prox/elemop/elem_operation_eigen_nxn.hpp -- prox of a function of the eigenvalues of a symmetric n x n matrix, n <= 32.
//
// Plugin contract of the reference's include/prost/prox/elemop/elem_operation_eigen_nxn.hpp:
// ElemOperationEigenNxN<T, FUN_1D> : ElemOperation<0, 7>.  A group is a row-major n x n matrix M (dim = n^2); it is symmetrised
// as (M + M^T) / 2 = V diag(l) V^T, and the result is V diag(p) V^T with both triangles written, p = the prox of
// c f(a t - b) + d t + (e/2) t^2  at each eigenvalue (spectral_common.hpp, including its `a == 0 || c == 0` branch).  The step is
// tau_scal * tau_diag[0].  The decomposition is two-sided Jacobi in fp64 -- no tridiagonalisation, no QL iteration.
//
// Two forms:
//   * EigenNApply<T, N>: N a compile-time constant, cyclic order, the matrix in registers (SymEigN).  The built-in names run it
//     for n <= 5, one matrix per lane (prost_amd/csrc/kernels_prox_spectral.hip).
//   * EigenNxNApply<T>: n a run-time value, round-robin order (the rotations of a round are disjoint: RoundRobinPair), A and V^T in
//     local arrays of 2 x 8 KiB.  This is what the functor ElemOperationEigenNxN runs: it is the source-compatible form for plugins
//     and the host, and THE SLOW ONE on the device, where the local arrays are scratch memory.  The built-in names do not use it:
//     for n >= 6 they run the same rounds with several lanes per matrix and A, V^T in LDS (kernels_prox_eigen_nxn.hip).
#ifndef PROST_PROX_ELEMOP_ELEM_OPERATION_EIGEN_NXN_HPP_
#define PROST_PROX_ELEMOP_ELEM_OPERATION_EIGEN_NXN_HPP_
#include "prost/prox/elemop/spectral_common.hpp"

namespace prost {
namespace elemop {

/// n in 1 .. kEigenNxNMax with n * n == dim, or 0 when there is none (at most kEigenNxNMax steps whatever dim is)
__host__ __device__ __forceinline__ int EigenNxNSide(size_t dim) {
  for (int n = 1; n <= kEigenNxNMax; n++)
    if ((size_t)(n * n) == dim) return n;
  return 0;
}

template <class T, int N, class RES, class ARG, class FUN_1D>
__host__ __device__ __forceinline__ void EigenNApply(RES& res, const ARG& arg, double tau, const T* coeffs, const FUN_1D& fun) {
  double a[N][N], v[N][N], l[N];
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = i; j < N; j++) a[i][j] = ((double)arg[i * N + j] + (double)arg[j * N + i]) / 2.;
  SymEigN<N>(a, v);
#pragma unroll
  for (int i = 0; i < N; i++) l[i] = a[i][i];
  SpectralProx1D(l, tau, SpectralCoeffs<T>(coeffs), fun);
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = i; j < N; j++) {
      double t = 0.;
#pragma unroll
      for (int k = 0; k < N; k++) t += v[i][k] * v[j][k] * l[k];
      res[i * N + j] = (T)t;
      res[j * N + i] = (T)t;
    }
}

/// run-time n (1 <= n <= kEigenNxNMax); `sweeps`, if given, receives the number of sweeps that ran
template <class T, class RES, class ARG, class FUN_1D>
__host__ __device__ inline void EigenNxNApply(RES& res, const ARG& arg, int n, double tau, const T* coeffs, const FUN_1D& fun, int* sweeps = nullptr) {
  const int m = n + (n & 1), half = m / 2;               // an odd n plays with a bye: row and column n are zero, V^T[n][n] = 1
  double A[kEigenNxNMax * kEigenNxNMax], Vt[kEigenNxNMax * kEigenNxNMax], cs[kEigenNxNMax];
  for (int i = 0; i < m; i++)
    for (int j = 0; j < m; j++) {
      A[i * m + j] = i < n && j < n ? ((double)arg[i * n + j] + (double)arg[j * n + i]) / 2. : 0.;
      Vt[i * m + j] = i == j ? 1. : 0.;
    }
  int sweep = 0;
  for (; sweep < kJacobiSweepsNxN; sweep++) {
    double off = 0., diag = 0.;
    for (int i = 0; i < m; i++)
      for (int j = 0; j < m; j++) (i == j ? diag : off) += t_abs(A[i * m + j]);
    if (JacobiConverged(diag, off)) break;
    for (int round = 0; round < m - 1; round++) {
      for (int k = 0; k < half; k++) {
        int p, q;
        double t;
        RoundRobinPair(m, round, k, p, q);
        JacobiAngle(A[p * m + p], A[q * m + q], A[p * m + q], cs[2 * k], cs[2 * k + 1], t);
      }
      for (int k = 0; k < half; k++) {
        int pk, qk;
        RoundRobinPair(m, round, k, pk, qk);
        for (int l = 0; l < half; l++) {
          int pl, ql;
          RoundRobinPair(m, round, l, pl, ql);
          JacobiBlock(cs[2 * k], cs[2 * k + 1], cs[2 * l], cs[2 * l + 1], A[pk * m + pl], A[pk * m + ql], A[qk * m + pl], A[qk * m + ql]);
          if (k == l) A[pk * m + ql] = A[qk * m + pl] = 0.;          // the annihilated pair: exact zeros
        }
        for (int j = 0; j < m; j++) {
          const double x = Vt[pk * m + j], y = Vt[qk * m + j];
          Vt[pk * m + j] = cs[2 * k] * x - cs[2 * k + 1] * y;
          Vt[qk * m + j] = cs[2 * k + 1] * x + cs[2 * k] * y;
        }
      }
    }
  }
  if (sweeps) *sweeps = sweep;
  const SpectralCoeffs<T> co(coeffs);
  for (int k = 0; k < n; k++) {
    double l[1] = {A[k * m + k]};
    SpectralProx1D(l, tau, co, fun);
    cs[k] = l[0];
  }
  for (int i = 0; i < n; i++)
    for (int j = i; j < n; j++) {
      double t = 0.;
      for (int k = 0; k < n; k++) t += Vt[k * m + i] * Vt[k * m + j] * cs[k];
      res[i * n + j] = (T)t;
      res[j * n + i] = (T)t;
    }
}

}  // namespace elemop

template <typename T, class FUN_1D>
struct ElemOperationEigenNxN : public ElemOperation<0, 7> {
  static const bool kWritesAllComponents = true;
  __host__ __device__ ElemOperationEigenNxN(T* coeffs, size_t dim, SharedMem<SharedMemType, GetSharedMemCount>& /*shared_mem*/)
      : coeffs_(coeffs), n_(elemop::EigenNxNSide(dim)) {}

  /// dim has to be n^2 with 1 <= n <= 32 (the factory checks it for the built-in names); any other dim leaves res untouched
  __host__ __device__ inline void operator()(Vector<T>& res, const Vector<const T>& arg, const Vector<const T>& tau_diag, T tau_scal, bool invert_tau) {
    if (n_ < 1 || n_ > elemop::kEigenNxNMax) return;
    elemop::EigenNxNApply<T>(res, arg, n_, elemop::SpectralStep(tau_scal, tau_diag[0], invert_tau), coeffs_, FUN_1D());
  }

 private:
  T* coeffs_;
  int n_;
};

}  // namespace prost
#endif
